#!/usr/bin/env python3
"""The inputs of two learnt MAPF policies, each written by one launch of policy_input(): SCRIMP's eight planes
(obstacles, agents, own goal, other agents' goals, then the four direction-to-goal planes) and PRIMAL's four (the first
four of them).  Nothing is assembled in torch and nothing goes through the host.  Each step checks the eight planes
against what a user had to build before: torch.cat of observe(), the `other_goals` plane of the CPU reference
(tests/policy_input_reference.py, computed from get_state()) and goal_directions().

    python examples/scrimp_input.py [--envs 64] [--agents 16] [--size 24] [--steps 16] [--dtype float32]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402
from policy_input_reference import other_goals_reference  # noqa: E402

SCRIMP = ("obstacles", "agents", "target", "other_goals", "up", "down", "left", "right")
PRIMAL = SCRIMP[:4]


def composed(env):
    """The eight planes the old way: three calls, a CPU loop for the plane the engine did not have, and a copy."""
    st = env.get_state()
    goals = other_goals_reference(st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                                  st["is_active"].cpu().numpy(), env.obs_radius)
    goals = torch.as_tensor(goals, device=env.device).to(torch.float32).unsqueeze(2)
    return torch.cat((env.observe(), goals, env.goal_directions()), dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--agents", type=int, default=16)
    ap.add_argument("--size", type=int, default=24)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--dtype", default="float32", choices=("float32", "float16", "bfloat16", "uint8"))
    args = ap.parse_args()

    r = 4
    dtype = getattr(torch, args.dtype)
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                    on_target="restart", max_episode_steps=256)
    env = VecPogema(gc, batch=args.envs, auto_reset=True)
    env.reset(seed=0)
    w = 2 * r + 1
    x8 = torch.empty((args.envs, args.agents, 8, w, w), dtype=dtype, device=env.device)
    x4 = torch.empty((args.envs, args.agents, 4, w, w), dtype=dtype, device=env.device)
    goal_cells = 0.0
    for t in range(args.steps):
        env.policy_input(channels=SCRIMP, dtype=dtype, out=x8)   # SCRIMP's policy(x8) goes here
        env.policy_input(channels=PRIMAL, dtype=dtype, out=x4)   # PRIMAL's policy(x4) goes here
        if not torch.equal(x8, composed(env).to(dtype)):
            raise SystemExit(f"step {t}: policy_input() differs from observe() + other_goals + goal_directions()")
        if not torch.equal(x4, x8[:, :, :4]):
            raise SystemExit(f"step {t}: the four PRIMAL planes are not the first four SCRIMP planes")
        goal_cells += float(x8[:, :, 3].sum())
        actions, _ = env.expert_actions()
        env.step(actions)
    print("SCRIMP input", tuple(x8.shape), x8.dtype, "and PRIMAL input", tuple(x4.shape), "on", x8.device)
    print(f"{goal_cells / (args.steps * args.envs * args.agents):.2f} other agents' goals per window on average; "
          f"all {args.steps} steps matched the composition")
    env.close()


if __name__ == "__main__":
    main()
