#!/usr/bin/env python3
"""The 7-channel input of DHC / DCC / SCRIMP-style policies, assembled on the device: the three observation planes
(obstacles, agents, target) and behind them the four direction-to-goal planes of goal_directions() -- plane a - 1 marks
the window cells from which move a (up, down, left, right) leads closer to the agent's target.  Nothing goes through
the host.  Each step checks the planes against the shortest-path expert: the lowest plane set at the window centre is
expert_actions()' action.

    python examples/direction_planes.py [--envs 1024] [--agents 32] [--size 32] [--steps 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402


def policy_input(env, obs, planes):
    """float32 [B, A, 7, W, W]: the observation, then the four direction planes (written into `planes`)."""
    return torch.cat((obs, env.goal_directions(out=planes)), dim=2)


def centre_action(planes, r):
    """The lowest move whose plane is set at the window centre, 0 when none is: int64 [B, A]."""
    centre = planes[:, :, :, r, r] > 0                           # [B, A, 4]
    first = torch.argmax(centre.to(torch.uint8), dim=2) + 1      # argmax returns the first maximum
    return torch.where(centre.any(dim=2), first, torch.zeros_like(first))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()

    r = 5
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=r, density=0.3, seed=0, collision_system="soft",
                    on_target="restart", max_episode_steps=256)
    env = VecPogema(gc, batch=args.envs, auto_reset=True)
    obs, _ = env.reset(seed=0)
    w = 2 * r + 1
    planes = torch.empty((args.envs, args.agents, 4, w, w), dtype=torch.float32, device=env.device)
    set_cells = torch.zeros((), dtype=torch.float64, device=env.device)
    for _ in range(args.steps):
        x = policy_input(env, obs, planes)                       # your policy(x) goes here
        actions, _ = env.expert_actions()
        if not torch.equal(centre_action(planes, r), actions):
            raise SystemExit("the centre of the direction planes disagrees with expert_actions()")
        set_cells += planes.sum()
        obs = env.step(actions)[0]
    print("policy input", tuple(x.shape), x.dtype, "on", x.device)
    print(f"{float(set_cells) / (args.steps * args.envs * args.agents * w * w):.2f} set direction bits per window cell on "
          f"average; the centre matched expert_actions() on all {args.steps} steps")
    env.close()


if __name__ == "__main__":
    main()
