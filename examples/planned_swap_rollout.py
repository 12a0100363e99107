#!/usr/bin/env python3
"""Planner-driven episodes in chunks with the swap operation inside the lookahead: PibtPolicy.plan(K, swap=True) looks K
steps ahead in one launch (pibt_plan(swap=True), docs/SPEC.md S27), rollout(actions) runs the K steps in one launch, and
the next plan starts from where the rollout ended -- two calls per K steps, on maps where the plain lookahead livelocks.
First the dead-end instance -- agent 0 wants the end of a dead-end corridor, agent 1 stands there and wants out -- then
a pool of small corridor-heavy random maps, every env solved when all its agents have reached their targets
(collision_system "soft", on_target "finish").  Prints steps and solved counts of both plans side by side.

    python examples/planned_swap_rollout.py [--envs 256] [--agents 8] [--size 12] [--density 0.35] [--steps 160] [--horizon 16]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402

DEAD_END = ["#######",
            "##.####",
            ".......",
            "#######"]


def run(env, swap, steps, horizon):
    """Plan-and-rollout chunks of `horizon` steps to the end of the episode.  Returns the steps until every env was
    solved (None: never, counted in whole chunks) and the solved envs, [batch] bool."""
    policy = PibtPolicy(env)
    solved = torch.zeros(env.batch, dtype=torch.bool, device=env.device)
    for t0 in range(0, steps, horizon):
        k = min(horizon, steps - t0)
        actions, _, _ = policy.plan(k, swap=swap)
        out = env.rollout(actions, obs_slots=0)
        # the plan does not know that an episode ended: those envs start over with equal priorities
        policy.priority[out["episode_done"].any(dim=0)] = 0
        solved |= ~env.get_state()["is_active"].any(dim=1)
        if bool(solved.all()):
            return t0 + k, solved
    return None, solved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--size", type=int, default=12)
    ap.add_argument("--density", type=float, default=0.35)
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    obstacles = np.array([[[c == "#" for c in row] for row in DEAD_END]], dtype=np.uint8)
    agents, targets = np.array([[(2, 3), (2, 5)]], dtype=np.int32), np.array([[(2, 6), (2, 0)]], dtype=np.int32)
    for swap in (False, True):
        env = VecPogema(GridConfig(map="\n".join(DEAD_END), num_agents=2, obs_radius=2, seed=0, collision_system="soft",
                                   on_target="finish", max_episode_steps=81), batch=1, auto_reset=False)
        env.reset_from_state(obstacles, agents, targets)
        arrival = env.pibt_plan(9, swap=swap)[2][0].tolist()
        took, _ = run(env, swap, 80, 9)
        print(f"dead end, plan(9, swap={swap}): arrival {arrival}, "
              + (f"solved within {took} steps" if took else "not solved in 80 steps"))
        env.close()

    rng = np.random.default_rng(args.seed)
    pool = (rng.random((32, args.size, args.size)) < args.density).astype(np.uint8)
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=args.density, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps + 1)
    counts = {}
    for swap in (False, True):
        env = VecPogema(gc, batch=args.envs, auto_reset=False, map_pool=torch.as_tensor(pool))
        env.reset(seed=args.seed)
        _, solved = run(env, swap, args.steps, args.horizon)
        counts[swap] = solved.cpu()
        env.close()
    plain, swap = counts[False], counts[True]
    calls = 2 * -(-args.steps // args.horizon)
    print(f"{args.envs} envs from a pool of 32 maps, {args.agents} agents on {args.size}x{args.size}, density "
          f"{args.density}, {args.steps} steps as plan({args.horizon}) + rollout(): at most {calls} calls per plan kind")
    print(f"solved: plain plan {int(plain.sum())}, plan with swap {int(swap.sum())}; lost by swap "
          f"{int((plain & ~swap).sum())}, won by swap {int((swap & ~plain).sum())}")


if __name__ == "__main__":
    main()
