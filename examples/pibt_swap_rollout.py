#!/usr/bin/env python3
"""The cooperative planner with and without the swap operation (pibt_actions(swap=True), docs/SPEC.md S23) run to the
end: first the dead-end instance plain PIBT livelocks in -- agent 0 wants the end of a dead-end corridor, agent 1 stands
there and wants out -- then a pool of small random maps, every env solved when all its agents have reached their targets
(collision_system "soft", on_target "finish").  Prints steps and solved counts.

    python examples/pibt_swap_rollout.py [--envs 256] [--agents 8] [--size 12] [--density 0.35] [--steps 150]
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


def run(env, swap, steps):
    """Steps until every env was solved (None: never) and the solved envs, [batch] bool, under PibtPolicy(env, swap)."""
    policy = PibtPolicy(env, swap=swap)
    solved = torch.zeros(env.batch, dtype=torch.bool, device=env.device)
    for t in range(steps):
        actions, _ = policy.act()
        _, rewards, _, _, infos = env.step(actions, compute_obs=False)
        policy.update(rewards, infos["episode_done"])
        solved |= ~env.get_state()["is_active"].any(dim=1)
        if bool(solved.all()):
            return t + 1, solved
    return None, solved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--size", type=int, default=12)
    ap.add_argument("--density", type=float, default=0.35)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    obstacles = np.array([[[c == "#" for c in row] for row in DEAD_END]], dtype=np.uint8)
    agents, targets = np.array([[(2, 3), (2, 5)]], dtype=np.int32), np.array([[(2, 6), (2, 0)]], dtype=np.int32)
    for swap in (False, True):
        env = VecPogema(GridConfig(map="\n".join(DEAD_END), num_agents=2, obs_radius=2, seed=0, collision_system="soft",
                                   on_target="finish", max_episode_steps=80), batch=1, auto_reset=False)
        env.reset_from_state(obstacles, agents, targets)
        took, _ = run(env, swap, 80)
        print(f"dead end, swap={swap}: " + (f"solved in {took} steps" if took else "not solved in 80 steps"))
        env.close()

    rng = np.random.default_rng(args.seed)
    pool = (rng.random((32, args.size, args.size)) < args.density).astype(np.uint8)
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=args.density, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps + 1)
    counts = {}
    for swap in (False, True):
        env = VecPogema(gc, batch=args.envs, auto_reset=False, map_pool=torch.as_tensor(pool))
        env.reset(seed=args.seed)
        _, solved = run(env, swap, args.steps)
        counts[swap] = solved.cpu()
        env.close()
    plain, swap = counts[False], counts[True]
    print(f"{args.envs} envs from a pool of 32 maps, {args.agents} agents on {args.size}x{args.size}, density "
          f"{args.density}, {args.steps} steps")
    print(f"solved: plain PIBT {int(plain.sum())}, with swap {int(swap.sum())}; lost by swap {int((plain & ~swap).sum())}, "
          f"won by swap {int((swap & ~plain).sum())}")


if __name__ == "__main__":
    main()
