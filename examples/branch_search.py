#!/usr/bin/env python
"""One-step lookahead by branching on the device (copy_envs(), docs/SPEC.md S19), next to the same policy without it.

R root environments live in slots 0, N, 2N, ... of one engine of R * N slots.  Every step each root is copied into the
other N - 1 slots of its group; all N slots (the root is branch 0) get shielded actions sampled with their own Gumbel
noise (shield_actions(), S15) and are stepped; the branch whose agents are closest to their targets -- the lowest sum of
expert_actions()' distances -- wins and is copied back onto the root, with indices computed on the device and
validate=False: no host sync anywhere in the loop.  The distance-field cache travels with the copies, so the queries
after a branch build nothing.  A second engine of R slots runs the same sampled policy from the same instances without
the search; the script prints the roots' mean sum of distances per step for both.

    python examples/branch_search.py [--roots 64] [--branches 8] [--agents 16] [--size 16] [--density 0.2] [--steps 48]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pogema_amd import GridConfig, VecPogema  # noqa: E402


def sampled_actions(env, gen, temperature):
    """Jointly collision-free actions for every slot: logits (2 for a move towards the target) plus Gumbel noise,
    through the shield."""
    r = env.window // 2
    towards = env.goal_directions(format="float32")[:, :, :, r, r]                 # [B, A, 4]
    logits = torch.cat([torch.zeros_like(towards[..., :1]), 2.0 * towards], dim=-1)
    u = torch.rand(logits.shape, generator=gen, device=env.device).clamp_(1e-9, 1.0 - 1e-7)
    actions, _, _ = env.shield_actions(logits / temperature - torch.log(-torch.log(u)))
    return actions


def distance_sum(env):
    """float32 [batch]: the sum over agents of the shortest-path distance to the target (0 for a finished agent)."""
    _, distance = env.expert_actions()
    return distance.clamp(min=0).sum(dim=1).float()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--roots", type=int, default=64)
    ap.add_argument("--branches", type=int, default=8)
    ap.add_argument("--agents", type=int, default=16)
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    R, N = args.roots, args.branches
    gc = GridConfig(size=args.size, num_agents=args.agents, density=args.density, obs_radius=5, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps)
    plain = VecPogema(gc, batch=R, auto_reset=False)
    search = VecPogema(gc, batch=R * N, auto_reset=False)
    state = plain.generate(args.seed)
    plain.reset_from_state(*state)
    search.reset_from_state(*(np.repeat(x, N, axis=0) for x in state))
    dev = search.device
    roots = torch.arange(R, dtype=torch.int32, device=dev) * N                   # slot of each group's root
    branch_src = roots.repeat_interleave(N - 1)
    branch_dst = (roots.view(R, 1) + torch.arange(1, N, dtype=torch.int32, device=dev)).reshape(-1).contiguous()
    gen_p = torch.Generator(device=dev).manual_seed(args.seed)
    gen_s = torch.Generator(device=dev).manual_seed(args.seed + 1)
    search.cost_to_go()                       # allocates the distance-field cache: from here on the copies carry its rows
    built = None
    print(f"{R} roots x {N} branches, {args.agents} agents on {args.size}x{args.size}: mean sum of distances to the targets")
    print("step    plain   search")
    for t in range(args.steps):
        plain.step(sampled_actions(plain, gen_p, args.temperature))
        search.copy_envs(branch_src, branch_dst, validate=False)                 # branch
        search.step(sampled_actions(search, gen_s, args.temperature))
        score = distance_sum(search).view(R, N)
        winner = (roots + score.argmin(dim=1).to(torch.int32)).contiguous()
        search.copy_envs(winner, roots, validate=False)                          # the winner becomes the root
        if t == 0:
            built = search.cost_to_go_builds
        d_plain, d_search = float(distance_sum(plain).mean()), float(distance_sum(search)[roots.long()].mean())
        print(f"{t + 1:4d} {d_plain:8.2f} {d_search:8.2f}")
    done_p = int((~plain.get_state()["is_active"]).sum())
    done_s = int((~search.get_state()["is_active"][roots.long()]).sum())
    print(f"finished agents: plain {done_p} / {R * args.agents}, search {done_s} / {R * args.agents}; distance fields built "
          f"after the first step: {search.cost_to_go_builds - built}")
    plain.close()
    search.close()


if __name__ == "__main__":
    main()
