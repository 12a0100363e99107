#!/usr/bin/env python
"""Collision shielding (shield_actions(), docs/SPEC.md S15) around a stand-in policy, next to the same policy unshielded.

The "policy" scores the four moves by goal_directions()' centre cell (1 where the move leads closer to the target) and
samples with Gumbel noise: `scores = logits + gumbel` taken in descending order is Plackett-Luce sampling without
replacement, so the shield stays deterministic and the caller owns the randomness.  One rollout steps the raw argmax of
the sampled scores, one steps the shielded actions; both under collision_system="soft", on seeded twin instances.

    python examples/shielded_policy.py [--envs 256] [--agents 32] [--size 16] [--density 0.2] [--steps 64]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402

MOVES = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))


def sampled_scores(env, gen, temperature):
    """[batch, agents, 5] float32: logits (2 for a move towards the target, 0 otherwise) plus Gumbel noise."""
    r = env.window // 2
    towards = env.goal_directions(format="float32")[:, :, :, r, r]                 # [B, A, 4]
    logits = torch.cat([torch.zeros_like(towards[..., :1]), 2.0 * towards], dim=-1)
    u = torch.rand(logits.shape, generator=gen, device=env.device).clamp_(1e-9, 1.0 - 1e-7)
    return logits / temperature - torch.log(-torch.log(u))


def rollout(gc, args, shielded):
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    env.reset(seed=args.seed)
    policy = PibtPolicy(env)
    gen = torch.Generator(device=env.device).manual_seed(args.seed)        # the same noise in both rollouts
    moves = torch.tensor(MOVES, dtype=torch.int32, device=env.device)
    reverted = torch.zeros((), dtype=torch.int64, device=env.device)
    overridden = torch.zeros((), dtype=torch.float64, device=env.device)
    planned = torch.zeros((), dtype=torch.int64, device=env.device)
    for _ in range(args.steps):
        scores = sampled_scores(env, gen, args.temperature)
        before = env.get_state()
        active = before["is_active"]
        if shielded:
            actions, _, o = policy.act(scores=scores)
            overridden += o[active].sum()
        else:
            actions = scores.argmax(dim=-1)
        out = env.step(actions)
        policy.update(out[1], out[4]["episode_done"])
        intended = before["agents_xy"] + moves[actions]
        reverted += ((env.get_state()["agents_xy"] != intended).any(-1) & active).sum()
        planned += active.sum()
    finished = int((~env.get_state()["is_active"]).sum())
    env.close()
    return int(reverted) / args.steps, finished, float(overridden) / max(int(planned), 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    gc = GridConfig(size=args.size, num_agents=args.agents, density=args.density, obs_radius=5, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps)
    total = args.envs * args.agents
    for name, shielded in (("raw samples", False), ("shielded", True)):
        reverted, finished, overridden = rollout(gc, args, shielded)
        print(f"{name:12s} reverted moves per step {reverted:9.1f}   finished agents {finished:6d} / {total}   "
              f"mean overridden {overridden:.4f}")


if __name__ == "__main__":
    main()
