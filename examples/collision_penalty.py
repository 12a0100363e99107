#!/usr/bin/env python
"""A collision penalty from the engine's own resolver: a random policy under each collision system, the shaped reward
r - lambda * [outcome >= 2] that PRIMAL-style methods train on, and the per-episode collision rates from `counts` --
then the same random scores through shield_actions(), after which no agent collides with another under `soft`.

    python examples/collision_penalty.py [--batch 256] [--agents 16] [--size 12] [--steps 64]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pogema_amd import OUTCOMES, GridConfig, VecPogema  # noqa: E402

OBSTACLE = OUTCOMES.index("OBSTACLE")
AGENT_CODES = [OUTCOMES.index(n) for n in ("SWAP", "OCCUPIED", "FOLLOW", "CONTESTED")]


def episode(env, steps, lam, shielded, gen):
    """One episode of `steps` steps; returns (mean shaped reward, obstacle-collision rate, agent-collision rate)."""
    B, A = env.batch, env.num_agents
    env.reset(seed=7)
    shaped = torch.zeros((), device=env.device)
    totals = torch.zeros(len(OUTCOMES), dtype=torch.int64, device=env.device)
    for _ in range(steps):
        scores = torch.randn((B, A, 5), device=env.device, generator=gen)
        actions = env.shield_actions(scores)[0] if shielded else scores.argmax(dim=-1)
        _, outcome, _, counts = env.move_outcomes(actions)      # before the step: what these actions will do
        _, rewards, _, _, _ = env.step(actions, compute_obs=False)
        shaped += (rewards - lam * (outcome >= OBSTACLE)).mean()
        totals += counts.sum(dim=0)
    acted = max(int(totals.sum()), 1)
    return float(shaped) / steps, int(totals[OBSTACLE]) / acted, int(totals[AGENT_CODES].sum()) / acted


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--agents", type=int, default=16)
    ap.add_argument("--size", type=int, default=12)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--penalty", type=float, default=0.3)
    args = ap.parse_args()
    print(f"{'collision system':<18}{'policy':<10}{'shaped reward':>14}{'obstacle rate':>15}{'agent rate':>12}")
    for collision in ("priority", "block_both", "soft"):
        gc = GridConfig(size=args.size, num_agents=args.agents, density=0.2, obs_radius=3, seed=7,
                        collision_system=collision, on_target="restart", max_episode_steps=args.steps)
        env = VecPogema(gc, batch=args.batch, auto_reset=False)
        for shielded in (False, True):
            gen = torch.Generator(device=env.device).manual_seed(7)
            reward, obstacle, agent = episode(env, args.steps, args.penalty, shielded, gen)
            print(f"{collision:<18}{'shielded' if shielded else 'random':<10}{reward:>14.4f}{obstacle:>15.4f}{agent:>12.4f}")
            if shielded and collision == "soft":
                assert obstacle == 0.0 and agent == 0.0, "the shield's actions collided under soft"
        env.close()


if __name__ == "__main__":
    main()
