#!/usr/bin/env python3
"""Follow the on-device cooperative planner (pibt_actions(), PIBT) to the end of an episode and print the individual
success rate (ISR); the shortest-path expert on the same seeded instances is printed next to it.  PibtPolicy keeps the
growing priorities on the device; nothing goes through the host until the metrics are read.

    python examples/pibt_rollout.py [--envs 1024] [--agents 32] [--size 32] [--density 0.3] [--steps 128]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402


def episode_isr(env, act, after_step, steps, seed):
    """Mean ISR over the envs after one episode of `steps` steps driven by `act()`."""
    env.reset(seed=seed)
    isr = torch.zeros(env.batch, dtype=torch.float32, device=env.device)
    seen = torch.zeros(env.batch, dtype=torch.bool, device=env.device)   # the metrics row counts where the episode ENDS
    for _ in range(steps):
        _, rewards, _, _, infos = env.step(act(), compute_obs=False)
        after_step(rewards, infos["episode_done"])
        done = infos["episode_done"].to(torch.bool) & ~seen
        isr = torch.where(done, infos["metrics"][:, 0], isr)
        seen |= done
    return float(isr.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=args.density, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps)
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    policy = PibtPolicy(env)
    planner = episode_isr(env, lambda: policy.act()[0], policy.update, args.steps, args.seed)
    expert = episode_isr(env, lambda: env.expert_actions()[0], lambda *_: None, args.steps, args.seed)
    print(f"{args.envs} envs, {args.agents} agents on {args.size}x{args.size}, density {args.density}, {args.steps} steps")
    print(f"ISR planner (PIBT) {planner:.4f}   ISR shortest-path expert {expert:.4f}   "
          f"distance fields built: {env.cost_to_go_builds}")
    env.close()


if __name__ == "__main__":
    main()
