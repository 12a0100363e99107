#!/usr/bin/env python3
"""Receding-horizon episodes with windowed cooperative A* (whca_plan(), docs/SPEC.md S28): plan K = 16 steps against the
reservation table, run the first 8 of them in one rollout() launch, grow the priorities by PibtPolicy's rule -- 0 for an
agent on its target or out of the game, else one more per step run -- and plan again from where the rollout ended, until
the episode is over.  An agent the planner could not serve (`failed`) stays put for that window and outranks its
neighbours in a later one.  Prints the solved envs, the individual success rate and the number of failed searches next to
the rates of examples/planned_rollout.py's plan (PibtPolicy.plan(16) + rollout()) on the same seeded instances.

    python examples/whca_rollout.py [--envs 1024] [--agents 32] [--size 32] [--density 0.3] [--steps 128]
                                    [--horizon 16] [--execute 8]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402


class FirstEpisode:
    """The metrics row of each env's first finished episode, collected from rollout() outputs."""

    def __init__(self, env):
        self.isr = torch.zeros(env.batch, dtype=torch.float32, device=env.device)
        self.csr = torch.zeros(env.batch, dtype=torch.float32, device=env.device)
        self.seen = torch.zeros(env.batch, dtype=torch.bool, device=env.device)

    def add(self, out):
        for done, metrics in zip(out["episode_done"], out["metrics"]):
            first = done & ~self.seen
            self.isr = torch.where(first, metrics[:, 0], self.isr)
            self.csr = torch.where(first, metrics[:, 1], self.csr)
            self.seen |= first


def whca_episode(env, steps, horizon=16, execute=8):
    """One episode of `steps` steps from the env's current state: whca_plan(horizon), rollout of the first `execute`
    steps, new priorities, again.  Returns (FirstEpisode, failed searches, plans made)."""
    prio = torch.zeros((env.batch, env.num_agents), dtype=torch.int32, device=env.device)
    first = FirstEpisode(env)
    failed_total = torch.zeros((), dtype=torch.int64, device=env.device)
    plans = 0
    for t0 in range(0, steps, execute):
        actions, _, _, failed = env.whca_plan(horizon, priority=prio)
        n = min(execute, horizon, steps - t0)
        out = env.rollout(actions[:n], obs_slots=0)
        first.add(out)
        failed_total += (failed.sum(dim=1) * ~first.seen).sum()      # (envs whose episode is over are not counted)
        plans += 1
        st = env.get_state()
        zero = (st["agents_xy"] == st["targets_xy"]).all(dim=-1) | ~st["is_active"] | out["episode_done"].any(dim=0).view(-1, 1)
        prio = torch.where(zero, torch.zeros_like(prio), prio + n)
    return first, int(failed_total), plans


def pibt_episode(env, steps, horizon=16):
    """The same episode under examples/planned_rollout.py's plan: PibtPolicy.plan(horizon) + rollout()."""
    policy = PibtPolicy(env)
    first = FirstEpisode(env)
    for t0 in range(0, steps, horizon):
        actions, _, _ = policy.plan(min(horizon, steps - t0))
        out = env.rollout(actions, obs_slots=0)
        first.add(out)
        policy.priority[out["episode_done"].any(dim=0)] = 0
    return first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--execute", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=args.density, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps)
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    env.reset(seed=args.seed)
    whca, failed, plans = whca_episode(env, args.steps, args.horizon, args.execute)
    env.reset(seed=args.seed)
    pibt = pibt_episode(env, args.steps, args.horizon)
    print(f"{args.envs} envs, {args.agents} agents on {args.size}x{args.size}, density {args.density}, {args.steps} steps")
    print(f"whca_plan({args.horizon}) + rollout({args.execute}): solved {int(whca.csr.sum())} of {args.envs} envs, "
          f"ISR {float(whca.isr.mean()):.4f}, {failed} failed searches in {plans} plans")
    print(f"pibt_plan({args.horizon}) + rollout({args.horizon}): solved {int(pibt.csr.sum())} of {args.envs} envs, "
          f"ISR {float(pibt.isr.mean()):.4f}")
    env.close()


if __name__ == "__main__":
    main()
