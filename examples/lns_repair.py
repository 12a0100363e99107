#!/usr/bin/env python3
"""Plan, repair, execute: whca_plan() as the plan source, path_conflicts() and `failed` as the validator, repair_plan()
(docs/SPEC.md S29) as the repair step of an LNS-style loop, rollout() as the executor.

1. whca_plan(16) plans every agent.
2. While an env holds a failed agent (a few rounds at most, and only while their number falls): the failed agents and
   the agents within Chebyshev distance 2 of them are replanned in place, the failed ones first; everybody else keeps its
   path as a reservation.  An agent that is off its target and whose path goes nowhere -- it is boxed in, typically by
   a kept agent that waits on its own target -- is treated like a failed one.
3. path_conflicts() counts what is left, rollout() runs the first 8 steps, and the rest of the plan is shifted to the
   front and padded with its last cell.  repair_plan() goes on from there: an agent whose shifted path can still be
   walked from where the rollout left it, and ends on its target, is kept; the others -- stale (a reverted move, a new
   target), broken, or with nowhere left to go -- are served again around them.
4. Every call prints how many agents it replanned.

    python examples/lns_repair.py [--envs 1024] [--agents 32] [--size 32] [--density 0.3] [--steps 128] [--quiet]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402
from whca_rollout import FirstEpisode, whca_episode  # noqa: E402

ROUNDS = 3      # repairs of failed searches per window, at most
REACH = 2       # the neighbourhood of a failed agent, Chebyshev


def in_trouble(env, path, failed):
    """The agents whose search failed, and the active agents off their target whose path ends where it starts."""
    st = env.get_state()
    xy = st["agents_xy"]
    stuck = (path[-1] == xy).all(dim=-1) & (xy != st["targets_xy"]).any(dim=-1) & st["is_active"].bool()
    return failed.bool() | stuck


def neighbourhood(env, bad):
    """The agents of `bad` and the active agents within REACH of one, bool [batch, agents]."""
    st = env.get_state()
    xy = st["agents_xy"]
    near = (xy[:, :, None] - xy[:, None]).abs().amax(dim=-1) <= REACH              # [batch, agent, other]
    return (near & bad[:, None, :]).any(dim=-1) & st["is_active"].bool() | bad


def repair_episode(env, steps, horizon=16, execute=8, log=print):
    """One episode of `steps` steps from the env's current state.  Returns (FirstEpisode, agent searches made, the
    conflicts path_conflicts() counted in the windows that were run)."""
    B, A, dev = env.batch, env.num_agents, env.device
    prio = torch.zeros((B, A), dtype=torch.int32, device=dev)
    outs = (torch.empty((horizon, B, A), dtype=torch.int64, device=dev), torch.empty((horizon, B, A, 2), dtype=torch.int32, device=dev),
            *(torch.empty((B, A), dtype=torch.int32, device=dev) for _ in range(3)))
    actions, path, arrival, failed, replanned = outs
    first = FirstEpisode(env)
    env.whca_plan(horizon, priority=prio, out=outs[:4])
    searches = int(env.get_state()["is_active"].sum())
    log(f"step 0: whca_plan({horizon}) served {searches} agents, {int(failed.sum())} searches failed")
    conflicts = 0
    for t0 in range(0, steps, execute):
        fewer = None
        for k in range(ROUNDS):
            bad = in_trouble(env, path, failed) & ~first.seen.view(-1, 1)
            if not bool(bad.any()) or (fewer is not None and int(bad.sum()) >= fewer):
                break
            fewer = int(bad.sum())
            # the failed agents outrank everybody, in their old order
            top = torch.where(bad, prio.max() + 1 + (prio - prio.min()), prio)
            env.repair_plan(path, replan=neighbourhood(env, bad), priority=top, out=outs)      # in place
            searches += int(replanned.sum())
            log(f"step {t0}: {fewer} agents failed or boxed in, repair {k + 1} replanned {int(replanned.sum())} agents, "
                f"{int(failed.sum())} searches failed")
        count = env.path_conflicts(path, kinds=("vertex", "edge"))[3]
        conflicts += int((count.sum(dim=1) * ~first.seen).sum())
        n = min(execute, steps - t0)
        out = env.rollout(actions[:n], obs_slots=0)
        first.add(out)
        if t0 + n >= steps:
            break
        st = env.get_state()
        on_target = (st["agents_xy"] == st["targets_xy"]).all(dim=-1)
        zero = on_target | ~st["is_active"].bool() | out["episode_done"].any(dim=0).view(-1, 1)
        prio = torch.where(zero, torch.zeros_like(prio), prio + n)
        path.copy_(torch.cat([path[n:], path[-1:].expand(n, -1, -1, -1)]))       # what is left of the plan, padded
        nowhere_to_go = (path[-1] != st["targets_xy"]).any(dim=-1)
        env.repair_plan(path, replan=nowhere_to_go, priority=prio, out=outs)
        searches += int(replanned.sum())
        stale = int((replanned.bool() & ~nowhere_to_go).sum())
        log(f"step {t0 + n}: repair replanned {int(replanned.sum())} of {int(st['is_active'].sum())} agents "
            f"({stale} of them because their path could not be walked any more)")
    return first, searches, conflicts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args()
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=args.density, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps)
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    env.reset(seed=args.seed)
    first, searches, conflicts = repair_episode(env, args.steps, log=(lambda *a: None) if args.quiet else print)
    env.reset(seed=args.seed)
    whca, failed, plans = whca_episode(env, args.steps, 16, 8)
    print(f"{args.envs} envs, {args.agents} agents on {args.size}x{args.size}, density {args.density}, {args.steps} steps")
    print(f"whca_plan(16) + repair_plan + rollout(8): solved {int(first.csr.sum())} of {args.envs} envs, "
          f"ISR {float(first.isr.mean()):.4f}, {searches} agent searches, {conflicts} conflicts left in the windows run")
    print(f"whca_plan(16) + rollout(8), all replanned: solved {int(whca.csr.sum())} of {args.envs} envs, "
          f"ISR {float(whca.isr.mean()):.4f}, {failed} failed searches in {plans} plans")
    env.close()


if __name__ == "__main__":
    main()
