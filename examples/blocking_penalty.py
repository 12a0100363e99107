#!/usr/bin/env python3
"""PRIMAL's reward per step, all of it from the device: the collision penalty from move_outcomes() before the step and
the blocking penalty from blocking() after it -- an agent is charged for every agent it sees whose way to its goal gets
`--inflation` steps longer, or is cut off, because of where the agent stands -- during one episode driven by PibtPolicy
under on_target="nothing".  At one step the blocking counts of the first envs are recomputed on the host with two plain
searches per pair, the way upstream implementations pay for the penalty at every step.

    python examples/blocking_penalty.py [--envs 256] [--agents 16] [--size 16] [--steps 64] [--inflation 10]
"""
import argparse
import os
import sys
from collections import deque

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import OUTCOMES, GridConfig, PibtPolicy, VecPogema  # noqa: E402

OBSTACLE = OUTCOMES.index("OBSTACLE")


def path_length(blocked, s, t):
    """Steps of a shortest path from s to t over the cells that are not blocked, -1 without one."""
    H, W = len(blocked), len(blocked[0])
    if blocked[t[0]][t[1]]:
        return -1
    dist = {s: 0}
    q = deque([s])
    while q:
        c = q.popleft()
        if c == t:
            return dist[c]
        for n in ((c[0] - 1, c[1]), (c[0] + 1, c[1]), (c[0], c[1] - 1), (c[0], c[1] + 1)):
            if 0 <= n[0] < H and 0 <= n[1] < W and not blocked[n[0]][n[1]] and n not in dist:
                dist[n] = dist[c] + 1
                q.append(n)
    return -1


def host_count(grid, xy, targets, active, r, inflation, on_target):
    """count[i] of one env (docs/SPEC.md S25), two searches per pair."""
    A = len(xy)
    count = [0] * A
    for i in range(A):
        if not active[i] or (on_target and xy[i] != targets[i]):
            continue
        for j in range(A):
            if j == i or not active[j] or max(abs(xy[j][0] - xy[i][0]), abs(xy[j][1] - xy[i][1])) > r or xy[j] == xy[i]:
                continue
            d0 = path_length(grid, xy[j], targets[j])
            if d0 < 0:
                continue
            without = [row[:] for row in grid]
            without[xy[i][0]][xy[i][1]] = 1
            d1 = path_length(without, xy[j], targets[j])
            count[i] += d1 < 0 or d1 > d0 + inflation - 1
    return count


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=16)
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--inflation", type=int, default=10)
    ap.add_argument("--blockers", default="on_target", choices=("all", "on_target"))
    ap.add_argument("--collision-penalty", type=float, default=2.0)
    ap.add_argument("--blocking-penalty", type=float, default=1.0)
    ap.add_argument("--check-envs", type=int, default=4)
    args = ap.parse_args()
    r = 5
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=r, density=args.density, seed=3,
                    collision_system="soft", on_target="nothing", max_episode_steps=args.steps)
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    env.reset(seed=3)
    policy = PibtPolicy(env)
    shaped = torch.zeros((), device=env.device)
    collided = torch.zeros((), dtype=torch.int64, device=env.device)
    blocked = torch.zeros((), dtype=torch.int64, device=env.device)
    checked = 0
    for t in range(args.steps):
        actions = policy.act()[0]
        _, outcome, _, _ = env.move_outcomes(actions)            # before the step: what these actions will do
        _, rewards, _, _, infos = env.step(actions, compute_obs=False)
        policy.update(rewards, infos["episode_done"])
        count, _ = env.blocking(inflation=args.inflation, blockers=args.blockers)   # after it: who stands in whose way
        hit = outcome >= OBSTACLE
        shaped += (rewards - args.collision_penalty * hit - args.blocking_penalty * count).mean()
        collided += hit.sum()
        blocked += count.sum()
        if t == args.steps // 2:                                 # the host's way, on the first envs
            st = env.get_state()
            n = min(args.check_envs, env.batch)
            xy, tg, act = (st[k][:n].cpu().tolist() for k in ("agents_xy", "targets_xy", "is_active"))
            maps = env.global_state(channels=("obstacles",), dtype=torch.uint8)[:n, 0].cpu().tolist()
            for mode in ("all", "on_target"):                    # the reward's mode and the other one
                got = count if mode == args.blockers else env.blocking(inflation=args.inflation, blockers=mode)[0]
                for b in range(n):
                    want = host_count(maps[b], [tuple(c) for c in xy[b]], [tuple(c) for c in tg[b]], act[b], r,
                                      args.inflation, mode == "on_target")
                    assert got[b].cpu().tolist() == want, f"step {t}, env {b}, {mode}: {got[b].cpu().tolist()} vs the host's {want}"
                    checked += sum(want)
    steps = args.steps * env.batch * env.num_agents
    print(f"{env.batch} envs, {env.num_agents} agents on {args.size}x{args.size}, {args.steps} steps of PIBT, inflation "
          f"{args.inflation}, blockers {args.blockers!r}")
    print(f"mean shaped reward per step {float(shaped) / args.steps:.4f}   collisions per agent-step {int(collided) / steps:.4f}   "
          f"blocked agents per agent-step {int(blocked) / steps:.4f}")
    print(f"host check at step {args.steps // 2}: the counts of {min(args.check_envs, env.batch)} envs agree under both "
          f"`blockers` modes ({checked} blocked pairs)")
    env.close()


if __name__ == "__main__":
    main()
