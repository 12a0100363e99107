#!/usr/bin/env python3
"""Build the input and the shaped reward of a planning-plus-learning policy ("Learn to Follow" style) every step of an
episode.  The input is two planes per agent: the obstacle plane of the observation with the planned path to the goal
written into it (obstacles 1, path cells -1, everything else 0), next to the agents plane.  The reward is intrinsic:
every K steps each agent is issued the sub-goal K cells down its path, and K steps later it earns 1 if it stands on it.
Both come from one goal_paths() launch per step.  The on-device planner (PibtPolicy) stands in for the network and
drives the episode, so most sub-goals are reached and the rest were lost to giving way.

    python examples/follow_path.py [--envs 256] [--agents 32] [--size 32] [--density 0.3] [--steps 64] [--every 4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--every", type=int, default=4, help="K: steps between sub-goals = cells a sub-goal lies ahead")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    K = args.every
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=args.density, seed=args.seed,
                    collision_system="soft", on_target="nothing", max_episode_steps=args.steps)
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    policy = PibtPolicy(env)
    B, A, W = env.batch, env.num_agents, env.window
    path = torch.empty((B, A, W, W), dtype=torch.float32, device=env.device)
    subgoal = torch.empty((B, A, 2), dtype=torch.int8, device=env.device)
    length = torch.empty((B, A), dtype=torch.int32, device=env.device)
    obs, _ = env.reset(seed=args.seed)
    issued_xy = issued = None
    earned = asked = 0
    for t in range(args.steps):
        env.goal_paths(out=(path, subgoal, length))                     # the whole visible path, for the input
        x = torch.stack((obs[:, :, 0].float() - path, obs[:, :, 1].float()), 2)   # what the network would read
        assert tuple(x.shape) == (B, A, 2, W, W) and float(x.min()) >= -1.0
        xy = env.get_state()["agents_xy"]
        if t % K == 0:
            if issued is not None:                                      # the reward for the sub-goals of K steps ago
                reached = (xy == issued_xy).all(-1) & issued
                earned += int(reached.sum())
                asked += int(issued.sum())
            _, ahead, n = env.goal_paths(steps=K, planes=False)         # the next sub-goals: K cells down the path
            issued_xy, issued = xy + ahead.to(xy.dtype), n > 0
        actions, _ = policy.act()
        obs, rewards, _, _, infos = env.step(actions)
        policy.update(rewards, infos["episode_done"])
    print(f"{args.envs} envs, {args.agents} agents on {args.size}x{args.size}, density {args.density}, {args.steps} steps: "
          f"{x.numel() * 4} bytes of input per step, sub-goals {K} cells ahead every {K} steps: {earned} of {asked} reached "
          f"({100.0 * earned / max(asked, 1):.1f} %)")
    env.close()


if __name__ == "__main__":
    main()
