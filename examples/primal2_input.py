#!/usr/bin/env python3
"""Build the input of a PRIMAL2-style decentralised policy every step of an episode: the obstacle, agents and own-target
planes and the goals of the visible agents (policy_input()), and behind them K planes that say where those agents are
going to be after 1 .. K steps if each follows its own shortest path (agent_forecasts()) -- the planes that let a policy
give way before a conflict instead of after it.  Two launches and a torch.cat per step.  Every step it also checks that
an agent's first forecast cell is the cell expert_actions() moves it to.  The on-device planner (PibtPolicy) stands in
for the network and drives the episode.

    python examples/primal2_input.py [--envs 256] [--agents 32] [--size 32] [--density 0.3] [--steps 64] [--ahead 3]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402

CHANNELS = ("obstacles", "agents", "target", "other_goals")
MOVES = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))      # noop, up, down, left, right as (row, column)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--ahead", type=int, default=3, help="K: forecast planes per agent")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    K = args.ahead
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=args.density, seed=args.seed,
                    collision_system="soft", on_target="nothing", max_episode_steps=args.steps)
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    policy = PibtPolicy(env)
    B, A, W = env.batch, env.num_agents, env.window
    base = torch.empty((B, A, len(CHANNELS), W, W), dtype=torch.uint8, device=env.device)
    ahead = torch.empty((B, A, K, W, W), dtype=torch.uint8, device=env.device)
    cells = torch.empty((B, A, K, 2), dtype=torch.int16, device=env.device)
    moves = torch.tensor(MOVES, device=env.device)
    env.reset(seed=args.seed)
    marked = 0
    for t in range(args.steps):
        env.policy_input(CHANNELS, dtype=torch.uint8, out=base)
        env.agent_forecasts(K, "uint8", out=(ahead, cells))
        x = torch.cat((base, ahead), 2)                                 # what the network would read
        assert tuple(x.shape) == (B, A, len(CHANNELS) + K, W, W)
        marked += int(ahead.sum())
        # the first forecast cell is where the shortest-path expert goes
        expert, _ = env.expert_actions()
        assert torch.equal(cells[:, :, 0].long(), env.get_state()["agents_xy"].long() + moves[expert])
        actions, _ = policy.act()
        _, rewards, _, _, infos = env.step(actions)
        policy.update(rewards, infos["episode_done"])
    print(f"{args.envs} envs, {args.agents} agents on {args.size}x{args.size}, density {args.density}, {args.steps} steps: "
          f"{x.numel()} bytes of input per step ({len(CHANNELS)} + {K} uint8 planes per agent), "
          f"{marked / (args.steps * B * A):.2f} forecast cells drawn per agent and step")
    env.close()


if __name__ == "__main__":
    main()
