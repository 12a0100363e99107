#!/usr/bin/env python3
"""The input of a centralised critic, written by one launch of global_state() per step: the whole map of every env --
obstacles, agents, targets, and who stands where -- while the cooperative planner (PibtPolicy) drives the agents and
finished envs draw a fresh map from a pool inside step() (auto_reset="regenerate").  A small critic reads
the tensor as it is; nothing is assembled in torch and nothing goes through the host.  Each step checks the obstacle
plane against map_pool[map_index]: it follows the env's map through every regeneration.

    python examples/central_critic.py [--envs 256] [--agents 16] [--size 24] [--maps 8] [--steps 48] [--dtype float32]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, PibtPolicy, VecPogema  # noqa: E402

CHANNELS = ("obstacles", "agents", "targets", "agent_ids")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=16)
    ap.add_argument("--size", type=int, default=24)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--dtype", default="float32", choices=("float32", "float16", "bfloat16"))
    args = ap.parse_args()

    dtype = getattr(torch, args.dtype)
    gen = torch.Generator().manual_seed(0)
    pool = (torch.rand((args.maps, args.size, args.size), generator=gen) < 0.2).to(torch.uint8)
    gc = GridConfig(num_agents=args.agents, obs_radius=4, seed=0, collision_system="soft", on_target="finish",
                    max_episode_steps=16)
    env = VecPogema(gc, batch=args.envs, auto_reset="regenerate", map_pool=pool)
    env.reset(seed=0)
    policy = PibtPolicy(env)
    critic = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(len(CHANNELS) * args.size * args.size, 64),
                                 torch.nn.ReLU(), torch.nn.Linear(64, 1))
    critic = critic.to(device=env.device, dtype=dtype)
    state = torch.empty((args.envs, len(CHANNELS), args.size, args.size), dtype=dtype, device=env.device)
    first = env.map_index.clone()
    redrawn = torch.zeros(args.envs, dtype=torch.bool, device=env.device)
    value = None
    for t in range(args.steps):
        env.global_state(channels=CHANNELS, dtype=dtype, out=state)
        with torch.no_grad():
            value = critic(state)                    # [envs, 1]: the critic's training step goes here
        index = env.map_index.long()
        if not torch.equal(state[:, 0], env.map_pool[index].to(dtype)):
            raise SystemExit(f"step {t}: the obstacle plane is not the map the env runs")
        redrawn |= index != first.long()
        actions, _ = policy.act()
        _, rewards, _, _, infos = env.step(actions, compute_obs=False)
        policy.update(rewards, infos["episode_done"])
    print("critic input", tuple(state.shape), state.dtype, "on", state.device, "-> values", tuple(value.shape))
    print(f"{int(redrawn.sum())} of {args.envs} envs ran another map than their first within {args.steps} steps; "
          f"the obstacle plane followed every one")
    env.close()


if __name__ == "__main__":
    main()
