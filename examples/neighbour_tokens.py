#!/usr/bin/env python3
"""Per-neighbour input features of a token / attention MAPF policy, assembled on the device: for every agent its
cost-to-go window (cost_to_go()) and, for each of its up-to-K nearest visible agents (visible_agents()), the relative
position, the relative target clamped to the window and the neighbour's greedy action (expert_actions()).  The
neighbour's own quantities are fetched with torch.gather on the index tensor; nothing goes through the host.

    python examples/neighbour_tokens.py [--envs 1024] [--agents 32] [--size 32] [--k 13] [--steps 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import GridConfig, VecPogema  # noqa: E402


def neighbour_features(env, k):
    """(window int32 [B, A, W, W], tokens int32 [B, A, k, 5], mask bool [B, A, k]); a token is (dx, dy, target dx, target dy,
    greedy action) of one visible agent, zeros where `mask` is False."""
    r = env.obs_radius
    index, offset, _ = env.visible_agents(k=k)            # [B, A, k], [B, A, k, 2]
    mask = index >= 0
    j = index.clamp(min=0).long()                          # a valid row to gather from; masked out below
    st = env.get_state()
    actions, _ = env.expert_actions(dtype=torch.int32)     # [B, A]
    B, A = actions.shape
    # what agent j carries, gathered per (agent, slot): flatten the slot axis into the gather index
    flat = j.view(B, A * k)
    their_action = torch.gather(actions, 1, flat).view(B, A, k)
    their_target = torch.gather(st["targets_xy"], 1, flat[..., None].expand(B, A * k, 2)).view(B, A, k, 2)
    # the neighbour's target relative to the observing agent, clamped to its window
    rel_target = (their_target - st["agents_xy"][:, :, None, :]).clamp(-r, r)
    tokens = torch.cat((offset.to(torch.int32), rel_target, their_action[..., None]), dim=-1)
    tokens = torch.where(mask[..., None], tokens, torch.zeros_like(tokens))
    return env.cost_to_go(), tokens, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--k", type=int, default=13)
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()

    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=0.3, seed=0, collision_system="soft",
                    on_target="restart", max_episode_steps=256)
    env = VecPogema(gc, batch=args.envs, auto_reset=True)
    env.reset(seed=0)
    seen = torch.zeros((), dtype=torch.int64, device=env.device)
    for _ in range(args.steps):
        window, tokens, mask = neighbour_features(env, args.k)      # your policy(window, tokens, mask) goes here
        seen += mask.sum()
        actions, _ = env.expert_actions(agents_as_obstacles=True)
        env.step(actions)
    print("cost-to-go window", tuple(window.shape), "neighbour tokens", tuple(tokens.shape), tokens.dtype, "on", tokens.device)
    print(f"{int(seen) / (args.steps * args.envs * args.agents):.2f} visible agents per agent and step on average "
          f"(at most {args.k} kept)")
    env.close()


if __name__ == "__main__":
    main()
