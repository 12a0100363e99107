#!/usr/bin/env python3
"""Build the 256-token context of a MAPF-GPT-style policy every step of an episode: agent_tokens() with obs_radius=5,
slots=13, length=256 is the 121 + 130 + 5 layout -- the cost-to-go window relative to the agent's own cost, ten entries
for the agent and each of its twelve nearest neighbours, padding.  The on-device planner (PibtPolicy) stands in for the
network and drives the episode; TokenHistory keeps the last five actions of every agent on the device and is all the
caller has to feed.  The first step's context is checked against the torch composition of the four queries it replaces
(cost_to_go(), visible_agents(), goal_directions("bits"), get_state()).

    python examples/mapf_gpt_tokens.py [--envs 256] [--agents 32] [--size 32] [--density 0.3] [--steps 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pogema_amd import TOKENS, GridConfig, PibtPolicy, TokenHistory, VecPogema, token_length  # noqa: E402

SLOTS, LENGTH = 13, 256


def composed(env, history):
    """The same rows from the separate queries: three engine launches, their outputs written and read back, and a dozen
    torch kernels."""
    B, A, W, r = env.batch, env.num_agents, env.window, env.obs_radius
    dev = env.device
    ctg = env.cost_to_go().long()
    own = ctg[:, :, r, r]
    st = env.get_state()
    xy, tg = st["agents_xy"].long(), st["targets_xy"].long()
    mask = env.goal_directions("bits")[:, :, r, r].long()
    index, offset, _ = env.visible_agents(k=SLOTS - 1)
    win = ctg.view(B, A, W * W)
    window = torch.where((win == -1) | (own == -1).unsqueeze(-1), TOKENS["BLOCKED"],
                         (win - own.unsqueeze(-1)).clamp(-TOKENS["CLIP"], TOKENS["CLIP"]) + TOKENS["CLIP"])
    j = torch.cat((torch.arange(A, device=dev).view(1, A, 1).expand(B, A, 1), index.long()), 2)
    off = torch.cat((torch.zeros((B, A, 1, 2), dtype=torch.long, device=dev), offset.long()), 2)
    jj = j.clamp(min=0)
    b = torch.arange(B, device=dev).view(B, 1, 1)
    goal = (tg[b, jj] - xy.unsqueeze(2)).clamp(-TOKENS["CLIP"], TOKENS["CLIP"]) + TOKENS["CLIP"]
    h = history.long()
    actions = torch.where((h >= 0) & (h <= 4), TOKENS["ACTION0"] + h, TOKENS["ACTION_NONE"])
    slots = torch.cat((off + TOKENS["CLIP"], goal, actions[b, jj], (TOKENS["GREEDY0"] + mask[b, jj]).unsqueeze(-1)), -1)
    slots = torch.where((j >= 0).unsqueeze(-1), slots, TOKENS["PAD"])
    pad = torch.full((B, A, LENGTH - token_length(r, SLOTS)), TOKENS["PAD"], dtype=torch.long, device=dev)
    rows = torch.cat((window, slots.view(B, A, -1), pad), 2)
    return torch.where(st["is_active"].bool().unsqueeze(-1), rows, TOKENS["PAD"]).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    gc = GridConfig(size=args.size, num_agents=args.agents, obs_radius=5, density=args.density, seed=args.seed,
                    collision_system="soft", on_target="finish", max_episode_steps=args.steps)
    env = VecPogema(gc, batch=args.envs, auto_reset=False)
    assert token_length(gc.obs_radius, SLOTS) == 251
    policy = PibtPolicy(env)
    history = TokenHistory(env)
    context = torch.empty((env.batch, env.num_agents, LENGTH), dtype=torch.uint8, device=env.device)
    env.reset(seed=args.seed)
    used = torch.zeros(TOKENS["NUM_TOKENS"], dtype=torch.bool, device=env.device)
    for t in range(args.steps):
        env.agent_tokens(slots=SLOTS, history=history.tensor, length=LENGTH, out=context)   # what the network would read
        if t == 1:                                # after one step: a history to compare, too
            assert torch.equal(context, composed(env, history.tensor)), "agent_tokens() differs from the composition"
        used[context.long().unique()] = True
        actions, _ = policy.act()
        _, rewards, _, _, infos = env.step(actions, compute_obs=False)
        policy.update(rewards, infos["episode_done"])
        history.push(actions, infos["episode_done"])
    finished = 1.0 - float(env.get_state()["is_active"].float().mean())
    print(f"{args.envs} envs, {args.agents} agents on {args.size}x{args.size}, density {args.density}, {args.steps} steps: "
          f"{context.numel()} bytes of context per step, {int(used.sum())} of {TOKENS['NUM_TOKENS']} token ids seen, "
          f"{100 * finished:.1f} % of the agents finished")
    env.close()


if __name__ == "__main__":
    main()
