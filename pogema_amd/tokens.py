"""What goes with VecPogema.agent_tokens() (docs/SPEC.md S21) and needs no engine: the row length of a shape, and the
action history the caller keeps and passes in."""
from __future__ import annotations

from . import _lib

TOKENS = _lib.TOKENS


def _int_in(name, value, lo, hi):
    """`value` as an int when it is an integer (not a bool) in lo..hi, else a ValueError naming `name` and the range."""
    import numpy as np
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {value!r}")
    return int(value)


def token_length(obs_radius, slots) -> int:
    """L0 = (2 * obs_radius + 1) ** 2 + 10 * slots: the entries of an agent_tokens() row before its padding
    (pgx_agent_tokens_length).  obs_radius 1..15, slots 1..32; anything else is a ValueError naming the range."""
    r = _int_in("obs_radius", obs_radius, 1, _lib.MAX_OBS_RADIUS)
    s = _int_in("slots", slots, 1, _lib.MAX_TOKEN_SLOTS)
    return (2 * r + 1) ** 2 + _lib.TOKEN_SLOT_LEN * s


class TokenHistory:
    """The last five actions of every agent, as agent_tokens(history=...) reads them: an int8 tensor [batch, agents, 5],
    most recent action first, -1 where nothing is recorded.  Pure torch on the env's device; it never touches the engine.

        hist = TokenHistory(env)
        obs = env.reset()
        while ...:
            tokens = env.agent_tokens(history=hist.tensor)
            actions = policy(tokens)
            *_, infos = env.step(actions)
            hist.push(actions, infos["episode_done"])

    `env`: anything with `batch`, `num_agents` and `device` (a VecPogema)."""

    def __init__(self, env):
        import torch
        self.batch, self.num_agents, self.device = int(env.batch), int(env.num_agents), torch.device(env.device)
        self.tensor = torch.full((self.batch, self.num_agents, _lib.TOKEN_HISTORY), -1, dtype=torch.int8, device=self.device)

    def reset(self) -> None:
        """Nothing is recorded anywhere."""
        self.tensor.fill_(-1)

    def push(self, actions, episode_done=None) -> None:
        """Records `actions` (an integer tensor [batch, agents]) as the most recent ones; the oldest are dropped.  Envs
        flagged in `episode_done` (a bool / uint8 tensor [batch], what step()'s infos carry) start over: their history
        is cleared, the actions that ended the episode included."""
        import torch
        if not isinstance(actions, torch.Tensor) or actions.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
            raise TypeError("actions must be an integer torch.Tensor")
        if tuple(actions.shape) != (self.batch, self.num_agents):
            raise ValueError(f"actions must have shape {(self.batch, self.num_agents)}, got {tuple(actions.shape)}")
        # values outside int8 are no actions: -1 reads as "nothing recorded" (agent_tokens() treats every value but 0..4 so)
        a = torch.where((actions >= 0) & (actions <= 4), actions, torch.full_like(actions, -1)).to(self.device, torch.int8)
        # in place: `tensor` stays the same storage, so a captured agent_tokens(history=hist.tensor) keeps reading it
        self.tensor.copy_(torch.cat((a.unsqueeze(-1), self.tensor[:, :, :-1]), dim=-1))
        if episode_done is not None:
            done = torch.as_tensor(episode_done, device=self.device).to(torch.bool)
            if tuple(done.shape) != (self.batch,):
                raise ValueError(f"episode_done must have shape {(self.batch,)}, got {tuple(done.shape)}")
            self.tensor.masked_fill_(done.view(-1, 1, 1), -1)
