"""PibtPolicy: the cooperative planner (VecPogema.pibt_actions, docs/SPEC.md S13) with the textbook dynamic priorities --
an agent's priority grows by one every step it has not reached its target and drops to zero when it has, so that an
agent that keeps being pushed aside eventually outranks its neighbours."""
from __future__ import annotations

import torch


class PibtPolicy:
    """`act()` -> (actions, next_xy) for `env.step`; `update(rewards, episode_done)` after the step.  The int32 priority
    tensor [batch, agents] lives on the env's device; nothing here synchronises with the host.
    `act(scores=...)` shields a learnt policy's action scores under the same priorities (VecPogema.shield_actions,
    docs/SPEC.md S15) and returns (actions, next_xy, overridden).
    `plan(horizon)` -> (actions, path_xy, arrival) for `env.rollout`: the same priorities grown inside the lookahead
    (VecPogema.pibt_plan, docs/SPEC.md S16); no `update()` is needed between a plan and the next.
    `PibtPolicy(env, swap=True)`: act() plans with the swap operation (VecPogema.pibt_actions(swap=True), docs/SPEC.md
    S23), which clears the dead ends and corridors the plain rule livelocks in; act(scores=...) is unchanged.
    `plan(horizon, swap=True)` plans with the swap operation at every step (VecPogema.pibt_plan(swap=True), S27) and
    `plan(horizon, swap=False)` without, whatever the policy was built with.  Without the keyword a policy built
    without swap plans without it, and one built with swap=True raises: the choice has to be made in the call."""

    def __init__(self, env, swap=False):
        if not isinstance(swap, bool):
            raise TypeError(f"swap must be a bool, got {type(swap).__name__}")
        self.env = env
        self.swap = swap
        self.priority = torch.zeros((env.batch, env.num_agents), dtype=torch.int32, device=env.device)

    def reset(self) -> None:
        self.priority.zero_()

    def act(self, dtype=torch.int64, out=None, *, scores=None, tie_break=None):
        if scores is None:
            if tie_break is not None:
                raise ValueError("tie_break belongs to act(scores=...)")
            return self.env.pibt_actions(priority=self.priority, dtype=dtype, out=out, swap=self.swap)
        return self.env.shield_actions(scores, priority=self.priority, tie_break=tie_break, dtype=dtype, out=out)

    def plan(self, horizon, dtype=torch.int64, out=None, *, swap=None):
        """`horizon` steps planned ahead from the current state under `self.priority`; the priorities the lookahead
        ends with replace it, so that the next plan() or act() after `env.rollout(actions)` continues where this one
        stopped.  The plan does not know when an episode ends: where the rollout reports `episode_done` for an env (its
        time limit, or every agent finished), zero that env's row of `self.priority` before planning again, as
        `update(rewards, episode_done)` does.  `out=(actions, path_xy, arrival, priority)` as VecPogema.pibt_plan takes
        it.  `swap`: True plans with the swap operation (docs/SPEC.md S27), False without; None leaves it to the
        policy -- without swap for one built without it, an error for one built with swap=True."""
        if swap is not None and not isinstance(swap, bool):
            raise TypeError(f"swap must be a bool or None, got {type(swap).__name__}")
        if swap is None:
            if self.swap:
                raise ValueError("plan() on a PibtPolicy(env, swap=True): the multi-step planner (pibt_plan) applies "
                                 "no swap rule unless asked: call plan(horizon, swap=True), or plan(horizon, "
                                 "swap=False) for the plain lookahead")
            keyword = {}                      # an env whose pibt_plan has no such keyword plans as before
        else:
            keyword = {"swap": swap}
        actions, path_xy, arrival, self.priority = self.env.pibt_plan(horizon, priority=self.priority, dtype=dtype,
                                                                     out=out, **keyword)
        return actions, path_xy, arrival

    def copy_envs(self, src, dst, *, cache: bool = True, validate: bool = True) -> None:
        """`env.copy_envs(src, dst)` (docs/SPEC.md S19) with the policy's priorities: row dst[k] of `self.priority`
        becomes row src[k], so that act() on a copy equals act() on its source.  A pair the engine skips (an index
        outside 0..batch-1 under `validate=False`) is skipped here too."""
        from .vec_env import copy_pairs
        B = self.env.batch
        s, d = copy_pairs(src, dst, B, validate)
        s, d = s.to(self.priority.device).long(), d.to(self.priority.device).long()
        ok = (s >= 0) & (s < B) & (d >= 0) & (d < B)
        spare = torch.full_like(d, B)  # a skipped pair moves the spare row B onto itself: no host sync, no clash
        rows = torch.cat([self.priority, self.priority.new_zeros((1, self.priority.shape[1]))])
        rows.index_copy_(0, torch.where(ok, d, spare), rows.index_select(0, torch.where(ok, s, spare)))
        self.priority = rows[:B]
        self.env.copy_envs(src, dst, cache=cache, validate=False)

    def update(self, rewards, episode_done=None) -> None:
        """Priority becomes 0 where the agent got a positive reward in this step, stands on its target, is inactive, or
        its env's episode finished (`episode_done`: bool / uint8 [batch], e.g. step()'s infos["episode_done"]);
        everywhere else it goes up by 1."""
        st = self.env.get_state()
        zero = (rewards > 0) | (st["agents_xy"] == st["targets_xy"]).all(dim=-1) | ~st["is_active"]
        if episode_done is not None:
            zero = zero | episode_done.to(torch.bool).view(-1, 1)
        self.priority = torch.where(zero, torch.zeros_like(self.priority), self.priority + 1)
