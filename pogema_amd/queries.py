"""VecPogema's read-only queries on the engine state: expert actions, cost-to-go windows, neighbour lists, the
cooperative planner and its multi-step lookahead, windowed cooperative A*, plan repair, collision shielding, direction-to-goal planes, path-to-goal planes,
agent forecasts, blocking counts, path conflicts, move outcomes, the policy input, the global state and the agent tokens.  Each is one C-ABI
call into caller-owned or fresh output tensors; query_output() is the one place an `out` tensor is checked or allocated.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def query_output(name, out, dtypes, shape, device, align=None):
    """The tensor a query writes its result `name` into: `out` itself when the caller gave one, else a fresh tensor of
    dtypes[0].  `out` must be a contiguous tensor of one of `dtypes` (a dtype or a sequence of them) and of `shape` on
    `device`, at an address that is a multiple of `align` bytes (default: its element size): anything else is a
    ValueError that names `name` and what is expected.  Needs no engine and no GPU."""
    dtypes = (dtypes,) if isinstance(dtypes, torch.dtype) else tuple(dtypes)
    shape, device = tuple(shape), torch.device(device)
    if out is None:
        return torch.empty(shape, dtype=dtypes[0], device=device)
    if not (isinstance(out, torch.Tensor) and out.dtype in dtypes and tuple(out.shape) == shape and out.is_contiguous()
            and out.device == device and out.data_ptr() % (align or out.element_size()) == 0):
        names = " / ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{name} must be a contiguous {names} tensor of shape {shape} on {device}, aligned to "
                         f"{f'{align} bytes' if align else 'its element size'}")
    return out


def _split(out, names):
    """The caller's `out` tuple as one entry per name; `out` = None: all to be allocated."""
    if out is None:
        return (None,) * len(names)
    if len(out) != len(names):
        raise ValueError(f"out must be ({', '.join(names)})")
    for name, t in zip(names, out):
        if t is None:  # (None would read as "allocate one": the caller gives every output or none)
            raise ValueError(f"out[{name}] is None: out must be ({', '.join(names)}), every one a tensor")
    return tuple(out)


def parse_channels(channels=_lib.DEFAULT_POLICY_CHANNELS):
    """The channel list of policy_input() as a tuple of PGX_CHANNEL_* codes, in the caller's order; the default is the
    seven-plane input: the observation, then the four direction planes.  Anything but a sequence of 1..8 distinct names of
    _lib.POLICY_CHANNELS is a ValueError that names the offending entry and lists the vocabulary.  Needs no engine and
    no GPU."""
    table = _lib.POLICY_CHANNELS
    known = f"the channels are {', '.join(repr(n) for n in table)}"
    if isinstance(channels, (str, bytes)) or not isinstance(channels, (tuple, list)):
        raise ValueError(f"channels must be a tuple or list of 1..{_lib.NUM_CHANNELS} channel names, got {channels!r}; {known}")
    if not 1 <= len(channels) <= _lib.NUM_CHANNELS:
        raise ValueError(f"channels must hold 1..{_lib.NUM_CHANNELS} names, got {len(channels)}; {known}")
    codes = []
    for k, name in enumerate(channels):
        if not isinstance(name, str) or name not in table:
            raise ValueError(f"channels[{k}] = {name!r} is not a channel; {known}")
        if table[name] in codes:
            raise ValueError(f"channels[{k}] = {name!r} is given twice; {known}")
        codes.append(table[name])
    return tuple(codes)


def parse_global_channels(channels=_lib.DEFAULT_GLOBAL_CHANNELS):
    """The channel list of global_state() as a tuple of PGX_GLOBAL_* codes, in the caller's order; the default is the
    three binary planes.  Anything but a sequence of 1..5 distinct names of _lib.GLOBAL_CHANNELS is a ValueError that names
    the offending entry and lists the vocabulary.  Needs no engine and no GPU."""
    table = _lib.GLOBAL_CHANNELS
    known = f"the channels are {', '.join(repr(n) for n in table)}"
    if isinstance(channels, (str, bytes)) or not isinstance(channels, (tuple, list)):
        raise ValueError(f"channels must be a tuple or list of 1..{_lib.NUM_GLOBAL_CHANNELS} channel names, got {channels!r}; {known}")
    if not 1 <= len(channels) <= _lib.NUM_GLOBAL_CHANNELS:
        raise ValueError(f"channels must hold 1..{_lib.NUM_GLOBAL_CHANNELS} names, got {len(channels)}; {known}")
    codes = []
    for k, name in enumerate(channels):
        if not isinstance(name, str) or name not in table:
            raise ValueError(f"channels[{k}] = {name!r} is not a channel; {known}")
        if table[name] in codes:
            raise ValueError(f"channels[{k}] = {name!r} is given twice; {known}")
        codes.append(table[name])
    return tuple(codes)


def check_global_ids(codes, dtype, num_agents):
    """global_state()'s id-range rule: with an id channel among `codes`, `dtype` must hold every id 1..num_agents
    exactly -- uint8 up to 255 agents, bfloat16 up to 256; float16 and float32 hold every count the engine accepts.
    Otherwise a ValueError that names the limit.  Needs no engine and no GPU."""
    limit = _lib.GLOBAL_ID_MAX.get(_lib.OBS_DTYPES[dtype])
    if limit is not None and num_agents > limit and any(_lib.GLOBAL_CHANNELS[n] in codes for n in _lib.GLOBAL_ID_CHANNELS):
        raise ValueError(f"an id channel in {str(dtype).replace('torch.', '')} holds at most {limit} agents exactly, the env "
                         f"has {num_agents}: use torch.float16 or torch.float32")


def parse_forecast_steps(steps=3):
    """The `steps` of agent_forecasts() as an int: an integer (a bool is none) in 1.._lib.MAX_FORECAST_STEPS, anything
    else is a ValueError that names the range.  Needs no engine and no GPU."""
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= _lib.MAX_FORECAST_STEPS:
        raise ValueError(f"steps must be an integer in 1..{_lib.MAX_FORECAST_STEPS}, got {steps!r}")
    return int(steps)


def parse_forecast_format(format="float32"):
    """The `format` of agent_forecasts() as (PGX_FORECAST_* code, the planes' dtype, True when a plane is one int32 word
    per row); a name outside _lib.FORECAST_FORMATS is a ValueError that lists the table.  Needs no engine and no GPU."""
    if not isinstance(format, str) or format not in _lib.FORECAST_FORMATS:
        raise ValueError(f"format must be one of {sorted(_lib.FORECAST_FORMATS)}, got {format!r}")
    dtype = {"float32": torch.float32, "uint8": torch.uint8, "rows": torch.int32}[format]
    return _lib.FORECAST_FORMATS[format], dtype, format == "rows"


def parse_blocking_inflation(inflation=10):
    """The `inflation` of blocking() as an int: an integer (a bool is none) in 1.._lib.MAX_BLOCKING_INFLATION.  Anything
    that is no integer is a TypeError, an integer outside the range a ValueError that names it.  Needs no engine and no
    GPU."""
    if isinstance(inflation, bool) or not isinstance(inflation, (int, np.integer)):
        raise TypeError(f"inflation must be an integer in 1..{_lib.MAX_BLOCKING_INFLATION}, got {type(inflation).__name__}")
    if not 1 <= inflation <= _lib.MAX_BLOCKING_INFLATION:
        raise ValueError(f"inflation must be an integer in 1..{_lib.MAX_BLOCKING_INFLATION}, got {inflation!r}")
    return int(inflation)


def parse_blockers(blockers="all"):
    """The `blockers` of blocking() as pgx_blocking's flags; a name outside _lib.BLOCKING_BLOCKERS is a ValueError that
    lists the vocabulary.  Needs no engine and no GPU."""
    if not isinstance(blockers, str) or blockers not in _lib.BLOCKING_BLOCKERS:
        raise ValueError(f"blockers must be one of {sorted(_lib.BLOCKING_BLOCKERS)}, got {blockers!r}")
    return _lib.BLOCKING_BLOCKERS[blockers]


def parse_conflict_kinds(kinds=("vertex", "edge")):
    """The `kinds` of path_conflicts() as the OR of their PGX_CONFLICT_* bits: a non-empty tuple or list of distinct names
    of _lib.CONFLICT_KINDS, anything else is a ValueError that lists the vocabulary.  Needs no engine and no GPU."""
    table = _lib.CONFLICT_KINDS
    known = f"the kinds are {', '.join(repr(n) for n in table)}"
    if isinstance(kinds, (str, bytes)) or not isinstance(kinds, (tuple, list)) or not kinds:
        raise ValueError(f"kinds must be a non-empty tuple or list of conflict kinds, got {kinds!r}; {known}")
    bits = 0
    for k, name in enumerate(kinds):
        if not isinstance(name, str) or name not in table:
            raise ValueError(f"kinds[{k}] = {name!r} is not a conflict kind; {known}")
        if bits & table[name]:
            raise ValueError(f"kinds[{k}] = {name!r} is given twice; {known}")
        bits |= table[name]
    return bits


def parse_conflict_arrived(arrived=None):
    """The `arrived` of path_conflicts() as pgx_path_conflicts' arrival flag (0: the engine's on_target decides); anything
    outside _lib.CONFLICT_ARRIVED is a ValueError that lists the vocabulary.  Needs no engine and no GPU."""
    if not (arrived is None or isinstance(arrived, str)) or arrived not in _lib.CONFLICT_ARRIVED:
        raise ValueError(f"arrived must be None, 'stay' or 'vanish', got {arrived!r}")
    return _lib.CONFLICT_ARRIVED[arrived]


class QueryMixin:
    """The queries of a VecPogema.  Expects of the class it is mixed into: `_handle`, `_lib`, `device`, `batch`,
    `num_agents`, `window`, `height`, `width`, `_ACTION_CODE`, `_prepare_actions()`, `_stream()`."""

    _SCORE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}  # PGX_SCORES_* of shield_actions' scores

    def _action_dtypes(self, dtype, actions):
        """The dtypes the `actions` output may have: the caller's tensor decides, else `dtype`."""
        if actions is not None:
            return tuple(self._ACTION_CODE)
        if dtype not in self._ACTION_CODE:
            raise ValueError(f"dtype must be one of torch.int8, torch.int32, torch.int64, got {dtype}")
        return dtype

    def expert_actions(self, agents_as_obstacles: bool = False, dtype=torch.int64, out=None):
        """Shortest-path expert (docs/SPEC.md "Shortest-path expert"), computed on the device from the current state --
        the state the next step() reads, which this call leaves untouched.  Returns (actions [batch, agents] of `dtype`,
        distance int32 [batch, agents]): distance is the 4-connected BFS distance from each agent to its target over the
        map's free cells (0 on the target, -1 without a path or for an inactive agent); the action is the lowest of
        1..4 (up, down, left, right) that lowers it, 0 when the distance is <= 0.  `agents_as_obstacles=True`: the
        cells of the other active agents are blocked too.  Stream-ordered, no host sync, capturable in a HIP graph.
        `out=(actions, distance)`: caller-owned contiguous tensors on this device (actions int8 / int32 / int64)."""
        B, A = self.batch, self.num_agents
        actions, distance = _split(out, ("actions", "distance"))
        actions = query_output("out[actions]", actions, self._action_dtypes(dtype, actions), (B, A), self.device)
        distance = query_output("out[distance]", distance, torch.int32, (B, A), self.device)
        _lib.check(self._lib.pgx_expert_actions(self._handle, 1 if agents_as_obstacles else 0, actions.data_ptr(),
                                                self._ACTION_CODE[actions.dtype], distance.data_ptr(), self._stream()))
        return actions, distance

    def cost_to_go(self, out=None) -> torch.Tensor:
        """Cost-to-go windows (docs/SPEC.md S11), computed on the device from the current state -- the state the next
        step() reads, which this call leaves untouched.  Returns int32 [batch, agents, W, W] (W = 2 * obs_radius + 1, the
        orientation of observation plane 0): the 4-connected BFS distance from each window cell to the agent's target
        over the map's free cells; -1 outside the map, on obstacles, for unreachable cells and for every cell of an
        inactive agent.  The centre equals expert_actions()' distance.  One distance field per agent is cached on the
        device and rebuilt only when the agent's target cell or its env's map changed (cost_to_go_builds counts them).
        The first call allocates that cache (pgx_cost_to_go_bytes) and must be made outside a graph capture; later calls
        are stream-ordered, need no host sync and can be captured.  `out`: a caller-owned contiguous int32 tensor of
        that shape on this device."""
        shape = (self.batch, self.num_agents, self.window, self.window)
        out = query_output("out", out, torch.int32, shape, self.device)
        _lib.check(self._lib.pgx_cost_to_go(self._handle, 0, out.data_ptr(), self._stream()))
        return out

    @property
    def cost_to_go_builds(self) -> int:
        """Distance fields cost_to_go(), pibt_actions(), pibt_plan(), whca_plan(), repair_plan(), goal_directions(), goal_paths(), agent_forecasts(), blocking(), agent_tokens() and
        shield_actions(tie_break="distance") have built since this env was created (synchronises the stream)."""
        n = self._lib.pgx_cost_to_go_builds(self._handle, self._stream())
        if n < 0:
            _lib.check(int(n))
        return int(n)

    def visible_agents(self, k: int = 13, out=None):
        """Neighbour lists (docs/SPEC.md S12), computed on the device from the current state -- the state the next
        step() reads, which this call leaves untouched.  Agent j is visible to agent i of the same env iff j != i, j is
        active and |dx| <= obs_radius and |dy| <= obs_radius for (dx, dy) = xy_j - xy_i (the square observation window;
        obstacles hide nobody, as in observation plane 1); an inactive agent sees nobody.  The visible agents are ordered
        by (dx * dx + dy * dy, dx + r, dy + r, j): nearest first, ties in the window's row-major order, then by index.
        Returns (index int32 [batch, agents, k]: the first min(count, k) of them, then -1;
                 offset int8 [batch, agents, k, 2]: their (dx, dy), (0, 0) where index is -1;
                 count int32 [batch, agents]: the number of visible agents, not capped by k).
        `k` is 1..MAX_NEIGHBOURS (32).  One kernel launch: allocates nothing on the engine side, stream-ordered, no host
        sync, capturable in a HIP graph from the first call.  `out=(index, offset, count)`: caller-owned contiguous
        tensors of those dtypes and shapes on this device."""
        B, A = self.batch, self.num_agents
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _lib.MAX_NEIGHBOURS:
            raise ValueError(f"k must be an integer in 1..{_lib.MAX_NEIGHBOURS}, got {k!r}")
        k = int(k)
        index, offset, count = _split(out, ("index", "offset", "count"))
        index = query_output("out[index]", index, torch.int32, (B, A, k), self.device)
        offset = query_output("out[offset]", offset, torch.int8, (B, A, k, 2), self.device, align=2)
        count = query_output("out[count]", count, torch.int32, (B, A), self.device)
        _lib.check(self._lib.pgx_visible_agents(self._handle, k, 0, index.data_ptr(), offset.data_ptr(), count.data_ptr(),
                                                self._stream()))
        return index, offset, count

    def _priority(self, priority):
        """The planners' `priority` argument as a contiguous int32 tensor [batch, agents], or None."""
        if priority is None:
            return None
        shape = (self.batch, self.num_agents)
        if not isinstance(priority, torch.Tensor):
            raise TypeError(f"priority must be a torch.Tensor or None, got {type(priority).__name__}")
        if priority.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
            raise TypeError(f"priority must be an integer tensor, got {priority.dtype}")
        if tuple(priority.shape) != shape or priority.device != self.device:
            raise ValueError(f"priority must have shape {shape} on {self.device}")
        return priority.to(torch.int32).contiguous()

    def pibt_actions(self, priority=None, dtype=torch.int64, out=None, *, swap=False):
        """Cooperative one-step planner (PIBT, docs/SPEC.md S13), computed on the device from the current state -- the
        state the next step() reads, which this call leaves untouched.  Returns (actions [batch, agents] of `dtype`,
        next_xy int32 [batch, agents, 2]: the cell each agent is sent to, unpadded (row, col)).  Every active agent gets
        one of its own cell and its free neighbours, preferred by the distance to its target (cost_to_go()'s fields),
        agents served by (-priority, index), with priority inheritance and backtracking: no two active agents get the
        same cell and no two swap.  Inactive agents get action 0 and their own cell.  Under collision_system="soft"
        step(actions) puts every active agent on its next_xy; under "priority" and "block_both" a move into a cell that
        another agent leaves in the same step may be reverted.
        `priority`: an integer tensor [batch, agents] on this device (converted to int32), None = all equal.
        Shares cost_to_go()'s cache: whichever is called first allocates it (not inside a graph capture); later calls are
        stream-ordered, need no host sync and can be captured.  `out=(actions, next_xy)`: caller-owned contiguous
        tensors on this device (actions int8 / int32 / int64, next_xy int32).
        `swap=True`: the planner with the swap operation (docs/SPEC.md S23, pgx_pibt_swap_actions) -- an agent that has
        to pass another one in a corridor or a dead end tries its cells back to front and pulls the other agent into the
        cell it leaves, which ends the livelocks of the plain rule there.  Same arguments, outputs, guarantees and cache
        rules; a heuristic that loses a few instances the plain rule solves, hence opt-in."""
        B, A = self.batch, self.num_agents
        if not isinstance(swap, (bool, np.bool_)):
            raise TypeError(f"swap must be a bool, got {type(swap).__name__}")
        priority = self._priority(priority)
        actions, next_xy = _split(out, ("actions", "next_xy"))
        actions = query_output("out[actions]", actions, self._action_dtypes(dtype, actions), (B, A), self.device)
        next_xy = query_output("out[next_xy]", next_xy, torch.int32, (B, A, 2), self.device)
        call = self._lib.pgx_pibt_swap_actions if swap else self._lib.pgx_pibt_actions
        _lib.check(call(self._handle, 0, priority.data_ptr() if priority is not None else None, actions.data_ptr(),
                        self._ACTION_CODE[actions.dtype], next_xy.data_ptr(), self._stream()))
        return actions, next_xy

    def pibt_plan(self, horizon, priority=None, growing: bool = True, dtype=torch.int64, out=None, *, swap=False):
        """Multi-step planner (docs/SPEC.md S16): pibt_actions()' planner iterated `horizon` times in one launch, on a
        private copy of the positions -- computed on the device from the current state, which the call leaves untouched.
        Step h plans from the cells step h - 1 sent the agents to; the targets are held for the whole lookahead.  Under
        on_target="finish" an agent is no longer planned once it has reached its target; under "nothing" and "restart" it
        stays planned on the same target.  Returns
            (actions [horizon, batch, agents] of `dtype`: what rollout(actions) takes;
             path_xy int32 [horizon, batch, agents, 2]: the cell each step sends each agent to, unpadded (row, col);
             arrival int32 [batch, agents]: the first h in 0..horizon after which the agent stands on its target, -1 when
                 it does not within the horizon or was inactive at the start;
             priority int32 [batch, agents]: the priorities after the last step, to continue from).
        `growing=True`: the textbook priorities, PibtPolicy.update()'s rule -- 0 when the agent's next cell is its target
        or it is not planned any more, else + 1 per step; False: `priority` is held for all steps.  pibt_actions()'
        guarantees hold for every step; with horizon = 1, actions[0] and path_xy[0] are pibt_actions()' outputs.
        Under collision_system="soft" with on_target "finish" or "nothing", rollout(actions) puts every agent on
        path_xy[h] after step h until the env's episode ends (the plan ignores max_episode_steps and auto-reset).  Under
        "restart" the plan is exact up to the first arrival in the env; under "priority" / "block_both" up to the first
        reverted move.
        `horizon`: an integer in 1..MAX_PLAN_HORIZON (256).  `priority`: as in pibt_actions().
        Shares cost_to_go()'s cache under pibt_actions()' rules, with one refresh per call whatever the horizon is.
        `out=(actions, path_xy, arrival, priority)`: caller-owned contiguous tensors on this device (actions int8 /
        int32 / int64, the others int32).
        `swap=True`: every step plans with the swap operation (docs/SPEC.md S27, pgx_pibt_swap_plan) -- the rule of
        pibt_actions(swap=True), evaluated on the positions and the planned agents of the step it plans, which takes a
        plan through the corridors and dead ends the plain lookahead livelocks in.  Same arguments, outputs, guarantees
        and cache rules; with horizon = 1, actions[0] and path_xy[0] are pibt_actions(swap=True)'s outputs."""
        B, A = self.batch, self.num_agents
        if not isinstance(swap, (bool, np.bool_)):
            raise TypeError(f"swap must be a bool, got {type(swap).__name__}")
        if (isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer))
                or not 1 <= horizon <= _lib.MAX_PLAN_HORIZON):
            raise ValueError(f"horizon must be an integer in 1..{_lib.MAX_PLAN_HORIZON}, got {horizon!r}")
        K = int(horizon)
        priority = self._priority(priority)
        actions, path_xy, arrival, priority_out = _split(out, ("actions", "path_xy", "arrival", "priority"))
        actions = query_output("out[actions]", actions, self._action_dtypes(dtype, actions), (K, B, A), self.device)
        path_xy = query_output("out[path_xy]", path_xy, torch.int32, (K, B, A, 2), self.device)
        arrival = query_output("out[arrival]", arrival, torch.int32, (B, A), self.device)
        priority_out = query_output("out[priority]", priority_out, torch.int32, (B, A), self.device)
        call = self._lib.pgx_pibt_swap_plan if swap else self._lib.pgx_pibt_plan
        _lib.check(call(self._handle, 0 if growing else _lib.PLAN_FIXED_PRIORITY, K,
                        priority.data_ptr() if priority is not None else None, actions.data_ptr(),
                        self._ACTION_CODE[actions.dtype], path_xy.data_ptr(), arrival.data_ptr(),
                        priority_out.data_ptr(), self._stream()))
        return actions, path_xy, arrival, priority_out

    def whca_plan(self, horizon, priority=None, dtype=torch.int64, out=None):
        """Windowed cooperative A* against a reservation table (WHCA*, docs/SPEC.md S28): prioritized planning in
        space-time, computed on the device from the current state, which the call leaves untouched.  The active agents
        of an env are served by (-priority, index); each gets a `horizon`-step path over the free cells that avoids
        every cell and every head-on move of the agents served before it.  Under on_target="finish" a path ends at the
        first step that can reach the target, and the agent reserves nothing afterwards; otherwise it ends at the cell
        reachable in `horizon` steps that is nearest to the target (cost_to_go()'s field, ties in row-major order), as
        early as the reservations allow, and waits there.  An agent whose search runs out of cells has failed: it
        stays on its cell, reserves it for the whole window, and later agents plan around it.  Returns
            (actions [horizon, batch, agents] of `dtype`: what rollout(actions) takes;
             path_xy int32 [horizon, batch, agents, 2]: the cell after each step, unpadded (row, col) -- pibt_plan()'s
                 layout, what path_conflicts() takes;
             arrival int32 [batch, agents]: the first h in 0..horizon at which the path stands on the target, -1 when
                 it does not, and for every inactive agent;
             failed int32 [batch, agents]: 1 for a failed agent, else 0).
        From a state with the active agents on distinct cells, no two agents that did not fail meet in a cell or swap
        cells at any step; in an env without a failed agent, under collision_system="soft" with on_target "finish" or
        "nothing", rollout(actions) puts every agent on path_xy[h] after step h until the env's episode ends.
        pibt_plan()'s caveats apply to "restart" (exact up to the first arrival) and to "priority" / "block_both"
        (exact up to the first reverted move).  Prioritized planning is incomplete: `failed` says where, and other
        priorities on the next call are the remedy.
        `horizon`: an integer in 1..MAX_WHCA_HORIZON (31).  `priority`: as in pibt_actions().
        Shares cost_to_go()'s cache under pibt_actions()' rules, with one refresh per call.
        `out=(actions, path_xy, arrival, failed)`: caller-owned contiguous tensors on this device (actions int8 /
        int32 / int64, the others int32)."""
        B, A = self.batch, self.num_agents
        if (isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer))
                or not 1 <= horizon <= _lib.MAX_WHCA_HORIZON):
            raise ValueError(f"horizon must be an integer in 1..{_lib.MAX_WHCA_HORIZON}, got {horizon!r}")
        K = int(horizon)
        priority = self._priority(priority)
        actions, path_xy, arrival, failed = _split(out, ("actions", "path_xy", "arrival", "failed"))
        actions = query_output("out[actions]", actions, self._action_dtypes(dtype, actions), (K, B, A), self.device)
        path_xy = query_output("out[path_xy]", path_xy, torch.int32, (K, B, A, 2), self.device)
        arrival = query_output("out[arrival]", arrival, torch.int32, (B, A), self.device)
        failed = query_output("out[failed]", failed, torch.int32, (B, A), self.device)
        _lib.check(self._lib.pgx_whca_plan(self._handle, 0, K, priority.data_ptr() if priority is not None else None,
                                           actions.data_ptr(), self._ACTION_CODE[actions.dtype], path_xy.data_ptr(),
                                           arrival.data_ptr(), failed.data_ptr(), self._stream()))
        return actions, path_xy, arrival, failed

    def repair_plan(self, paths, replan=None, priority=None, dtype=torch.int64, out=None):
        """Plan repair (docs/SPEC.md S29): whca_plan() for chosen agents, around the paths the others keep -- the repair
        step of an LNS-style solver, and a receding-horizon replan of only the agents whose plan went stale.  Computed
        on the device from the current state, which the call leaves untouched.
        `paths`: int32 [K, batch, agents, 2] on this device, contiguous -- a plan in pibt_plan()'s / whca_plan()'s
        path_xy layout (the cell after step h + 1 at index h, unpadded (row, col)); K, 1..MAX_WHCA_HORIZON (31), is the
        horizon.  The cells may be any int32.  An active agent's given path is a walk when every cell lies inside the
        map, is no obstacle and is the cell before it or one of its four neighbours, the first one counted from the
        agent's cell; under on_target="finish" only up to the first step on the agent's target, which is its last step
        (what `paths` holds afterwards is ignored), else up to K.
        `replan`: bool / uint8 [batch, agents] on this device, contiguous; None = nobody is asked for.
        An active agent with replan == 0 whose given path is a walk is kept: all kept agents' cells and moves are reserved
        first (up to their last step; conflicts among them are not looked for: that is path_conflicts()' job).  Every
        other active agent is replanned: served by (-priority, index) exactly as whca_plan() serves an agent, against
        the kept agents and the replanned agents served before it.  Returns
            (actions [K, batch, agents] of `dtype`: a kept agent walks its given path up to its last step, then 0;
             path_xy int32 [K, batch, agents, 2]: a kept agent's given cells, its last cell after its last step;
             arrival int32 [batch, agents]: whca_plan()'s rule on path_xy;
             failed int32 [batch, agents]: 1 for a replanned agent whose search ran empty, else 0;
             replanned int32 [batch, agents]: 1 for every replanned agent -- asked for or not a walk -- else 0).
        With replan all ones the first four are whca_plan(K, priority)'s.  whca_plan()'s own path_xy with its last m
        agents of the service order replanned under the same priorities gives that plan again; with replan=None it is
        returned unchanged and nobody is replanned.  From distinct start cells, where the kept agents are free of
        conflicts among themselves and nobody failed, the result has no vertex and no edge conflict and whca_plan()'s
        statement about rollout(actions) holds, with its caveats.
        `priority`: as in pibt_actions().  Shares cost_to_go()'s cache under pibt_actions()' rules, with one refresh per
        call.  `out=(actions, path_xy, arrival, failed, replanned)`: caller-owned contiguous tensors on this device
        (actions int8 / int32 / int64, the others int32); out[path_xy] may be `paths` itself (the repair in place), any
        other overlap of an output with `paths` is refused."""
        B, A = self.batch, self.num_agents
        if not isinstance(paths, torch.Tensor) or paths.dtype != torch.int32:
            raise TypeError(f"paths must be an int32 torch.Tensor, got "
                            f"{paths.dtype if isinstance(paths, torch.Tensor) else type(paths).__name__}")
        if (paths.dim() != 4 or tuple(paths.shape[1:]) != (B, A, 2) or not 1 <= paths.shape[0] <= _lib.MAX_WHCA_HORIZON
                or not paths.is_contiguous() or paths.device != self.device or paths.data_ptr() % 4):
            raise ValueError(f"paths must be a contiguous int32 tensor of shape (K, {B}, {A}, 2) with K in "
                             f"1..{_lib.MAX_WHCA_HORIZON} on {self.device}, got shape {tuple(paths.shape)}")
        K = int(paths.shape[0])
        if replan is not None:
            if not isinstance(replan, torch.Tensor) or replan.dtype not in (torch.bool, torch.uint8):
                raise TypeError(f"replan must be a bool or uint8 torch.Tensor or None, got "
                                f"{replan.dtype if isinstance(replan, torch.Tensor) else type(replan).__name__}")
            if tuple(replan.shape) != (B, A) or replan.device != self.device or not replan.is_contiguous():
                raise ValueError(f"replan must be a contiguous tensor of shape {(B, A)} on {self.device}")
        priority = self._priority(priority)
        names = ("actions", "path_xy", "arrival", "failed", "replanned")
        actions, path_xy, arrival, failed, replanned = _split(out, names)
        actions = query_output("out[actions]", actions, self._action_dtypes(dtype, actions), (K, B, A), self.device)
        path_xy = query_output("out[path_xy]", path_xy, torch.int32, (K, B, A, 2), self.device)
        arrival = query_output("out[arrival]", arrival, torch.int32, (B, A), self.device)
        failed = query_output("out[failed]", failed, torch.int32, (B, A), self.device)
        replanned = query_output("out[replanned]", replanned, torch.int32, (B, A), self.device)
        if out is not None:
            lo, hi = paths.data_ptr(), paths.data_ptr() + paths.numel() * 4
            for name, t in zip(names, (actions, path_xy, arrival, failed, replanned)):
                if name == "path_xy" and t.data_ptr() == lo:      # the same buffer (shape and strides were checked)
                    continue
                if t.data_ptr() < hi and lo < t.data_ptr() + t.numel() * t.element_size():
                    raise ValueError(f"out[{name}] overlaps paths: only out[path_xy] may, as the same tensor")
        _lib.check(self._lib.pgx_repair_plan(self._handle, 0, K, paths.data_ptr(),
                                             replan.data_ptr() if replan is not None else None,
                                             priority.data_ptr() if priority is not None else None, actions.data_ptr(),
                                             self._ACTION_CODE[actions.dtype], path_xy.data_ptr(), arrival.data_ptr(),
                                             failed.data_ptr(), replanned.data_ptr(), self._stream()))
        return actions, path_xy, arrival, failed, replanned

    def shield_actions(self, scores, priority=None, tie_break=None, dtype=torch.int64, out=None):
        """Collision shielding (docs/SPEC.md S15): pibt_actions()' planner with every agent's candidate cells ordered by
        a policy's action scores instead of by the distance to its target -- each active agent gets the best-scored
        action that is jointly collision-free.  Computed on the device from the current state, which the call leaves
        untouched.  Returns (actions [batch, agents] of `dtype`, next_xy int32 [batch, agents, 2], overridden uint8
        [batch, agents]: 1 where an active agent's action is not the argmax of its scores).
        `scores`: float32 / float16 / bfloat16 [batch, agents, 5] on this device (made contiguous if it is not), one
        score per action, higher is better; then the lower action.  -0.0 equals +0.0, infinities are ordinary values, a
        NaN ranks lowest.  Moves off the map or into an obstacle are dropped whatever their score, so the call is also
        the action mask.  pibt_actions()' guarantees (no shared next cell, no swap, under collision_system="soft" every
        active agent lands on its next_xy) hold for any scores.  The call is deterministic; to sample, pass
        `logits + gumbel_noise`: taking candidates in that order is Plackett-Luce sampling without replacement.
        `priority`: as in pibt_actions().  `tie_break`: None, or "distance": equal scores are ordered as pibt_actions()
        orders its candidates (with constant scores the result is pibt_actions()' exactly).
        tie_break=None reads no distance field: one launch that allocates nothing, stream-ordered, no host sync,
        capturable in a HIP graph from the first call.  tie_break="distance" shares cost_to_go()'s cache under
        pibt_actions()' rules (whichever call is first allocates it, not inside a graph capture).
        `out=(actions, next_xy, overridden)`: caller-owned contiguous tensors on this device (actions int8 / int32 /
        int64, next_xy int32, overridden uint8)."""
        B, A = self.batch, self.num_agents
        if not isinstance(scores, torch.Tensor):
            raise TypeError(f"scores must be a torch.Tensor, got {type(scores).__name__}")
        if scores.dtype not in self._SCORE_CODE:
            raise TypeError(f"scores must be a float32, float16 or bfloat16 tensor, got {scores.dtype}")
        if tuple(scores.shape) != (B, A, 5) or scores.device != self.device:
            raise ValueError(f"scores must have shape {(B, A, 5)} on {self.device}")
        if tie_break not in _lib.SHIELD_TIE_BREAKS:
            raise ValueError(f"tie_break must be None or 'distance', got {tie_break!r}")
        scores = scores.contiguous()
        priority = self._priority(priority)
        actions, next_xy, overridden = _split(out, ("actions", "next_xy", "overridden"))
        actions = query_output("out[actions]", actions, self._action_dtypes(dtype, actions), (B, A), self.device)
        next_xy = query_output("out[next_xy]", next_xy, torch.int32, (B, A, 2), self.device)
        overridden = query_output("out[overridden]", overridden, torch.uint8, (B, A), self.device)
        _lib.check(self._lib.pgx_shield_actions(self._handle, _lib.SHIELD_TIE_BREAKS[tie_break], scores.data_ptr(),
                                                self._SCORE_CODE[scores.dtype], priority.data_ptr() if priority is not None else None,
                                                actions.data_ptr(), self._ACTION_CODE[actions.dtype], next_xy.data_ptr(),
                                                overridden.data_ptr(), self._stream()))
        return actions, next_xy, overridden

    def goal_directions(self, format: str = "float32", out=None) -> torch.Tensor:
        """Direction-to-goal planes (docs/SPEC.md S14), the "heuristic channels" of DHC-style policies, computed on the
        device from the current state -- the state the next step() reads, which this call leaves untouched.  Plane
        a - 1 of an agent's window (W = 2 * obs_radius + 1, the orientation of observation plane 0) is 1 at a cell iff
        move a (1..4: up, down, left, right) from that cell leads to a cell strictly closer to the agent's target; the
        cell moved to is looked up in the agent's whole distance field, so the window's edge is exact.  All four are 0
        on the target, wherever cost_to_go() gives -1 and for inactive agents.  The lowest plane set at the centre is
        expert_actions()' action.
        `format`: "float32" -> float32 [batch, agents, 4, W, W] of 0.0 / 1.0, ready for torch.cat behind the observation;
                  "uint8"   -> uint8 [batch, agents, 4, W, W] of 0 / 1;
                  "bits"    -> uint8 [batch, agents, W, W], bit a - 1 = plane a - 1.
        Shares cost_to_go()'s cache: whichever of cost_to_go(), pibt_actions() and this is called first allocates it
        (not inside a graph capture); later calls are stream-ordered, need no host sync and can be captured.  `out`: a
        caller-owned contiguous tensor of that dtype and shape on this device."""
        if format not in _lib.DIRECTIONS_FORMATS:
            raise ValueError(f"format must be one of {sorted(_lib.DIRECTIONS_FORMATS)}, got {format!r}")
        dtype = torch.float32 if format == "float32" else torch.uint8
        planes = () if format == "bits" else (4,)
        shape = (self.batch, self.num_agents) + planes + (self.window, self.window)
        out = query_output("out", out, dtype, shape, self.device)
        _lib.check(self._lib.pgx_goal_directions(self._handle, 0, out.data_ptr(), _lib.DIRECTIONS_FORMATS[format],
                                                 self._stream()))
        return out

    def goal_paths(self, steps=None, format: str = "float32", planes: bool = True, out=None):
        """Path-to-goal planes and sub-goals (docs/SPEC.md S22), the input and the reward signal of planning-plus-learning
        policies ("Learn to Follow" style), computed on the device from the current state -- the state the next step()
        reads, which this call leaves untouched.  An agent's path descends its distance field from its own cell: at
        every cell the lowest of the moves 1..4 (up, down, left, right) that leads to a cell strictly closer to the
        target -- the lowest plane goal_directions() sets there, so its first cell is the one expert_actions() moves to.
        The cells p1..pn are marked until the target is reached, the next cell would leave the agent's window (nothing
        after it is marked, even if the path re-enters) or n = `steps`.  Returns
            (planes [batch, agents, W, W] (W = 2 * obs_radius + 1, the orientation of observation plane 0): 1 on the
                 marked cells; the centre is never marked, the target is when reached.  None with `planes=False`;
             subgoal int8 [batch, agents, 2]: the offset (dx, dy) of the last marked cell from the agent, in
                 visible_agents()' convention;
             length int32 [batch, agents]: n; at most cost_to_go()'s centre value, equal iff the path ended on the target).
        An agent that is inactive, stands on its target or has no path to it gets zero planes, (0, 0) and 0.
        `steps`: None = no cap, or an integer in 1..MAX_PATH_STEPS (960).
        `format`: "float32" -> float32 [batch, agents, W, W] of 0.0 / 1.0;
                  "uint8"   -> uint8 [batch, agents, W, W] of 0 / 1;
                  "rows"    -> int32 [batch, agents, W], bit v of word u = cell (u, v).
        `planes=False` writes no planes at all: the sub-goals and lengths alone.
        Shares cost_to_go()'s cache under goal_directions()' rules: stale fields are rebuilt first, whichever call is
        first allocates the cache (not inside a graph capture); later calls are stream-ordered, need no host sync and can
        be captured.  `out=(planes, subgoal, length)`, with `planes=False` `out=(subgoal, length)`: caller-owned
        contiguous tensors of those dtypes and shapes on this device; a 16-byte aligned `planes` is written fastest."""
        B, A, W = self.batch, self.num_agents, self.window
        if format not in _lib.PATHS_FORMATS:
            raise ValueError(f"format must be one of {sorted(_lib.PATHS_FORMATS)}, got {format!r}")
        if steps is not None and (isinstance(steps, bool) or not isinstance(steps, (int, np.integer))
                                  or not 1 <= steps <= _lib.MAX_PATH_STEPS):
            raise ValueError(f"steps must be None or an integer in 1..{_lib.MAX_PATH_STEPS}, got {steps!r}")
        if planes:
            plane_out, subgoal, length = _split(out, ("planes", "subgoal", "length"))
            dtype = {"float32": torch.float32, "uint8": torch.uint8, "rows": torch.int32}[format]
            shape = (B, A, W) if format == "rows" else (B, A, W, W)
            plane_out = query_output("out[planes]", plane_out, dtype, shape, self.device)
        else:
            plane_out = None
            subgoal, length = _split(out, ("subgoal", "length"))
        subgoal = query_output("out[subgoal]", subgoal, torch.int8, (B, A, 2), self.device)
        length = query_output("out[length]", length, torch.int32, (B, A), self.device)
        _lib.check(self._lib.pgx_goal_paths(self._handle, 0, 0 if steps is None else int(steps), _lib.PATHS_FORMATS[format],
                                            plane_out.data_ptr() if plane_out is not None else None, subgoal.data_ptr(),
                                            length.data_ptr(), self._stream()))
        return plane_out, subgoal, length

    def agent_forecasts(self, steps: int = 3, format: str = "float32", planes: bool = True, out=None):
        """Agent forecasts (docs/SPEC.md S24), the planes PRIMAL2-style policies add to their input: where the other
        agents an observer can see are going to be at t+1 .. t+K (K = `steps`) if each follows its own shortest path --
        computed on the device from the current state, the state the next step() reads, which this call leaves
        untouched.  An agent's forecast descends its distance field from its own cell for K steps: at every cell the
        lowest of the moves 1..4 (up, down, left, right) that leads to a cell strictly closer to the target -- goal_paths()'
        rule with no window ending it, so its first cell is the one expert_actions() moves to -- and it waits where nothing
        is closer (on the target, or without a path).  Other agents are not obstacles.  Returns
            (planes [batch, agents, K, W, W] (W = 2 * obs_radius + 1, the orientation of observation plane 0): plane s-1
                 of an active observer is 1 on the window cells that hold the step-s forecast cell of another active
                 agent it sees now (visible_agents()' rule; every such agent, however many).  A forecast cell outside
                 the window is not drawn, the observer's own forecast is not in its planes, an inactive observer gets
                 zeros.  None with `planes=False`;
             cells int16 [batch, agents, K, 2]: every agent's own forecast cells (x, y) in get_state()'s coordinates;
                 (-1, -1) for an inactive agent).
        `steps`: an integer in 1..MAX_FORECAST_STEPS (8).
        `format`: "float32" -> float32 [batch, agents, K, W, W] of 0.0 / 1.0;
                  "uint8"   -> uint8 [batch, agents, K, W, W] of 0 / 1;
                  "rows"    -> int32 [batch, agents, K, W], bit v of word u = cell (u, v).
        `planes=False` writes no planes at all: the cells alone, in one launch instead of two.
        Shares cost_to_go()'s cache under goal_paths()' rules: stale fields are rebuilt first, whichever call is first
        allocates the cache (not inside a graph capture); later calls are stream-ordered, need no host sync and can be
        captured.  `out=(planes, cells)`, with `planes=False` `out=(cells,)`: caller-owned contiguous tensors of those
        dtypes and shapes on this device; a 16-byte aligned `planes` is written fastest."""
        B, A, W = self.batch, self.num_agents, self.window
        code, dtype, rows = parse_forecast_format(format)
        K = parse_forecast_steps(steps)
        if planes:
            plane_out, cells = _split(out, ("planes", "cells"))
            plane_out = query_output("out[planes]", plane_out, dtype, (B, A, K, W) if rows else (B, A, K, W, W), self.device)
        else:
            plane_out = None
            cells, = _split(out, ("cells",))
        cells = query_output("out[cells]", cells, torch.int16, (B, A, K, 2), self.device)
        _lib.check(self._lib.pgx_agent_forecasts(self._handle, K, code, 0,
                                                 plane_out.data_ptr() if plane_out is not None else None, cells.data_ptr(),
                                                 self._stream()))
        return plane_out, cells

    def blocking(self, inflation: int = 10, blockers: str = "all", out=None):
        """Blocking counts (docs/SPEC.md S25), the blocking penalty of PRIMAL / PRIMAL2 / SCRIMP style rewards: which
        agents stand in the way of others -- computed on the device from the current state, the state the next step()
        reads, which this call leaves untouched.  Agent i blocks agent j of the same env iff both are active, i sees j
        (visible_agents()' rule; every such agent, however many), j has a path to its target at all, they stand on
        different cells and, on the map with i's cell made an obstacle, j has no path to its target of fewer than
        `inflation` steps more than its shortest one: a detour of at least `inflation` steps, a cut-off agent and an
        agent sitting on j's target alike.  Other agents are never obstacles for these paths.  Returns
            (count int32 [batch, agents]: the number of agents that agent i blocks;
             blocked_by int32 [batch, agents]: the number of agents that block agent j).
        Inactive agents get 0 in both; per env the two have the same sum.
        `inflation`: an integer in 1..MAX_BLOCKING_INFLATION (64); PRIMAL uses 10; 1 asks whether i stands on every
        shortest path of j.  `blockers`: "all", or "on_target": only agents standing on their own target block.
        A pair whose blocker lies on no shortest path of j is dismissed from the cached distance fields alone; the
        others take one bounded search each.  Shares cost_to_go()'s cache under goal_paths()' rules: stale fields are
        rebuilt first, whichever call is first allocates the cache (not inside a graph capture); later calls are
        stream-ordered, need no host sync and can be captured.  `out=(count, blocked_by)`: caller-owned contiguous int32
        tensors of that shape on this device."""
        B, A = self.batch, self.num_agents
        inflation = parse_blocking_inflation(inflation)
        flags = parse_blockers(blockers)
        count, blocked_by = _split(out, ("count", "blocked_by"))
        count = query_output("out[count]", count, torch.int32, (B, A), self.device)
        blocked_by = query_output("out[blocked_by]", blocked_by, torch.int32, (B, A), self.device)
        _lib.check(self._lib.pgx_blocking(self._handle, inflation, flags, count.data_ptr(), blocked_by.data_ptr(),
                                          self._stream()))
        return count, blocked_by

    def path_conflicts(self, paths=None, steps: int = 3, kinds=("vertex", "edge"), arrived=None, out=None):
        """Path conflicts (docs/SPEC.md S26): where K-step paths run into each other, per agent -- computed on the device
        from the current state, the state the next step() reads, and `paths`; the call changes neither.
        `paths`: K cells per agent as unpadded (x, y) in get_state()'s coordinates, contiguous, on this device, K in
        1..MAX_CONFLICT_STEPS (256), in one of two layouts told apart by dtype:
            int32 [K, batch, agents, 2]  -- pibt_plan()'s path_xy;
            int16 [batch, agents, K, 2]  -- agent_forecasts()' cells.
        None: agent_forecasts(steps, planes=False)'s cells, `steps` in 1..8 (with its cache contract and first-call
        rule); `steps` is ignored when `paths` is given.  Cells are keys, not moves: the call does not judge whether a
        path is legal, and a cell outside the map (a (-1, -1)) takes no part at its step.
        With pos_0 the current cell and pos_h the path's cell h, an agent takes part at step h iff it is active, pos_h
        lies inside the map and, under arrived="vanish", no earlier pos_h' (h' < h, the current cell included) is its
        target.  Conflicts at h = 1..K between two agents that take part (for edge and follow: at h and at h - 1):
            "vertex"  both are on one cell at h;
            "edge"    they change places between h - 1 and h;
            "follow"  this agent moves to the cell the other one leaves for a third cell (on the follower only).
        `kinds`: a non-empty tuple or list of those names: the kinds that exist for this call.  "follow" is opt-in: only
        the `priority` and `block_both` collision systems revert such moves.
        `arrived`: "stay", "vanish" or None: "vanish" iff the engine's on_target is "finish", pibt_plan()'s rule.
        Returns (first_step int32 [batch, agents]: the first step with a conflict of this agent, -1 if none;
                 partner int32 [batch, agents]: the lowest agent it conflicts with at that step, -1 if none;
                 kind uint8 [batch, agents]: the OR of pogema_amd.CONFLICT_KINDS' bits over its conflicts at that step;
                 count int32 [batch, agents]: its conflicts (pairs of a step and another agent) over all K steps).
        An inactive agent gets -1, -1, 0, 0.  One launch that reads no distance field and allocates nothing on the engine
        side: with `paths` given it is stream-ordered, needs no host sync and is capturable in a HIP graph from the first
        call.  `out=(first_step, partner, kind, count)`: caller-owned contiguous tensors of those dtypes and shapes on
        this device."""
        B, A = self.batch, self.num_agents
        flags = parse_conflict_kinds(kinds) | parse_conflict_arrived(arrived)
        if paths is None:
            _, paths = self.agent_forecasts(parse_forecast_steps(steps), planes=False)
        if not isinstance(paths, torch.Tensor) or paths.dtype not in (torch.int32, torch.int16):
            raise TypeError("paths must be an int32 [K, batch, agents, 2] or an int16 [batch, agents, K, 2] tensor, got "
                            f"{paths.dtype if isinstance(paths, torch.Tensor) else type(paths).__name__}")
        plan = paths.dtype == torch.int32
        K = paths.shape[0 if plan else 2] if paths.dim() == 4 else 0
        want = (K, B, A, 2) if plan else (B, A, K, 2)
        if not (1 <= K <= _lib.MAX_CONFLICT_STEPS and tuple(paths.shape) == want and paths.is_contiguous()
                and paths.device == torch.device(self.device)):
            raise ValueError(f"paths must be a contiguous {'int32' if plan else 'int16'} tensor of shape "
                             f"{('K', B, A, 2) if plan else (B, A, 'K', 2)} with K in 1..{_lib.MAX_CONFLICT_STEPS} on "
                             f"{self.device}, got shape {tuple(paths.shape)} on {paths.device}")
        first_step, partner, kind, count = _split(out, ("first_step", "partner", "kind", "count"))
        first_step = query_output("out[first_step]", first_step, torch.int32, (B, A), self.device)
        partner = query_output("out[partner]", partner, torch.int32, (B, A), self.device)
        kind = query_output("out[kind]", kind, torch.uint8, (B, A), self.device)
        count = query_output("out[count]", count, torch.int32, (B, A), self.device)
        _lib.check(self._lib.pgx_path_conflicts(
            self._handle, paths.data_ptr(), _lib.CONFLICT_PATHS_PLAN if plan else _lib.CONFLICT_PATHS_CELLS, K, flags,
            first_step.data_ptr(), partner.data_ptr(), kind.data_ptr(), count.data_ptr(), self._stream()))
        return first_step, partner, kind, count

    def move_outcomes(self, actions, out=None):
        """Move outcomes (docs/SPEC.md S17): what the move phase of step(actions) would do to every agent and why a move
        that fails does, under this env's collision system and `soft_vertex` rule -- computed on the device from the
        current state, the state the next step() reads, which this call leaves untouched.  Returns
            (next_xy int32 [batch, agents, 2]: the cell the agent stands on after the moves, unpadded (row, col), before
                 goals, hiding, new lifelong targets and auto-reset; an inactive agent's own cell;
             outcome uint8 [batch, agents]: an index into pogema_amd.OUTCOMES -- STAY (inactive, noop, out-of-range
                 action), MOVED, OBSTACLE, SWAP, OCCUPIED (the agent on the destination stays), FOLLOW (it leaves, but
                 the collision system forbids following: never under "soft"), CONTESTED (another mover claims the cell);
             blocker int32 [batch, agents]: the agent standing on the destination for SWAP / OCCUPIED / FOLLOW, the
                 lowest-index other claimant for CONTESTED, else -1;
             counts int32 [batch, NUM_OUTCOMES]: the env's active agents per code).
        `actions`: as step() takes them; a value outside 0..4 counts as 0 whatever Semantics.bad_action says, and the
        call neither raises for it nor counts it.  One kernel launch: allocates nothing on the engine side,
        stream-ordered, no host sync, capturable in a HIP graph from the first call.
        `out=(next_xy, outcome, blocker, counts)`: caller-owned contiguous tensors of those dtypes and shapes on this
        device."""
        B, A = self.batch, self.num_agents
        actions = self._prepare_actions(actions)
        next_xy, outcome, blocker, counts = _split(out, ("next_xy", "outcome", "blocker", "counts"))
        next_xy = query_output("out[next_xy]", next_xy, torch.int32, (B, A, 2), self.device)
        outcome = query_output("out[outcome]", outcome, torch.uint8, (B, A), self.device)
        blocker = query_output("out[blocker]", blocker, torch.int32, (B, A), self.device)
        counts = query_output("out[counts]", counts, torch.int32, (B, _lib.NUM_OUTCOMES), self.device)
        _lib.check(self._lib.pgx_move_outcomes(self._handle, actions.data_ptr(), self._ACTION_CODE[actions.dtype], 0,
                                               next_xy.data_ptr(), outcome.data_ptr(), blocker.data_ptr(),
                                               counts.data_ptr(), self._stream()))
        return next_xy, outcome, blocker, counts

    def policy_input(self, channels=_lib.DEFAULT_POLICY_CHANNELS, dtype=torch.float32, out=None) -> torch.Tensor:
        """The network's input tensor (docs/SPEC.md S18): [batch, agents, C, W, W] of 0 / 1 in `dtype`, plane c the
        channel channels[c], written once in one launch -- computed on the device from the current state, the state
        the next step() reads, which this call leaves untouched.
        `channels`: a tuple or list of 1..8 distinct names, in the order the network wants them:
            "obstacles", "agents", "target"  -- planes 0, 1, 2 of observe(), bit for bit;
            "other_goals"  -- 1 where an agent visible_agents() calls visible has its target, clamped per axis to the
                window's edge as "target" is; every visible agent counts, however many; all zero for an inactive agent;
            "up", "down", "left", "right"  -- planes 0..3 of goal_directions(), bit for bit.
        The default is ("obstacles", "agents", "target", "up", "down", "left", "right"), what
        torch.cat((observe(), goal_directions()), 2) builds on a float32 engine.  PRIMAL reads the first four names,
        SCRIMP all eight.
        `dtype`: torch.float32, float16, bfloat16 or uint8, chosen per call whatever `obs_dtype` the engine has.
        Without a direction channel: one launch that reads no distance field and allocates nothing, stream-ordered, no
        host sync, capturable in a HIP graph from the first call.  With one it shares cost_to_go()'s cache under
        goal_directions()' rules (stale fields are rebuilt first; whichever call is first allocates the cache, not inside
        a graph capture).  `out`: a caller-owned contiguous tensor of that shape and dtype on this device."""
        codes = parse_channels(channels)
        if dtype not in _lib.OBS_DTYPES:
            raise ValueError(f"dtype must be one of torch.float32, torch.float16, torch.bfloat16, torch.uint8, got {dtype!r}")
        shape = (self.batch, self.num_agents, len(codes), self.window, self.window)
        out = query_output("out", out, dtype, shape, self.device)
        _lib.check(self._lib.pgx_policy_input(self._handle, (_lib.C.c_int32 * len(codes))(*codes), len(codes),
                                              _lib.OBS_DTYPES[dtype], out.data_ptr(), self._stream()))
        return out

    def global_state(self, channels=_lib.DEFAULT_GLOBAL_CHANNELS, dtype=torch.float32, out=None) -> torch.Tensor:
        """The global state (docs/SPEC.md S20): [batch, C, H, W] in `dtype`, the whole unpadded map of every env, row x,
        column y (the orientation of the maps reset() installs, the coordinates of get_state()), plane c the channel
        channels[c], written once in one launch -- computed on the device from the current state, the state the next
        step() reads, which this call leaves untouched.  What a centralised critic, a QMIX-style mixer or a central
        planner reads.
        `channels`: a tuple or list of 1..5 distinct names, in the order the network wants them:
            "obstacles"  -- the env's map as it is now (after regeneration, a pool draw or copy_envs()), 0 / 1;
            "agents"     -- the interior of get_state(occupancy=True)["occupancy"], bit for bit: 1 where an agent stands
                that is neither hidden nor a `soft` ghost, as in observation plane 1;
            "targets"    -- 1 on the target cell of every agent whose is_active is set (a ghost's counts, a finished,
                hidden agent's does not);
            "agent_ids"  -- i + 1 for the lowest agent i "agents" counts on the cell, else 0;
            "target_ids" -- j + 1 for the lowest agent j "targets" counts whose target is the cell, else 0 (lifelong
                targets may coincide).
        `dtype`: torch.float32, float16, bfloat16 or uint8, chosen per call whatever `obs_dtype` the engine has.  With an
        id channel it must hold num_agents exactly: uint8 up to 255 agents, bfloat16 up to 256 (ValueError otherwise).
        One launch that reads no distance field and allocates nothing on the engine side, stream-ordered, no host sync,
        capturable in a HIP graph from the first call after reset().  `out`: a caller-owned contiguous tensor of that
        shape and dtype on this device; a 16-byte aligned one is written fastest."""
        codes = parse_global_channels(channels)
        if dtype not in _lib.OBS_DTYPES:
            raise ValueError(f"dtype must be one of torch.float32, torch.float16, torch.bfloat16, torch.uint8, got {dtype!r}")
        check_global_ids(codes, dtype, self.num_agents)
        shape = (self.batch, len(codes), self.height, self.width)
        out = query_output("out", out, dtype, shape, self.device)
        _lib.check(self._lib.pgx_global_state(self._handle, (_lib.C.c_int32 * len(codes))(*codes), len(codes),
                                              _lib.OBS_DTYPES[dtype], out.data_ptr(), self._stream()))
        return out

    def _token_history(self, history):
        """agent_tokens()' `history` argument as a contiguous int8 tensor [batch, agents, 5] on this device, or None."""
        if history is None:
            return None
        shape = (self.batch, self.num_agents, _lib.TOKEN_HISTORY)
        if not isinstance(history, torch.Tensor):
            raise TypeError(f"history must be a torch.Tensor or None, got {type(history).__name__}")
        if history.dtype != torch.int8:
            raise TypeError(f"history must be an int8 tensor, got {history.dtype}")
        if tuple(history.shape) != shape or history.device != self.device:
            raise ValueError(f"history must have shape {shape} on {self.device}")
        return history.contiguous()

    def agent_tokens(self, slots: int = 13, history=None, length=None, out=None) -> torch.Tensor:
        """Token observations (docs/SPEC.md S21), the input of MAPF-GPT-style policies: uint8 [batch, agents, length],
        one row of token ids (pogema_amd.TOKENS) per agent, written once in one launch -- computed on the device from
        the current state, the state the next step() reads, which this call leaves untouched.  With W = 2 * obs_radius
        + 1 and L0 = W * W + 10 * slots (pogema_amd.token_length), the row of an active agent i is
            entries 0 .. W*W-1: its cost_to_go() window relative to its own cost, row-major: BLOCKED where cost_to_go()
                gives -1 there or at the centre, else clamp(cost - own, -20, 20) + 20;
            ten entries per slot: slot 0 the agent itself, slot s >= 1 entry s - 1 of visible_agents(k=slots - 1) --
                dx + 20, dy + 20; the listed agent's target minus i's position, clamped to -20..20, + 20 per axis; the
                listed agent's five `history` values (43 + v for an action v in 0..4, ACTION_NONE for anything else);
                48 + its greedy-move mask, goal_directions("bits") at its own window centre.  Ten PAD where the list
                has no entry;
            entries L0 .. length-1: PAD.
        An inactive agent's row is all PAD.  obs_radius=5, slots=13, length=256 is MAPF-GPT's 121 + 130 + 5 context.
        `slots`: 1..32, the agent included.  `length`: L0..2048, None = L0.  `history`: an int8 tensor [batch, agents, 5]
        on this device, most recent action first (TokenHistory keeps one; made contiguous if it is not), None = nothing
        recorded.
        Shares cost_to_go()'s cache under goal_directions()' rules: stale fields are rebuilt first, whichever call is
        first allocates the cache (not inside a graph capture); later calls are stream-ordered, need no host sync and can
        be captured.  `out`: a caller-owned contiguous uint8 tensor of that shape on this device, at any alignment."""
        if isinstance(slots, bool) or not isinstance(slots, (int, np.integer)) or not 1 <= slots <= _lib.MAX_TOKEN_SLOTS:
            raise ValueError(f"slots must be an integer in 1..{_lib.MAX_TOKEN_SLOTS}, got {slots!r}")
        slots = int(slots)
        l0 = self.window * self.window + _lib.TOKEN_SLOT_LEN * slots
        if length is None:
            length = l0
        if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or not l0 <= length <= _lib.MAX_TOKEN_LENGTH:
            raise ValueError(f"length must be an integer in {l0}..{_lib.MAX_TOKEN_LENGTH} (L0 = {l0} for this window and "
                             f"{slots} slots), got {length!r}")
        length = int(length)
        history = self._token_history(history)
        out = query_output("out", out, torch.uint8, (self.batch, self.num_agents, length), self.device)
        _lib.check(self._lib.pgx_agent_tokens(self._handle, slots, length, 0,
                                              history.data_ptr() if history is not None else None, out.data_ptr(),
                                              self._stream()))
        return out
