"""CPU reference of the multi-step planner with the swap operation (docs/SPEC.md S27): pibt_plan_reference.pibt_plan_env's
loop around the one-step reference with the swap rule (pibt_swap_reference.pibt_swap_env), with the same memoised
distance fields -- the targets do not move during the lookahead.  Every step is planned on the positions and the planned
flags of that step, so an agent that stopped being planned is in nobody's now().  Besides the five arrays of the plain
plan reference it returns what the swap rule did at every step (pibt_swap_reference.COUNTERS).  Test infrastructure
only; the package never imports it."""
from __future__ import annotations

import numpy as np

import pibt_reference
from pibt_plan_reference import _bfs_memo, _prefill, _wrap_i32
from pibt_swap_reference import COUNTERS, MAX_WALK, pibt_swap_env


def pibt_swap_plan_env(obstacles, agents_xy, targets_xy, is_active, horizon, priority=None, on_target="finish",
                       growing=True, max_walk=MAX_WALK):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A], priority [A] or None ->
    (actions int64 [K, A], path_xy int32 [K, A, 2], arrival int32 [A], priority int32 [A], planned bool [K + 1, A],
     counters: a dict of int64 arrays [K] with the keys of COUNTERS); planned[h] are the flags step h plans with,
    planned[K] those the lookahead ends with, counters[name][h] what step h did."""
    obstacles = np.asarray(obstacles) != 0
    pos = np.asarray(agents_xy).astype(np.int32).copy()
    tgt = np.asarray(targets_xy).astype(np.int32)
    A, K = len(pos), int(horizon)
    planned = np.asarray(is_active).astype(bool).copy()
    planned0 = planned.copy()
    prio = [0] * A if priority is None else [_wrap_i32(v) for v in np.asarray(priority)]
    actions = np.zeros((K, A), dtype=np.int64)
    path = np.zeros((K, A, 2), dtype=np.int32)
    flags = np.zeros((K + 1, A), dtype=bool)
    counters = {name: np.zeros(K, dtype=np.int64) for name in COUNTERS}
    arrival = np.where(planned0 & (pos == tgt).all(axis=1), 0, -1).astype(np.int32)
    _prefill(obstacles, tgt)                     # the walks ask for the fields of partners, parked() for nobody's
    saved = pibt_reference.bfs_from
    pibt_reference.bfs_from = _bfs_memo          # pibt_swap_env looks bfs_from up in pibt_reference at every call
    try:
        for h in range(K):
            flags[h] = planned
            actions[h], path[h], count = pibt_swap_env(obstacles, pos, tgt, planned, prio, max_walk)
            for name in COUNTERS:
                counters[name][h] = count[name]
            pos = path[h].copy()
            on = (pos == tgt).all(axis=1)
            arrival = np.where(planned0 & on & (arrival < 0), h + 1, arrival).astype(np.int32)
            if on_target == "finish":
                planned = planned & ~on
            if growing:
                prio = [0 if (not planned[i] or on[i]) else _wrap_i32(prio[i] + 1) for i in range(A)]
    finally:
        pibt_reference.bfs_from = saved
    flags[K] = planned
    return actions, path, arrival, np.array(prio, dtype=np.int32), flags, counters


def pibt_swap_plan_reference(obstacles, agents_xy, targets_xy, is_active, horizon, priority=None, on_target="finish",
                             growing=True, max_walk=MAX_WALK):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A], priority [B, A] or None ->
    (actions int64 [K, B, A], path_xy int32 [K, B, A, 2], arrival int32 [B, A], priority int32 [B, A],
     planned bool [K + 1, B, A], counters: a dict of int64 arrays [K, B] with the keys of COUNTERS)."""
    obstacles, agents_xy, targets_xy, is_active = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy, is_active))
    B = agents_xy.shape[0]
    outs = [pibt_swap_plan_env(obstacles[b], agents_xy[b], targets_xy[b], is_active[b], horizon,
                               None if priority is None else np.asarray(priority)[b], on_target, growing, max_walk)
            for b in range(B)]
    actions, path, arrival, prio, flags, counters = zip(*outs)
    return (np.stack(actions, axis=1), np.stack(path, axis=1), np.stack(arrival), np.stack(prio), np.stack(flags, axis=1),
            {name: np.stack([c[name] for c in counters], axis=1) for name in COUNTERS})


def late(counters, name):
    """What steps h >= 1 of a lookahead did, summed: step 0 is the one-step planner's ground."""
    return int(np.asarray(counters[name])[1:].sum())
