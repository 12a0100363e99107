"""CPU reference of the multi-step planner (docs/SPEC.md S16): the specification's loop around the one-step reference
(pibt_reference.pibt_env), on the state `VecPogema.get_state()` and the installed maps describe.  The targets do not move
during the lookahead, so the distance field of a (map, target) pair is computed once and shared by every step and every
agent that asks for it.  Test infrastructure only; the package never imports it."""
from __future__ import annotations

import numpy as np

import pibt_reference
from expert_reference import bfs_from

_fields = {}
_cells = [0]


def _bfs_memo(blocked, tx, ty):
    """bfs_from, memoised per (map, target); forgets everything once it holds 16 M cells (128 MB)."""
    blocked = np.ascontiguousarray(blocked)
    key = (blocked.shape, blocked.tobytes(), int(tx), int(ty))
    if key not in _fields:
        if _cells[0] > 1 << 24:
            _fields.clear()
            _cells[0] = 0
        _fields[key] = bfs_from(blocked, tx, ty)
        _cells[0] += blocked.size
    return _fields[key]


def _prefill(blocked, targets):
    """The fields of all `targets` on one map at once -- bfs_from's distances, every frontier advanced in one array
    operation -- so that a thousand agents do not cost a thousand Python searches."""
    blocked = np.ascontiguousarray(blocked)
    H, W = blocked.shape
    raw = blocked.tobytes()
    todo = sorted({(int(x), int(y)) for x, y in targets} - {k[2:] for k in _fields if k[:2] == (blocked.shape, raw)})
    todo = [(x, y) for x, y in todo if 0 <= x < H and 0 <= y < W]
    if not todo:
        return
    if _cells[0] > 1 << 24:
        _fields.clear()
        _cells[0] = 0
    dist = np.full((len(todo), H, W), -1, dtype=np.int64)
    front = np.zeros(dist.shape, dtype=bool)
    for k, (x, y) in enumerate(todo):
        front[k, x, y] = not blocked[x, y]
    dist[front] = 0
    free = ~blocked[None]
    d = 0
    while front.any():
        d += 1
        nb = np.zeros_like(front)
        nb[:, 1:] |= front[:, :-1]
        nb[:, :-1] |= front[:, 1:]
        nb[:, :, 1:] |= front[:, :, :-1]
        nb[:, :, :-1] |= front[:, :, 1:]
        nb &= free
        nb &= dist < 0
        dist[nb] = d
        front = nb
    for k, (x, y) in enumerate(todo):
        _fields[(blocked.shape, raw, x, y)] = dist[k].copy()
        _cells[0] += blocked.size


def _wrap_i32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def pibt_plan_env(obstacles, agents_xy, targets_xy, is_active, horizon, priority=None, on_target="finish", growing=True):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A], priority [A] or None ->
    (actions int64 [K, A], path_xy int32 [K, A, 2], arrival int32 [A], priority int32 [A], planned bool [K + 1, A]);
    planned[h] are the flags step h plans with, planned[K] those the lookahead ends with."""
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
    arrival = np.where(planned0 & (pos == tgt).all(axis=1), 0, -1).astype(np.int32)
    _prefill(obstacles, tgt[planned])
    saved = pibt_reference.bfs_from
    pibt_reference.bfs_from = _bfs_memo          # pibt_env asks for the field of every target in every step
    try:
        for h in range(K):
            flags[h] = planned
            actions[h], path[h] = pibt_reference.pibt_env(obstacles, pos, tgt, planned, prio)
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
    return actions, path, arrival, np.array(prio, dtype=np.int32), flags


def pibt_plan_reference(obstacles, agents_xy, targets_xy, is_active, horizon, priority=None, on_target="finish",
                        growing=True):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A], priority [B, A] or None ->
    (actions int64 [K, B, A], path_xy int32 [K, B, A, 2], arrival int32 [B, A], priority int32 [B, A],
     planned bool [K + 1, B, A])."""
    obstacles, agents_xy, targets_xy, is_active = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy, is_active))
    B = agents_xy.shape[0]
    outs = [pibt_plan_env(obstacles[b], agents_xy[b], targets_xy[b], is_active[b], horizon,
                          None if priority is None else np.asarray(priority)[b], on_target, growing) for b in range(B)]
    actions, path, arrival, prio, flags = zip(*outs)
    return (np.stack(actions, axis=1), np.stack(path, axis=1), np.stack(arrival), np.stack(prio), np.stack(flags, axis=1))
