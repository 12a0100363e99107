"""CPU reference of collision shielding (docs/SPEC.md S15): a literal, recursive transcription of the specification's
pseudo-code -- S13's planner with the candidates ordered by the caller's scores -- on the state `VecPogema.get_state()`
and the installed maps describe.  Test infrastructure only; the package never imports it."""
from __future__ import annotations

import math
import sys

import numpy as np

from expert_reference import MOVES, bfs_from

INF = float("inf")


def _score_key(s):
    """(isnan(s), -s): ascending = the higher score first, -0.0 == +0.0, a NaN after -inf."""
    s = float(s)
    return (1, 0.0) if math.isnan(s) else (0, -s)


def shield_env(obstacles, agents_xy, targets_xy, is_active, scores, priority=None, tie_break=None):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A], scores [A, 5] (any float dtype,
    widened exactly to float32), priority [A] or None, tie_break None or "distance" ->
    (actions int64 [A], next_xy int32 [A, 2], overridden uint8 [A], number of PIBT calls that returned False)."""
    assert tie_break in (None, "distance")
    obstacles = np.asarray(obstacles) != 0
    H, W = obstacles.shape
    pos = [tuple(int(v) for v in p) for p in np.asarray(agents_xy)]
    tgt = [tuple(int(v) for v in p) for p in np.asarray(targets_xy)]
    A = len(pos)
    planned = [bool(v) for v in np.asarray(is_active)]   # get_state()'s is_active is bit 0 of the flag
    prio = [0] * A if priority is None else [int(v) for v in np.asarray(priority)]
    scores = np.asarray(scores).astype(np.float32)
    assert scores.shape == (A, 5)

    fields = {}

    def D(i, c):
        if tgt[i] not in fields:
            fields[tgt[i]] = bfs_from(obstacles, *tgt[i])
        d = int(fields[tgt[i]][c])
        return INF if d < 0 else d

    now = {}
    for i in range(A):
        if planned[i]:
            now.setdefault(pos[i], i)     # the lowest-index planned agent standing on the cell

    def cands(i):
        out = []
        for a in range(5):
            v = (pos[i][0] + MOVES[a][0], pos[i][1] + MOVES[a][1])
            if 0 <= v[0] < H and 0 <= v[1] < W and not obstacles[v]:
                key = _score_key(scores[i, a])
                if tie_break == "distance":
                    key = key + (D(i, v), 1 if (v in now and now[v] != i) else 0)
                out.append((key + (a,), a, v))
        out.sort(key=lambda e: e[0])
        return [(a, v) for _, a, v in out]

    res = {}
    nxt = [None] * A
    action = [0] * A
    failed = [0]

    def pibt(i, parent):
        for a, v in cands(i):
            if v in res:
                continue
            if parent is not None and v == pos[parent]:
                continue
            nxt[i], action[i], res[v] = v, a, i
            j = now.get(v)
            if j is not None and j != i and nxt[j] is None:
                if not pibt(j, i):
                    continue
            return True
        nxt[i], action[i], res[pos[i]] = pos[i], 0, i
        failed[0] += 1
        return False

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * A + 200))
    try:
        for i in sorted((i for i in range(A) if planned[i]), key=lambda i: (-prio[i], i)):
            if nxt[i] is None:
                pibt(i, None)
    finally:
        sys.setrecursionlimit(limit)
    overridden = np.zeros(A, dtype=np.uint8)
    for i in range(A):
        if not planned[i]:
            nxt[i], action[i] = pos[i], 0
        else:
            best = min(range(5), key=lambda a: _score_key(scores[i, a]) + (a,))
            overridden[i] = 1 if action[i] != best else 0
    return np.array(action, dtype=np.int64), np.array(nxt, dtype=np.int32).reshape(A, 2), overridden, failed[0]


def shield_reference(obstacles, agents_xy, targets_xy, is_active, scores, priority=None, tie_break=None):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A], scores [B, A, 5], priority
    [B, A] or None -> (actions int64 [B, A], next_xy int32 [B, A, 2], overridden uint8 [B, A], failed int64 [B])."""
    obstacles, agents_xy, targets_xy, is_active = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy, is_active))
    scores = np.asarray(scores)
    B, A = agents_xy.shape[:2]
    actions = np.zeros((B, A), dtype=np.int64)
    next_xy = np.zeros((B, A, 2), dtype=np.int32)
    overridden = np.zeros((B, A), dtype=np.uint8)
    failed = np.zeros(B, dtype=np.int64)
    for b in range(B):
        actions[b], next_xy[b], overridden[b], failed[b] = shield_env(
            obstacles[b], agents_xy[b], targets_xy[b], is_active[b], scores[b],
            None if priority is None else np.asarray(priority)[b], tie_break)
    return actions, next_xy, overridden, failed
