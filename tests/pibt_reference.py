"""CPU reference of the cooperative planner (docs/SPEC.md S13): a literal, recursive transcription of the specification's
pseudo-code, on the state `VecPogema.get_state()` and the installed maps describe.  Test infrastructure only; the
package never imports it."""
from __future__ import annotations

import sys

import numpy as np

from expert_reference import MOVES, bfs_from

INF = float("inf")


def pibt_env(obstacles, agents_xy, targets_xy, is_active, priority=None):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A], priority [A] or None ->
    (actions int64 [A], next_xy int32 [A, 2])."""
    obstacles = np.asarray(obstacles) != 0
    H, W = obstacles.shape
    pos = [tuple(int(v) for v in p) for p in np.asarray(agents_xy)]
    tgt = [tuple(int(v) for v in p) for p in np.asarray(targets_xy)]
    A = len(pos)
    planned = [bool(v) for v in np.asarray(is_active)]   # get_state()'s is_active is bit 0 of the flag
    prio = [0] * A if priority is None else [int(v) for v in np.asarray(priority)]

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
                out.append((D(i, v), 1 if (v in now and now[v] != i) else 0, a, v))
        out.sort(key=lambda e: e[:3])
        return [(a, v) for _, _, a, v in out]

    res = {}
    nxt = [None] * A
    action = [0] * A

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
        return False

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * A + 200))
    try:
        for i in sorted((i for i in range(A) if planned[i]), key=lambda i: (-prio[i], i)):
            if nxt[i] is None:
                pibt(i, None)
    finally:
        sys.setrecursionlimit(limit)
    for i in range(A):
        if not planned[i]:
            nxt[i], action[i] = pos[i], 0
    return np.array(action, dtype=np.int64), np.array(nxt, dtype=np.int32).reshape(A, 2)


def pibt_reference(obstacles, agents_xy, targets_xy, is_active, priority=None):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A], priority [B, A] or None ->
    (actions int64 [B, A], next_xy int32 [B, A, 2])."""
    obstacles, agents_xy, targets_xy, is_active = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy, is_active))
    B, A = agents_xy.shape[:2]
    actions = np.zeros((B, A), dtype=np.int64)
    next_xy = np.zeros((B, A, 2), dtype=np.int32)
    for b in range(B):
        actions[b], next_xy[b] = pibt_env(obstacles[b], agents_xy[b], targets_xy[b], is_active[b],
                                          None if priority is None else np.asarray(priority)[b])
    return actions, next_xy


def check_invariants(obstacles, agents_xy, is_active, next_xy):
    """The guarantees of S13 for one environment; returns a list of violations (empty: all hold)."""
    obstacles = np.asarray(obstacles) != 0
    H, W = obstacles.shape
    pos = [tuple(int(v) for v in p) for p in np.asarray(agents_xy)]
    nxt = [tuple(int(v) for v in p) for p in np.asarray(next_xy)]
    ids = [i for i, a in enumerate(np.asarray(is_active)) if a]
    bad = []
    seen = {}
    for i in ids:
        x, y = nxt[i]
        if not (0 <= x < H and 0 <= y < W) or obstacles[x, y]:
            bad.append(("cell", i, nxt[i]))
        if abs(x - pos[i][0]) + abs(y - pos[i][1]) > 1:
            bad.append(("far", i, nxt[i]))
        if nxt[i] in seen:
            bad.append(("vertex", seen[nxt[i]], i, nxt[i]))
        seen[nxt[i]] = i
    for i in ids:
        for j in ids:
            if i < j and pos[i] != pos[j] and nxt[i] == pos[j] and nxt[j] == pos[i]:
                bad.append(("swap", i, j))
    return bad
