"""CPU reference of the cooperative planner with the swap operation (docs/SPEC.md S23): a literal, recursive
transcription of the specification's pseudo-code, on the state `VecPogema.get_state()` and the installed maps describe,
in the structure of tests/pibt_reference.py.  Every call also reports what the swap rule did: lists reversed (in all,
for a `usual` and for a `clear` partner), agents pulled, and the longest corridor walk.  Test infrastructure only; the
package never imports it."""
from __future__ import annotations

import sys

import numpy as np

import pibt_reference as _plain     # (its bfs_from is looked up per call: agent_counts.shared_fields swaps in a memo)
from expert_reference import MOVES

INF = float("inf")
MAX_WALK = 2048                      # PGX_SWAP_MAX_WALK
COUNTERS = ("reversed", "usual", "clear", "pulled", "longest_walk")


def pibt_swap_env(obstacles, agents_xy, targets_xy, is_active, priority=None, max_walk=MAX_WALK):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A], priority [A] or None ->
    (actions int64 [A], next_xy int32 [A, 2], counters: a dict with the keys of COUNTERS)."""
    obstacles = np.asarray(obstacles) != 0
    H, W = obstacles.shape
    pos = [tuple(int(v) for v in p) for p in np.asarray(agents_xy)]
    tgt = [tuple(int(v) for v in p) for p in np.asarray(targets_xy)]
    A = len(pos)
    planned = [bool(v) for v in np.asarray(is_active)]
    prio = [0] * A if priority is None else [int(v) for v in np.asarray(priority)]
    count = dict.fromkeys(COUNTERS, 0)

    fields = {}

    def D(i, c):
        if tgt[i] not in fields:
            fields[tgt[i]] = _plain.bfs_from(obstacles, *tgt[i])
        d = int(fields[tgt[i]][c])
        return INF if d < 0 else d

    now = {}
    for i in range(A):
        if planned[i]:
            now.setdefault(pos[i], i)

    def cands(i):
        out = []
        for a in range(5):
            v = (pos[i][0] + MOVES[a][0], pos[i][1] + MOVES[a][1])
            if 0 <= v[0] < H and 0 <= v[1] < W and not obstacles[v]:
                out.append((D(i, v), 1 if (v in now and now[v] != i) else 0, a, v))
        out.sort(key=lambda e: e[:3])
        return [(a, v) for _, _, a, v in out]

    def neigh(v):
        out = []
        for dx, dy in MOVES[1:]:
            u = (v[0] + dx, v[1] + dy)
            if 0 <= u[0] < H and 0 <= u[1] < W and not obstacles[u]:
                out.append(u)
        return out

    def parked(u):
        return u in now and tgt[now[u]] == u and len(neigh(u)) == 1

    def ahead(v_pusher, v_puller):
        n, tmp = 0, None
        for u in neigh(v_puller):
            if u != v_pusher and not parked(u):
                n += 1
                tmp = u
        return n, tmp

    def walked(it):
        count["longest_walk"] = max(count["longest_walk"], it)

    def swap_required(pusher, puller, v_pusher, v_puller):
        for it in range(max_walk + 1):
            walked(it)
            if not D(pusher, v_puller) < D(pusher, v_pusher):
                break
            if it == max_walk:
                return False
            n, tmp = ahead(v_pusher, v_puller)
            if n >= 2:
                return False
            if n == 0:
                break
            v_pusher, v_puller = v_puller, tmp
        return D(puller, v_pusher) < D(puller, v_puller) and (
            D(pusher, v_pusher) == 0 or D(pusher, v_puller) < D(pusher, v_pusher))

    def swap_possible(v_pusher0, v_puller0):
        v_pusher, v_puller = v_pusher0, v_puller0
        for it in range(max_walk + 1):
            walked(it)
            if v_puller == v_pusher0:
                return False
            if it == max_walk:
                return False
            n, tmp = ahead(v_pusher, v_puller)
            if n >= 2:
                return True
            if n == 0:
                return False
            v_pusher, v_puller = v_puller, tmp
        return False

    def partners(i):
        best = cands(i)[0][1]
        if best == pos[i]:
            return None, None
        usual = clear = None
        j = now.get(best)
        if j is not None and j != i and swap_required(i, j, pos[i], best) and swap_possible(best, pos[i]):
            usual = j
        for u in neigh(pos[i]):
            k = now.get(u)
            if (k is not None and k != i and u != best and swap_required(k, i, pos[i], best)
                    and swap_possible(best, pos[i])):
                clear = k
                break
        return usual, clear

    res = {}
    nxt = [None] * A
    action = [0] * A

    def move(a, b):
        return MOVES.index((b[0] - a[0], b[1] - a[1]))

    def pibt(i, parent):
        C = cands(i)
        usual, clear = partners(i)
        sw = usual if usual is not None and nxt[usual] is None else clear
        if sw is not None:
            C = C[::-1]
            count["reversed"] += 1
            count["usual" if sw == usual else "clear"] += 1
        for k, (a, v) in enumerate(C):
            if v in res:
                continue
            if parent is not None and v == pos[parent]:
                continue
            nxt[i], action[i], res[v] = v, a, i
            j = now.get(v)
            if j is not None and j != i and nxt[j] is None:
                if not pibt(j, i):
                    continue
            if k == 0 and sw is not None and nxt[sw] is None and pos[i] not in res:
                nxt[sw], action[sw], res[pos[i]] = pos[i], move(pos[sw], pos[i]), sw
                count["pulled"] += 1
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
    return np.array(action, dtype=np.int64), np.array(nxt, dtype=np.int32).reshape(A, 2), count


def pibt_swap_reference(obstacles, agents_xy, targets_xy, is_active, priority=None, max_walk=MAX_WALK):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A], priority [B, A] or None ->
    (actions int64 [B, A], next_xy int32 [B, A, 2], counters: a dict of int64 arrays [B] with the keys of COUNTERS)."""
    obstacles, agents_xy, targets_xy, is_active = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy, is_active))
    B, A = agents_xy.shape[:2]
    actions = np.zeros((B, A), dtype=np.int64)
    next_xy = np.zeros((B, A, 2), dtype=np.int32)
    counters = {name: np.zeros(B, dtype=np.int64) for name in COUNTERS}
    for b in range(B):
        actions[b], next_xy[b], count = pibt_swap_env(obstacles[b], agents_xy[b], targets_xy[b], is_active[b],
                                                       None if priority is None else np.asarray(priority)[b], max_walk)
        for name in COUNTERS:
            counters[name][b] = count[name]
    return actions, next_xy, counters
