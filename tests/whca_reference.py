"""CPU reference of windowed cooperative A* against a reservation table (docs/SPEC.md S28): the specification's
pseudo-code, literally -- a set of reserved (step, cell) pairs, a set of reserved (step, from, to) moves, the layers R_h
as Python sets, one BFS distance field per agent (pibt_plan_reference's memo of expert_reference.bfs_from), on the state
`VecPogema.get_state()` and the installed maps describe.  Test infrastructure only; the package never imports it."""
from __future__ import annotations

import numpy as np

from expert_reference import MOVES
from pibt_plan_reference import _bfs_memo, _prefill, _wrap_i32

MAX_HORIZON = 31


def whca_env(obstacles, agents_xy, targets_xy, is_active, horizon, priority=None, on_target="finish"):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A], priority [A] or None ->
    (actions int64 [K, A], path_xy int32 [K, A, 2], arrival int32 [A], failed int32 [A], last int32 [A]);
    last[i] is the last step agent i reserves (-1 for an agent that is not planned)."""
    blocked = np.asarray(obstacles) != 0
    H, W = blocked.shape
    pos = [tuple(int(v) for v in p) for p in np.asarray(agents_xy)]
    tgt = [tuple(int(v) for v in p) for p in np.asarray(targets_xy)]
    planned = [bool(a) for a in np.asarray(is_active)]
    A, K = len(pos), int(horizon)
    assert 1 <= K <= MAX_HORIZON
    prio = [0] * A if priority is None else [_wrap_i32(v) for v in np.asarray(priority)]

    cells = [[pos[i]] * (K + 1) for i in range(A)]
    actions = np.zeros((K, A), dtype=np.int64)
    failed = np.zeros(A, dtype=np.int32)
    last = np.full(A, -1, dtype=np.int32)
    vertex = set()        # (h, cell): a served agent occupies `cell` at step h
    edge = set()          # (h, from, to): a served agent moves from -> to in step h

    def free(h, c):
        return 0 <= c[0] < H and 0 <= c[1] < W and not blocked[c] and (h, c) not in vertex

    def move_ok(h, u, c):     # i goes u -> c in step h: nobody goes c -> u in it
        return (h, c, u) not in edge

    _prefill(blocked, [tgt[i] for i in range(A) if planned[i]])
    for i in sorted((i for i in range(A) if planned[i]), key=lambda i: (-prio[i], i)):
        R = [{pos[i]}]
        end = None
        for h in range(1, K + 1):
            layer = set()
            for u in R[h - 1]:
                for a, (dx, dy) in enumerate(MOVES):
                    c = (u[0] + dx, u[1] + dy)
                    if free(h, c) and (a == 0 or move_ok(h, u, c)):
                        layer.add(c)
            R.append(layer)
            if not layer:
                break
            if on_target == "finish" and tgt[i] in layer:
                end = (tgt[i], h)
                break
        if not R[-1]:
            failed[i] = 1
            path, h_end = [pos[i]] * (K + 1), K
        else:
            if end is None:
                D = _bfs_memo(blocked, *tgt[i])
                if D[pos[i]] < 0:
                    key = lambda c: (abs(c[0] - pos[i][0]) + abs(c[1] - pos[i][1]), c[0] * W + c[1])
                else:
                    assert all(D[c] >= 0 for c in R[K])
                    key = lambda c: (int(D[c]), c[0] * W + c[1])
                end = (min(R[K], key=key), K)
            cur, h_end = end
            path = [cur] * (K + 1)
            for h in range(h_end, 0, -1):
                for a, (dx, dy) in enumerate(MOVES):
                    u = (cur[0] - dx, cur[1] - dy)
                    if u in R[h - 1] and (a == 0 or move_ok(h, u, cur)):
                        break
                else:
                    raise AssertionError("the backtrack found no predecessor")
                actions[h - 1, i] = a
                path[h - 1] = u
                cur = u
            assert path[0] == pos[i]
        cells[i] = path
        last[i] = h_end
        for h in range(h_end + 1):
            vertex.add((h, path[h]))
            if h >= 1 and path[h - 1] != path[h]:
                edge.add((h, path[h - 1], path[h]))

    path_xy = np.array([[cells[i][h + 1] for i in range(A)] for h in range(K)], dtype=np.int32).reshape(K, A, 2)
    arrival = np.full(A, -1, dtype=np.int32)
    for i in range(A):
        if planned[i]:
            arrival[i] = next((h for h in range(K + 1) if cells[i][h] == tgt[i]), -1)
    return actions, path_xy, arrival, failed, last


def whca_reference(obstacles, agents_xy, targets_xy, is_active, horizon, priority=None, on_target="finish"):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A], priority [B, A] or None ->
    (actions int64 [K, B, A], path_xy int32 [K, B, A, 2], arrival int32 [B, A], failed int32 [B, A], last int32 [B, A])."""
    obstacles, agents_xy, targets_xy, is_active = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy, is_active))
    outs = [whca_env(obstacles[b], agents_xy[b], targets_xy[b], is_active[b], horizon,
                     None if priority is None else np.asarray(priority)[b], on_target) for b in range(agents_xy.shape[0])]
    actions, path, arrival, failed, last = zip(*outs)
    return np.stack(actions, axis=1), np.stack(path, axis=1), np.stack(arrival), np.stack(failed), np.stack(last)


def conflicts(agents_xy, path_xy, last, failed):
    """The independent validator: all pairs of non-failed planned agents of one env, every step -> a list of
    (kind, h, i, j).  Agent i occupies its cell at step h iff h <= last[i] (the vanish rule of `finish`)."""
    K, A = path_xy.shape[:2]
    cell = lambda i, h: tuple(int(v) for v in (agents_xy[i] if h == 0 else path_xy[h - 1, i]))
    ids = [i for i in range(A) if last[i] >= 0 and not failed[i]]
    found = []
    for h in range(K + 1):
        for n, i in enumerate(ids):
            for j in ids[n + 1:]:
                if h > last[i] or h > last[j]:
                    continue
                if cell(i, h) == cell(j, h):
                    found.append(("vertex", h, i, j))
                if h >= 1 and cell(i, h) != cell(i, h - 1) and cell(i, h) == cell(j, h - 1) and cell(j, h) == cell(i, h - 1):
                    found.append(("edge", h, i, j))
    return found
