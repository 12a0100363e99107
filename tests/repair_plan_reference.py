"""CPU reference of plan repair (docs/SPEC.md S29): the specification's pseudo-code, literally -- the walk scan of the
given paths, the kept agents entered into a set of reserved (step, cell) pairs and a set of reserved (step, from, to)
moves, then S28's service of the replanned agents with the layers R_h as Python sets and one BFS distance field per
agent (pibt_plan_reference's memo), on the state `VecPogema.get_state()` and the installed maps describe.  Test
infrastructure only; the package never imports it."""
from __future__ import annotations

import numpy as np

from expert_reference import MOVES
from pibt_plan_reference import _bfs_memo, _prefill, _wrap_i32
from whca_reference import MAX_HORIZON


def walk_scan(blocked, pos, tgt, given, on_target):
    """The scan of one planned agent's given path: `given` is a list of K (row, col) pairs of Python ints ->
    (is a walk, last step)."""
    H, W = blocked.shape
    K = len(given)
    prev = pos
    for h in range(1, K + 1):
        c = given[h - 1]
        if not (0 <= c[0] < H and 0 <= c[1] < W):      # the range check comes first
            return False, K
        if blocked[c] or (c[0] - prev[0], c[1] - prev[1]) not in MOVES:
            return False, K
        if on_target == "finish" and c == tgt:
            return True, h
        prev = c
    return True, K


def repair_env(obstacles, agents_xy, targets_xy, is_active, paths, replan=None, priority=None, on_target="finish"):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A], paths [K, A, 2] (any int32),
    replan [A] or None, priority [A] or None ->
    (actions int64 [K, A], path_xy int32 [K, A, 2], arrival int32 [A], failed int32 [A], replanned int32 [A],
     last int32 [A]); last[i] is the last step agent i reserves (-1 for an agent that is not planned)."""
    blocked = np.asarray(obstacles) != 0
    H, W = blocked.shape
    pos = [tuple(int(v) for v in p) for p in np.asarray(agents_xy)]
    tgt = [tuple(int(v) for v in p) for p in np.asarray(targets_xy)]
    planned = [bool(a) for a in np.asarray(is_active)]
    paths = np.asarray(paths)
    K, A = int(paths.shape[0]), len(pos)
    assert 1 <= K <= MAX_HORIZON and paths.shape == (K, A, 2)
    ask = [False] * A if replan is None else [bool(v) for v in np.asarray(replan)]
    prio = [0] * A if priority is None else [_wrap_i32(v) for v in np.asarray(priority)]

    cells = [[pos[i]] * (K + 1) for i in range(A)]
    actions = np.zeros((K, A), dtype=np.int64)
    failed = np.zeros(A, dtype=np.int32)
    replanned = np.zeros(A, dtype=np.int32)
    last = np.full(A, -1, dtype=np.int32)
    vertex = set()        # (h, cell): a kept or served agent occupies `cell` at step h
    edge = set()          # (h, from, to): a kept or served agent moves from -> to in step h

    def reserve(i):
        for h in range(last[i] + 1):
            vertex.add((h, cells[i][h]))
            if h >= 1 and cells[i][h - 1] != cells[i][h]:
                edge.add((h, cells[i][h - 1], cells[i][h]))

    # the kept agents: all of them are reserved before anyone is served
    for i in range(A):
        if not planned[i]:
            continue
        given = [tuple(int(v) for v in paths[h, i]) for h in range(K)]
        walk, last_i = walk_scan(blocked, pos[i], tgt[i], given, on_target)
        if ask[i] or not walk:
            replanned[i] = 1
            continue
        cells[i] = [pos[i]] + given[:last_i] + [given[last_i - 1]] * (K - last_i)
        last[i] = last_i
        for h in range(last_i):
            actions[h, i] = MOVES.index((cells[i][h + 1][0] - cells[i][h][0], cells[i][h + 1][1] - cells[i][h][1]))
        reserve(i)

    def free(h, c):
        return 0 <= c[0] < H and 0 <= c[1] < W and not blocked[c] and (h, c) not in vertex

    def move_ok(h, u, c):     # i goes u -> c in step h: nobody goes c -> u in it
        return (h, c, u) not in edge

    _prefill(blocked, [tgt[i] for i in range(A) if replanned[i]])
    for i in sorted((i for i in range(A) if replanned[i]), key=lambda i: (-prio[i], i)):     # S28's service
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
        reserve(i)

    path_xy = np.array([[cells[i][h + 1] for i in range(A)] for h in range(K)], dtype=np.int32).reshape(K, A, 2)
    arrival = np.full(A, -1, dtype=np.int32)
    for i in range(A):
        if planned[i]:
            arrival[i] = next((h for h in range(K + 1) if cells[i][h] == tgt[i]), -1)
    return actions, path_xy, arrival, failed, replanned, last


def repair_reference(obstacles, agents_xy, targets_xy, is_active, paths, replan=None, priority=None, on_target="finish"):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A], paths [K, B, A, 2], replan and
    priority [B, A] or None -> (actions int64 [K, B, A], path_xy int32 [K, B, A, 2], arrival, failed, replanned, last
    int32 [B, A])."""
    obstacles, agents_xy, targets_xy, is_active, paths = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy,
                                                                                   is_active, paths))
    outs = [repair_env(obstacles[b], agents_xy[b], targets_xy[b], is_active[b], paths[:, b],
                       None if replan is None else np.asarray(replan)[b],
                       None if priority is None else np.asarray(priority)[b], on_target) for b in range(agents_xy.shape[0])]
    actions, path, arrival, failed, replanned, last = zip(*outs)
    return (np.stack(actions, axis=1), np.stack(path, axis=1), np.stack(arrival), np.stack(failed), np.stack(replanned),
            np.stack(last))
