"""CPU reference of the move outcomes (docs/SPEC.md S17; VecPogema.move_outcomes / pgx_move_outcomes): S2's literal
move loops, restated here on plain Python data (tests/test_move_outcomes.py proves them equal to
PogemaOracle.move_agents), then S17's table applied to the cells they leave the agents on.  Pure numpy / Python."""
from __future__ import annotations

import numpy as np

MOVES = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))
STAY, MOVED, OBSTACLE, SWAP, OCCUPIED, FOLLOW, CONTESTED = range(7)
NUM_OUTCOMES = 7


def _clean(actions):
    """An action outside 0..4 counts as 0."""
    return [int(a) if 0 <= int(a) <= 4 else 0 for a in actions]


def move_phase(obst, cur, active, actions, collision, soft_vertex="lowest_index"):
    """S2's move phase of one env, literally.  obst: [H, W], nonzero = obstacle, everything outside it is one (the ring
    around the map); cur: A cells (x, y), unpadded; active: A flags; actions: A integers.  Returns the A cells after the
    moves."""
    H, W = np.asarray(obst).shape
    n = len(cur)
    cur = [(int(x), int(y)) for x, y in cur]
    active = [bool(a) for a in active]
    actions = _clean(actions)

    def obstacle(c):
        return not (0 <= c[0] < H and 0 <= c[1] < W) or obst[c[0]][c[1]] != 0

    def dest(i, acts):
        return (cur[i][0] + MOVES[acts[i]][0], cur[i][1] + MOVES[acts[i]][1])

    xy = list(cur)
    occupied = {c for i, c in enumerate(cur) if active[i]}          # the occupancy array: visible agents' cells

    def move(i, a):                                                 # Grid.move
        d = (xy[i][0] + MOVES[a][0], xy[i][1] + MOVES[a][1])
        if not obstacle(d) and d not in occupied:
            occupied.discard(xy[i])
            occupied.add(d)
            xy[i] = d

    if collision == "priority":
        for i in range(n):
            if active[i]:
                move(i, actions[i])
        return xy
    if collision == "block_both":
        used = {}
        for i in range(n):
            if active[i]:
                d = dest(i, actions)
                used[d] = "blocked" if d in used else "visited"
                used[cur[i]] = "blocked"
        for i in range(n):
            if active[i] and used.get(dest(i, actions)) != "blocked":
                move(i, actions[i])
        return xy
    assert collision == "soft", collision
    acts = list(actions)
    if soft_vertex == "all_stay":
        standing = {cur[i]: i for i in range(n) if active[i]}
        changed = True
        while changed:
            changed = False
            claims = {}
            for i in range(n):
                if active[i]:
                    claims.setdefault(dest(i, acts), []).append(i)
            revert = []
            for i in range(n):
                if active[i] and acts[i] != 0:
                    d = dest(i, acts)
                    o = standing.get(d)
                    swap = o is not None and acts[o] != 0 and dest(o, acts) == cur[i]
                    if obstacle(d) or len(claims[d]) > 1 or swap:
                        revert.append(i)
            for i in revert:
                acts[i] = 0
                changed = True
    else:
        assert soft_vertex == "lowest_index", soft_vertex
        cells, edges = {}, {}
        for i in range(n):
            if active[i]:
                d = dest(i, acts)
                cells.setdefault(d, []).append(i)
                edges[cur[i] + d] = [i]
                if acts[i] != 0:
                    edges.setdefault(d + cur[i], []).append(i)
        for i in range(n):
            if active[i]:
                d = dest(i, acts)
                if len(edges[cur[i] + d]) > 1:
                    cells[d].remove(i)
                    cells.setdefault(cur[i], []).append(i)
                    acts[i] = 0

        def revert_action(i, cell):                                 # the literal recursion, as a loop
            for _ in range(4 * n + 4):
                acts[i] = 0
                cells[cell].remove(i)
                own = cur[i]
                if own in cells and len(cells[own]) > 0:
                    cells[own].append(i)
                    i, cell = cells[own][0], own
                    continue
                cells.setdefault(own, []).append(i)
                return
            raise RecursionError("the literal `soft` algorithm does not end on this state")

        for i in reversed(range(n)):
            if active[i]:
                d = dest(i, acts)
                if len(cells[d]) > 1 or obstacle(d):
                    revert_action(i, d)
    return [dest(i, acts) if active[i] else cur[i] for i in range(n)]   # the moves that survive, without checks


def classify(obst, cur, active, actions, nxt):
    """S17's table for one env, given the cells `nxt` the move phase leaves the agents on.  Returns (outcome, blocker)."""
    H, W = np.asarray(obst).shape
    n = len(cur)
    cur = [(int(x), int(y)) for x, y in cur]
    nxt = [(int(x), int(y)) for x, y in nxt]
    actions = _clean(actions)
    mover = [bool(active[i]) and actions[i] != 0 for i in range(n)]
    d = [(cur[i][0] + MOVES[actions[i]][0], cur[i][1] + MOVES[actions[i]][1]) for i in range(n)]
    now = {}
    for i in range(n):
        if active[i]:
            now.setdefault(cur[i], i)                               # the lowest index standing on the cell
    claimants = {}
    for j in range(n):
        if mover[j]:
            claimants.setdefault(d[j], []).append(j)                # the movers that claim the cell, in index order
    outcome, blocker = [STAY] * n, [-1] * n
    for i in range(n):
        if not mover[i]:
            continue
        o = now.get(d[i])
        others = [j for j in claimants[d[i]] if j != i]
        if nxt[i] == d[i]:
            outcome[i] = MOVED
        elif not (0 <= d[i][0] < H and 0 <= d[i][1] < W) or obst[d[i][0]][d[i][1]] != 0:
            outcome[i] = OBSTACLE
        elif o is not None and o != i and mover[o] and d[o] == cur[i]:
            outcome[i], blocker[i] = SWAP, o
        elif o is not None and o != i and nxt[o] == d[i]:
            outcome[i], blocker[i] = OCCUPIED, o
        elif o is not None and o != i and not others:
            outcome[i], blocker[i] = FOLLOW, o
        else:
            outcome[i], blocker[i] = CONTESTED, (others[0] if others else -1)
    return outcome, blocker


def move_outcomes_one(obst, cur, active, actions, collision, soft_vertex="lowest_index"):
    """(next_xy [A, 2], outcome [A], blocker [A], counts [7]) of one env."""
    nxt = move_phase(obst, cur, active, actions, collision, soft_vertex)
    outcome, blocker = classify(obst, cur, active, actions, nxt)
    counts = [0] * NUM_OUTCOMES
    for i, c in enumerate(outcome):
        if active[i]:
            counts[c] += 1
    return nxt, outcome, blocker, counts


def move_outcomes_reference(maps, pos, active, actions, collision, soft_vertex="lowest_index"):
    """The four outputs of VecPogema.move_outcomes: maps [B, H, W], pos [B, A, 2] unpadded, active [B, A], actions
    [B, A] -> (next_xy int32 [B, A, 2], outcome uint8 [B, A], blocker int32 [B, A], counts int32 [B, 7])."""
    B, A = np.asarray(active).shape
    next_xy = np.zeros((B, A, 2), dtype=np.int32)
    outcome = np.zeros((B, A), dtype=np.uint8)
    blocker = np.zeros((B, A), dtype=np.int32)
    counts = np.zeros((B, NUM_OUTCOMES), dtype=np.int32)
    for b in range(B):
        n, o, k, c = move_outcomes_one(np.asarray(maps[b]).tolist(), pos[b], active[b], actions[b], collision, soft_vertex)
        next_xy[b], outcome[b], blocker[b], counts[b] = np.asarray(n, dtype=np.int32).reshape(A, 2), o, k, c
    return next_xy, outcome, blocker, counts
