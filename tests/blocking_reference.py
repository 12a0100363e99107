"""CPU reference of the blocking counts (docs/SPEC.md S25), deliberately naive: per eligible ordered pair (i, j) two
plain queue searches from j's cell to j's target, one on the map and one on the map with i's cell made an obstacle.  No
filter, no cached field.  i blocks j iff the first search finds a path (d0 steps), the two stand on different cells and
the second finds none of at most d0 + inflation - 1 steps.  Test infrastructure only; the package never imports it."""
from __future__ import annotations

from collections import deque

import numpy as np

from expert_reference import MOVES, bfs_from

# what a pair is, for the suites that prove their inputs are not vacuous
NOT_ELIGIBLE, NO_PATH, SAME_CELL, FREE, DETOUR, CUT_OFF = "not eligible", "no path", "same cell", "free", "detour", "cut off"


def path_length(blocked, s, t):
    """Steps of a shortest path from cell s to cell t over the unblocked cells, -1 when there is none."""
    H, W = blocked.shape
    s, t = (int(s[0]), int(s[1])), (int(t[0]), int(t[1]))
    if blocked[s] or blocked[t]:
        return -1
    dist = {s: 0}
    q = deque([s])
    while q:
        cell = q.popleft()
        if cell == t:
            return dist[cell]
        for dx, dy in MOVES[1:]:
            n = (cell[0] + dx, cell[1] + dy)
            if 0 <= n[0] < H and 0 <= n[1] < W and not blocked[n] and n not in dist:
                dist[n] = dist[cell] + 1
                q.append(n)
    return -1


def eligible(agents_xy, targets_xy, is_active, r, i, j, blockers="all"):
    """One env: is the ordered pair (i, j) eligible?"""
    if i == j or not (is_active[i] and is_active[j]):
        return False
    if np.abs(np.asarray(agents_xy[j]) - np.asarray(agents_xy[i])).max() > r:
        return False
    return blockers == "all" or tuple(agents_xy[i]) == tuple(targets_xy[i])


def classify_pair(blocked, agents_xy, targets_xy, is_active, r, inflation, i, j, blockers="all"):
    """One env, `blocked` bool [H, W]: what the ordered pair (i, j) is -- DETOUR and CUT_OFF are the blocked ones."""
    if not eligible(agents_xy, targets_xy, is_active, r, i, j, blockers):
        return NOT_ELIGIBLE
    c, s, t = (tuple(int(v) for v in p) for p in (agents_xy[i], agents_xy[j], targets_xy[j]))
    d0 = path_length(blocked, s, t)
    if d0 < 0:
        return NO_PATH
    if s == c:
        return SAME_CELL
    without = blocked.copy()
    without[c] = True
    d1 = path_length(without, s, t)
    if d1 < 0:
        return CUT_OFF
    return DETOUR if d1 > d0 + inflation - 1 else FREE


def blocking_env(obstacles, agents_xy, targets_xy, is_active, r, inflation, blockers="all"):
    """One env -> (count [A], blocked_by [A], kinds {(i, j): what the eligible pair is})."""
    blocked = np.asarray(obstacles) != 0
    A = len(agents_xy)
    count, blocked_by, kinds = np.zeros(A, np.int32), np.zeros(A, np.int32), {}
    # the pairs in each other's windows, in one numpy expression (A^2 Python calls are the slow part at 1024 agents);
    # classify_pair states every condition again
    xy = np.asarray(agents_xy).astype(np.int64)
    near = (np.abs(xy[:, None] - xy[None]) <= r).all(-1)
    for i, j in np.argwhere(near).tolist():
        kind = classify_pair(blocked, agents_xy, targets_xy, is_active, r, inflation, i, j, blockers)
        if kind == NOT_ELIGIBLE:
            continue
        kinds[(i, j)] = kind
        if kind in (DETOUR, CUT_OFF):
            count[i] += 1
            blocked_by[j] += 1
    return count, blocked_by, kinds


def blocking_reference(obstacles, agents_xy, targets_xy, is_active, r, inflation=10, blockers="all", envs=None,
                       kinds=None):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A] -> (count int32 [B, A],
    blocked_by int32 [B, A]).  `envs`: only these environments (the other rows stay 0).  `kinds`: a dict that receives
    {(b, i, j): what the eligible pair is}."""
    assert blockers in ("all", "on_target")
    obstacles, agents_xy, targets_xy = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy))
    is_active = np.asarray(is_active).astype(bool)
    B, A = agents_xy.shape[:2]
    count, blocked_by = np.zeros((B, A), np.int32), np.zeros((B, A), np.int32)
    for b in (range(B) if envs is None else envs):
        count[b], blocked_by[b], k = blocking_env(obstacles[b], agents_xy[b], targets_xy[b], is_active[b], r, inflation,
                                                   blockers)
        if kinds is not None:
            kinds.update({(b, i, j): v for (i, j), v in k.items()})
    return count, blocked_by


def filter_dismisses(obstacles, c, s, t, field=None):
    """The exact shortcut of S25 on j's distance field F (to t): True iff F[c] is undefined or F[c] + |c - s|_1 > F[s] --
    then c is on no shortest path from s to t and the pair is not blocked, without a search.  Asked only where F[s] is
    defined.  `field`: F, when the caller has it already."""
    F = bfs_from(np.asarray(obstacles) != 0, int(t[0]), int(t[1])) if field is None else field
    d0 = F[int(s[0]), int(s[1])]
    assert d0 >= 0
    fc = F[int(c[0]), int(c[1])]
    return bool(fc < 0 or fc + abs(int(c[0]) - int(s[0])) + abs(int(c[1]) - int(s[1])) > d0)


def searched_pairs(obstacles, agents_xy, targets_xy, kinds, envs=None):
    """Of the eligible pairs `kinds` holds ({(b, i, j): kind}): (those the filter dismisses, those left for a search) --
    pairs without a path for j or on one cell take neither."""
    dismissed, searched, fields = [], [], {}
    for (b, i, j), kind in kinds.items():
        if kind in (NO_PATH, SAME_CELL) or (envs is not None and b not in envs):
            continue
        t = (int(targets_xy[b][j][0]), int(targets_xy[b][j][1]))
        if (b, t) not in fields:                 # one field per distinct (env, target) of this call
            fields[(b, t)] = bfs_from(np.asarray(obstacles[b]) != 0, *t)
        out = filter_dismisses(obstacles[b], agents_xy[b][i], agents_xy[b][j], t, field=fields[(b, t)])
        (dismissed if out else searched).append((b, i, j))
    return dismissed, searched
