"""The hand-built instances of the planner with the swap operation (docs/SPEC.md S23) and the random suites, shared by
the CPU file (tests/test_pibt_swap.py) and the GPU file (tests/test_pibt_swap_gpu.py).  Nothing here needs a GPU.  Test
infrastructure only."""
from __future__ import annotations

import numpy as np

from expert_reference import bfs_from
from pibt_swap_reference import MAX_WALK


def grid(rows):
    """Map rows ('#' obstacle) -> uint8 [H, W]."""
    return np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)


# name -> (map rows, agents, targets)
DEAD_END_MAP = ("#######", "##.####", ".......", "#######")
DEAD_END = (DEAD_END_MAP, [(2, 3), (2, 5)], [(2, 6), (2, 0)])
DEAD_END_INSIDE = (DEAD_END_MAP, [(2, 5), (2, 6)], [(2, 6), (2, 0)])     # the state in which plain PIBT is stuck for good
CLEAR = (("#.###", "....."), [(1, 1), (1, 0)], [(1, 2), (1, 4)])
RING = (("....", ".##.", ".##.", "...."), [(0, 0), (0, 1), (3, 3)], [(0, 1), (0, 0), (0, 2)])

# (instance, priority) -> (actions, next cells, counters that are not 0) of the swap planner
PINNED = [
    ("dead end, first step", DEAD_END, None, [4, 0], [(2, 4), (2, 5)], {}),
    ("dead end, inside", DEAD_END_INSIDE, None, [3, 3], [(2, 4), (2, 5)], {"reversed": 1, "usual": 1, "pulled": 1}),
    ("clear", CLEAR, None, [1, 0], [(0, 1), (1, 0)], {"reversed": 1, "clear": 1}),
    ("clear, 1 outranks 0", CLEAR, [0, 5], [1, 4], [(0, 1), (1, 1)], {"reversed": 1, "clear": 1}),
    ("ring", RING, None, [4, 4, 1], [(0, 1), (0, 2), (2, 3)], {}),
]

SERPENTINE_SHAPE = (65, 68)


def serpentine(length):
    """A dead-end corridor of `length` cells that winds through a 65 x 68 map, one obstacle row between its runs, and at
    its mouth a junction: (0, 1) with the side cells (0, 0) and (1, 1).  The dead-end case's two agents stand on the
    corridor's last two cells: 0 wants the last cell, 1 stands on it and wants out, to (0, 0).  swap_possible walks the
    whole corridor back to the junction, which it meets after length - 1 steps.
    Returns (obstacles [65, 68], agents, targets)."""
    H, W = SERPENTINE_SHAPE
    path = []
    for run in range((H + 1) // 2):
        cols = range(2, W) if run % 2 == 0 else range(W - 1, 1, -1)
        path += [(2 * run, c) for c in cols]
        if 2 * run + 1 < H:
            path.append((2 * run + 1, W - 1 if run % 2 == 0 else 2))
    assert 2 <= length <= len(path)
    obstacles = np.ones((H, W), dtype=np.uint8)
    for c in [(0, 0), (0, 1), (1, 1)] + path[:length]:
        obstacles[c] = 0
    return obstacles, [path[length - 2], path[length - 1]], [path[length - 1], (0, 0)]


CAP_LENGTHS = {"below the cap": MAX_WALK, "above the cap": MAX_WALK + 1}   # the junction is met in step length - 1


def solve_suite(n=80, size=12, density=0.35, agents=8, seed=0, min_cells=40):
    """The instances of the solve-rate measurement: one generator `default_rng(seed)` for all of them; per instance the
    map is redrawn until the component of its first free cell has at least `min_cells` cells; agents and targets are
    two independent permutations of that component.  Yields (obstacles, agents, targets)."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        while True:
            obstacles = (rng.random((size, size)) < density).astype(np.uint8)
            free = np.argwhere(obstacles == 0)
            comp = np.argwhere(bfs_from(obstacles != 0, *free[0]) >= 0)
            if len(comp) >= min_cells:
                break
        yield (obstacles, comp[rng.permutation(len(comp))[:agents]].astype(np.int32),
               comp[rng.permutation(len(comp))[:agents]].astype(np.int32))


def head_on_instances(batch, size, agents, seed, density=0.3):
    """States in which the swap rule has work to do from the first call on: random maps of `density` (lowered in steps of
    0.05 for as long as a map has too few free cells).  About half of the agents stand in adjacent pairs whose targets
    are each other's cells -- head on, in whatever corridor, dead end or open space the pair fell into (S23's `usual`
    partner).  About a quarter stand in couples: one agent next to its target, a second one right behind it whose
    target is a random cell, often past the first one's (S23's `clear` partner).  The others stand on random free cells
    with random free targets (reachable or not).  Agent indices are shuffled.
    Returns (obstacles [B, size, size], agents [B, A, 2], targets [B, A, 2], the density used)."""
    rng = np.random.default_rng(seed)
    while True:
        obstacles = (rng.random((batch, size, size)) < density).astype(np.uint8)
        if int((obstacles == 0).sum(axis=(1, 2)).min()) >= max(agents + 2, 4):
            break
        density = round(density - 0.05, 2)
    pos = np.zeros((batch, agents, 2), dtype=np.int32)
    tgt = np.zeros((batch, agents, 2), dtype=np.int32)
    for b in range(batch):
        free = [tuple(c) for c in np.argwhere(obstacles[b] == 0)[rng.permutation(int((obstacles[b] == 0).sum()))]]
        taken, cells, goals = set(), [], []

        def around(c):
            out = [(c[0] + dx, c[1] + dy) for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1))]
            return [u for u in out if 0 <= u[0] < size and 0 <= u[1] < size and not obstacles[b][u] and u not in taken]

        for c in free:                        # head-on pairs
            if len(cells) + 2 > min(agents // 2 + 1, agents):
                break
            if c not in taken and around(c):
                u = around(c)[0]
                taken.update((c, u))
                cells += [c, u]
                goals += [u, c]
        for c in free:                        # couples: c next to its target q, u behind c
            if len(cells) + 2 > min(3 * agents // 4 + 1, agents):
                break
            if c not in taken and len(around(c)) >= 2:
                u, q = around(c)[:2]
                taken.update((c, u, q))
                cells += [c, u]
                goals += [q, free[int(rng.integers(len(free)))]]
        rest = [c for c in free if c not in cells]
        for k in range(agents - len(cells)):
            cells.append(rest[k])
            goals.append(free[int(rng.integers(len(free)))])
        order = rng.permutation(agents)
        pos[b], tgt[b] = np.array(cells, dtype=np.int32)[order], np.array(goals, dtype=np.int32)[order]
    return obstacles, pos, tgt, density


def layout_case(agents, size, batch, r):
    """The state a lane-layout case of the GPU suite installs and its three priority forms (none, random, all equal):
    (obstacles, agents, targets, priorities)."""
    obstacles, pos, tgt, _ = head_on_instances(min(batch, 40), size, agents, seed=agents + r)
    rng = np.random.default_rng(1000 * agents + r)
    shape = pos.shape[:2]
    return obstacles, pos, tgt, (None, rng.integers(-3, 4, size=shape).astype(np.int32), np.full(shape, 7, dtype=np.int32))


def layout_radii(agents):
    return (1, 5) if agents < 1024 else (2,)


def layout_priorities(agents, prios):
    """The priority forms a layout case checks on its installed state: all three up to 256 agents, the random one above
    (the reference is a Python recursion per env)."""
    return prios if agents <= 256 else prios[1:2]


# agents -> what the reference reports at least, summed over the installed states of the layout's case (all radii, the
# priority forms of layout_priorities); `unpulled`: reversed lists whose pull did not happen.  The counts behind it, as
# reversed / clear / pulled: 2: 86 / 0 / 86, 3: 77 / 0 / 77, 8: 161 / 0 / 157, 16: 250 / 3 / 226, 33: 164 / 6 / 125,
# 64: 225 / 8 / 152, 65: 166 / 3 / 139, 200: 295 / 0 / 232, 257: 186 / 0 / 151, 342: 153 / 1 / 126, 512: 223 / 0 / 182,
# 513: 144 / 2 / 125, 1023: 291 / 1 / 216, 1024: 155 / 0 / 124.
LAYOUT_MIN = {2: {"pulled": 1}, 3: {"pulled": 1},
              **{a: {"pulled": 1, "unpulled": 1} for a in (8, 200, 257, 512, 1024)},
              **{a: {"clear": 1, "pulled": 1, "unpulled": 1} for a in (16, 33, 64, 65, 342, 513, 1023)}}


def run_policy(planner, obstacles, agents, targets, steps, finish=False, each_step=None):
    """`planner` (pibt_env or pibt_swap_env) iterated under PibtPolicy's priority rule with every planned agent moving to
    its next cell (what a `soft` step does).  finish: an agent on its target is not planned any more (on_target =
    "finish"), else it stays planned ("nothing") and the instance is solved when all stand on their targets at once.
    Returns the number of steps it took, None when `steps` were not enough.  each_step(pos, active, prio, out): a hook."""
    pos, tgt = np.array(agents), np.array(targets)
    prio = np.zeros(len(pos), dtype=np.int64)
    active = np.ones(len(pos), dtype=bool)
    if finish:
        active &= ~(pos == tgt).all(axis=1)
    for t in range(steps):
        out = planner(obstacles, pos, tgt, active, prio)
        if each_step is not None:
            each_step(pos, active, prio, out)
        pos = out[1].astype(pos.dtype)
        home = (pos == tgt).all(axis=1)
        if finish:
            active = active & ~home
        if (not active.any()) if finish else home.all():
            return t + 1
        prio = np.where(home | ~active, 0, prio + 1)
    return None
