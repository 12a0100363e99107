"""Hand-built cases of the blocking counts (docs/SPEC.md S25), shared by the CPU and the GPU suite.  Every case is an
explicit map of at most 5 x 7 cells ('.' free, '#' obstacle), `agents_xy`, `targets_xy` (row, column) and the radius (1
or 2), with the expected arrays written out: `expect` maps (inflation, blockers) to (count, blocked_by).  `is_active` is
the state the arrays are for; a case with `start_xy` and `actions` reaches it from those start cells by one step under
on_target="finish" (the agent that arrives is hidden), the others are installed as they stand under on_target="nothing".
Path lengths between two cells of a grid all have the same parity, so a detour is an even number of steps: the detour
maps below have detours of exactly 2 and 4 steps, each checked at the inflation that equals it (blocked) and at the
inflation one above (detour = inflation - 1: not blocked).  Test infrastructure only."""
import numpy as np

CORRIDOR5 = ["#####",
             ".....",
             "#####"]
CORRIDOR7 = ["#######",
             ".......",
             "#######"]
OPEN3 = ["...",
         "...",
         "..."]
# the straight way along row 2 is the only shortest path from (2, 0) to (2, 4); around (2, 2) through row 1: 2 steps more
DETOUR2 = [".....",
           ".....",
           ".....",
           "#####"]
# the same map with one more wall, at (1, 2): around (2, 2) through row 0 now, 4 steps more
DETOUR4 = [".....",
           "..#..",
           ".....",
           "#####"]
ANY = (1, 2, 10, 64)          # the inflations a cut-off pair (or nobody blocked) is checked at: the answer is the same


def _every(count, blocked_by, on_target=None, inflations=ANY):
    """The same arrays at every inflation; `on_target`: the arrays under blockers="on_target" (default: the same)."""
    other = (count, blocked_by) if on_target is None else on_target
    out = {}
    for k in inflations:
        out[(k, "all")] = (count, blocked_by)
        out[(k, "on_target")] = other
    return out


def _upto(limit, count, blocked_by):
    """Blocked as written for inflation <= limit, nobody blocked above it; the blocker stands on its own target."""
    out = {}
    for k in (1, 2, 3, 4, 5, 10):
        got = (count, blocked_by) if k <= limit else ([0] * len(count), [0] * len(count))
        out[(k, "all")] = out[(k, "on_target")] = got
    return out


CASES = [
    # agent 1 stands behind agent 0 in a one-wide corridor and wants to pass: cut off, at any inflation.  Agent 0 walks
    # away from agent 1, which is not in its way; it does not stand on its target, so "on_target" leaves it out
    dict(name="corridor, cut off", map=CORRIDOR5, r=1, agents_xy=[[1, 2], [1, 1]], targets_xy=[[1, 3], [1, 4]],
         is_active=[True, True], expect=_every([1, 0], [0, 1], on_target=([0, 0], [0, 0]))),
    # agent 1 sits in the middle of agent 0's diagonal: 0 walks around it in as many steps
    dict(name="open 3 x 3, nobody blocked", map=OPEN3, r=1, agents_xy=[[0, 0], [1, 1]], targets_xy=[[2, 2], [1, 1]],
         is_active=[True, True], expect=_every([0, 0], [0, 0])),
    dict(name="detour of 2", map=DETOUR2, r=2, agents_xy=[[2, 2], [2, 0]], targets_xy=[[2, 2], [2, 4]],
         is_active=[True, True], expect=_upto(2, [1, 0], [0, 1])),
    dict(name="detour of 4, one more wall", map=DETOUR4, r=2, agents_xy=[[2, 2], [2, 0]], targets_xy=[[2, 2], [2, 4]],
         is_active=[True, True], expect=_upto(4, [1, 0], [0, 1])),
    # agent 0 stands on agent 1's target: no path ends there, at any inflation.  Agent 1 is not in agent 0's way
    dict(name="on the other's target", map=OPEN3, r=1, agents_xy=[[2, 2], [1, 1]], targets_xy=[[0, 0], [2, 2]],
         is_active=[True, True], expect=_every([1, 0], [0, 1], on_target=([0, 0], [0, 0]))),
    # the wall cuts agent 1 off from its target: nobody blocks it.  It stands in the only way of agent 0
    dict(name="unreachable target", map=[".#.",
                                         ".#.",
                                         ".#."], r=1, agents_xy=[[0, 0], [1, 0]], targets_xy=[[2, 0], [1, 2]],
         is_active=[True, True], expect=_every([0, 1], [1, 0], on_target=([0, 0], [0, 0]))),
    # agent 0 stands on the only path of agent 1, two columns away: outside its 3 x 3 window, not counted (the rule is
    # symmetric: agent 0 is as far outside agent 1's).  Agent 2 between them is in both windows: blocked by 0, blocks 1
    dict(name="outside the window", map=CORRIDOR7, r=1, agents_xy=[[1, 3], [1, 1], [1, 2]],
         targets_xy=[[1, 3], [1, 6], [1, 5]], is_active=[True, True, True],
         expect=_every([1, 0, 1], [0, 1, 1], on_target=([1, 0, 0], [0, 0, 1]))),
    # agent 0 steps right onto its target and is hidden: where it stands it would cut agent 1 off, but it is not active
    dict(name="inactive agent", map=CORRIDOR5, r=2, agents_xy=[[1, 2], [1, 0]], targets_xy=[[1, 2], [1, 4]],
         is_active=[False, True], start_xy=[[1, 1], [1, 0]], actions=[4, 0], expect=_every([0, 0], [0, 0])),
    # agent 0 in the middle of the corridor, agents 1 and 2 want to pass it from both sides (and do not see each other)
    dict(name="one blocks two", map=CORRIDOR5, r=1, agents_xy=[[1, 2], [1, 1], [1, 3]],
         targets_xy=[[1, 2], [1, 4], [1, 0]], is_active=[True, True, True], expect=_every([2, 0, 0], [0, 1, 1])),
    # agents 0 and 2 wait on their targets, one behind the other, in front of agent 1
    dict(name="one blocked by two", map=CORRIDOR5, r=2, agents_xy=[[1, 1], [1, 0], [1, 2]],
         targets_xy=[[1, 1], [1, 4], [1, 2]], is_active=[True, True, True], expect=_every([1, 0, 1], [0, 2, 0])),
    # as before, but agent 2 is on its way to (1, 3): "all" counts it, "on_target" does not
    dict(name="on_target leaves a blocker out", map=CORRIDOR5, r=2, agents_xy=[[1, 1], [1, 0], [1, 2]],
         targets_xy=[[1, 1], [1, 4], [1, 3]], is_active=[True, True, True],
         expect=_every([1, 0, 1], [0, 2, 0], on_target=([1, 0, 0], [0, 1, 0]))),
]


def grid(rows):
    """The case's map as uint8 [H, W], 1 = obstacle."""
    return np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)


# ---- the random inputs of the GPU suite, built on the host so that the CPU suite can prove they are not vacuous --------
def _component(blocked, x, y):
    """The cells 4-connected to the free cell (x, y), as an int array [n, 2] in row-major order."""
    H, W = blocked.shape
    seen = np.zeros((H, W), dtype=bool)
    seen[x, y] = True
    stack = [(x, y)]
    while stack:
        cx, cy = stack.pop()
        for nx, ny in ((cx - 1, cy), (cx + 1, cy), (cx, cy - 1), (cx, cy + 1)):
            if 0 <= nx < H and 0 <= ny < W and not blocked[nx, ny] and not seen[nx, ny]:
                seen[nx, ny] = True
                stack.append((nx, ny))
    return np.argwhere(seen)


def instances(batch, height, width, agents, density, seed, cluster=None, reach=None):
    """`batch` random instances (obstacles uint8 [B, H, W], agents_xy int32 [B, A, 2], targets_xy int32 [B, A, 2]), a
    pure function of the arguments.  Per env: Bernoulli(density) obstacles; a connected component of at least `agents`
    cells and at least a quarter of the free ones (an env that has none within 64 draws gets an open map); distinct start
    cells in it -- with `cluster` all within that Chebyshev distance of one of its cells (grown until they fit), so that
    the agents see each other; a target for every agent in it (targets may coincide, and lie on start cells) -- with
    `reach` within that Chebyshev distance of the agent's start, so that a naive search ends early."""
    rng = np.random.default_rng(seed)
    obstacles = np.zeros((batch, height, width), dtype=np.uint8)
    starts = np.zeros((batch, agents, 2), dtype=np.int32)
    targets = np.zeros((batch, agents, 2), dtype=np.int32)
    for b in range(batch):
        blocked = rng.random((height, width)) < density
        comp = None
        for _ in range(64):
            free = np.argwhere(~blocked)
            if len(free) == 0:
                break
            x, y = free[rng.integers(len(free))]
            cells = _component(blocked, x, y)
            if len(cells) >= max(agents, len(free) // 4):
                comp = cells
                break
        if comp is None:
            blocked[:] = False
            comp = np.argwhere(~blocked)
        pool = comp
        if cluster is not None:
            centre = comp[rng.integers(len(comp))]
            rad = cluster
            while True:
                pool = comp[np.abs(comp - centre).max(1) <= rad]
                if len(pool) >= agents:
                    break
                rad += 1
        starts[b] = pool[rng.permutation(len(pool))[:agents]]
        for a in range(agents):
            cand = comp if reach is None else comp[np.abs(comp - starts[b, a]).max(1) <= reach]
            targets[b, a] = cand[rng.integers(len(cand))]
        obstacles[b] = blocked
    return obstacles, starts, targets


# one env per line covers every collision system and every on_target mode
MODES = (("priority", "finish"), ("block_both", "restart"), ("soft", "nothing"))
RADIUS = 3
# map side -> the three runs of the side's group: (agents, inflation, density, seed).  Chosen so that the reference alone
# finds, over the reset states of each group, a pair blocked by cut-off, one blocked by a detour and one that passes
# the filter and is still not blocked (tests/test_blocking.py proves it).  Four cells hold no detour and one agent no
# pair: side 2 is there for the kernel's smallest shape, not for the counts
SQUARE_GROUPS = {
    2: ((1, 2, 0.0, 2), (1, 3, 0.0, 3), (1, 4, 0.0, 4)),
    8: ((1, 2, 0.35, 8), (6, 3, 0.35, 9), (13, 4, 0.3, 10)),
    33: ((1, 2, 0.35, 33), (6, 3, 0.38, 34), (13, 4, 0.38, 35)),
    64: ((1, 2, 0.35, 64), (6, 3, 0.38, 65), (13, 2, 0.38, 66)),
    65: ((1, 2, 0.35, 67), (6, 3, 0.38, 68), (13, 2, 0.38, 69)),
}
SQUARE_BATCH = 3


def square_instance(size, k):
    """Run k of SQUARE_GROUPS[size]: (obstacles, agents_xy, targets_xy, inflation)."""
    agents, inflation, density, seed = SQUARE_GROUPS[size][k]
    return instances(SQUARE_BATCH, size, size, agents, density, seed, cluster=RADIUS) + (inflation,)


# 257 x 256 has more than 65536 cells: 4-byte fields
WIDE = dict(height=257, width=256, agents=6, batch=2, r=2, density=0.38, seed=257, inflation=3)


def wide_instance():
    c = WIDE
    return instances(c["batch"], c["height"], c["width"], c["agents"], c["density"], c["seed"], cluster=c["r"], reach=12)


# (agents, map side, batch) -> obs_radius, inflation, density, seed: a row of tests/agent_counts.py's LAYOUT_ROWS and the
# 1024-agent row, each at a radius it accepts that keeps the naive reference of one env at a few thousand short searches
MANY = {(257, 40, 5): dict(r=5, inflation=2, density=0.2, seed=257, reach=6),
        (1024, 64, 2): dict(r=1, inflation=2, density=0.1, seed=1024, reach=3)}


def many_instance(row):
    agents, size, batch = row
    c = MANY[row]
    return instances(batch, size, size, agents, c["density"], c["seed"], reach=c["reach"])
