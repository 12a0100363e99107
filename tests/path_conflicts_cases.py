"""Hand-built cases of the path conflicts (docs/SPEC.md S26), shared by the CPU and the GPU suite.  Every case is an
explicit map ('.' free), `agents_xy`, `targets_xy` (row, column), per agent its K path cells, and `checks`: for a choice
of `kinds` and `arrived` the four expected arrays written out, one entry per agent.  `is_active` is the state the arrays
are for; a case with `start_xy` and `actions` reaches it from those start cells by one step under on_target="finish"
(the agent that arrives is hidden), the others are installed as they stand under on_target="nothing".  Targets lie off
the paths unless the case is about them.  Test infrastructure only."""
import numpy as np

VE, ALL = ("vertex", "edge"), ("vertex", "edge", "follow")
BOTH = ("stay", "vanish")


def _open(h, w):
    return ["." * w] * h


def check(kinds, arrived, first, partner, kind, count):
    return dict(kinds=kinds, arrived=arrived, first=first, partner=partner, kind=kind, count=count)


def _same_for(kinds_list, arrived_list, *arrays):
    return [check(k, a, *arrays) for k in kinds_list for a in arrived_list]


_CELLS40 = [[n // 7, n % 7] for n in range(40)]

CASES = [
    # 1. head on in a corridor, three cells apart: they change places between steps 1 and 2
    dict(name="head on, odd distance: edge", map=_open(2, 6), agents_xy=[[0, 0], [0, 3]], targets_xy=[[1, 0], [1, 5]],
         is_active=[True, True],
         paths=[[(0, 1), (0, 2), (0, 3)], [(0, 2), (0, 1), (0, 0)]],
         checks=_same_for((VE, ALL, ("edge",)), BOTH, [2, 2], [1, 0], [2, 2], [1, 1])
         + _same_for((("vertex",), ("follow",)), BOTH, [-1, -1], [-1, -1], [0, 0], [0, 0])),
    # ... four cells apart: both stand on the middle cell at step 2
    dict(name="head on, even distance: vertex", map=_open(2, 6), agents_xy=[[0, 0], [0, 4]], targets_xy=[[1, 0], [1, 5]],
         is_active=[True, True],
         paths=[[(0, 1), (0, 2), (0, 3)], [(0, 3), (0, 2), (0, 1)]],
         checks=_same_for((VE, ALL, ("vertex",)), BOTH, [2, 2], [1, 0], [1, 1], [1, 1])
         + _same_for((("edge",), ("follow",), ("edge", "follow")), BOTH, [-1, -1], [-1, -1], [0, 0], [0, 0])),
    # 2. three agents step onto (1, 1) at once
    dict(name="three reach one cell", map=_open(3, 3), agents_xy=[[0, 1], [1, 0], [1, 2]],
         targets_xy=[[2, 1], [2, 2], [2, 0]], is_active=[True, True, True],
         paths=[[(1, 1)], [(1, 1)], [(1, 1)]],
         checks=_same_for((VE, ALL), BOTH, [1, 1, 1], [1, 0, 0], [1, 1, 1], [2, 2, 2])),
    # 3. three in a row, all moving right for two steps: 1 follows 0 and 2 follows 1, twice; 0 follows nobody
    dict(name="follow chain", map=_open(2, 5), agents_xy=[[0, 2], [0, 1], [0, 0]], targets_xy=[[1, 4], [1, 3], [1, 2]],
         is_active=[True, True, True],
         paths=[[(0, 3), (0, 4)], [(0, 2), (0, 3)], [(0, 1), (0, 2)]],
         checks=_same_for((ALL, ("follow",)), BOTH, [-1, 1, 1], [-1, 0, 1], [0, 4, 4], [0, 2, 2])
         + _same_for((VE,), BOTH, [-1, -1, -1], [-1, -1, -1], [0, 0, 0], [0, 0, 0])),
    # 4. agent 1 arrives at (1, 2) at step 2 and waits there; agent 0 steps onto that cell at step 4
    dict(name="crosses a target after the arrival", map=_open(3, 5), agents_xy=[[0, 2], [1, 0]],
         targets_xy=[[2, 4], [1, 2]], is_active=[True, True],
         paths=[[(0, 2), (0, 2), (0, 2), (1, 2)], [(1, 1), (1, 2), (1, 2), (1, 2)]],
         checks=_same_for((VE, ALL), ("stay",), [4, 4], [1, 0], [1, 1], [1, 1])
         + _same_for((VE, ALL), ("vanish",), [-1, -1], [-1, -1], [0, 0], [0, 0])),
    # ... agent 0 steps onto it at step 2, the arrival step itself: agent 1 still takes part
    dict(name="enters a target at the arrival step", map=_open(3, 5), agents_xy=[[0, 2], [1, 0]],
         targets_xy=[[2, 4], [1, 2]], is_active=[True, True],
         paths=[[(0, 2), (1, 2), (2, 2), (2, 2)], [(1, 1), (1, 2), (1, 2), (1, 2)]],
         checks=_same_for((VE, ALL), BOTH, [2, 2], [1, 0], [1, 1], [1, 1])),
    # 5. agent 0 is active and stands on its target: under vanish it takes part in no step 1..K
    dict(name="stands on its target", map=_open(2, 4), agents_xy=[[0, 0], [0, 2]], targets_xy=[[0, 0], [1, 3]],
         is_active=[True, True],
         paths=[[(0, 0), (0, 0)], [(0, 1), (0, 0)]],
         checks=_same_for((VE, ALL), ("stay",), [2, 2], [1, 0], [1, 1], [1, 1])
         + _same_for((VE, ALL), ("vanish",), [-1, -1], [-1, -1], [0, 0], [0, 0])),
    # 6. agent 0 has arrived and is hidden on (0, 1); agent 1 walks over that cell
    dict(name="inactive agent", map=_open(3, 3), agents_xy=[[0, 1], [1, 1]], targets_xy=[[0, 1], [2, 2]],
         is_active=[False, True], start_xy=[[0, 0], [1, 1]], actions=[4, 0],
         paths=[[(0, 1), (0, 1)], [(0, 1), (0, 2)]],
         checks=_same_for((VE, ALL), BOTH, [-1, -1], [-1, -1], [0, 0], [0, 0])),
    # 7. a vertex at step 1; agent 0 is off the map at step 2; at step 3 it enters the cell agent 1 leaves, which is no
    #    follow, as it took no part at step 2; at step 4 they change places
    dict(name="a cell outside the map", map=_open(2, 4), agents_xy=[[0, 0], [0, 2]], targets_xy=[[1, 0], [1, 3]],
         is_active=[True, True],
         paths=[[(0, 1), (-1, -1), (0, 2), (0, 3)], [(0, 1), (0, 2), (0, 3), (0, 2)]],
         checks=_same_for((VE, ALL), BOTH, [1, 1], [1, 0], [1, 1], [2, 2])
         + _same_for((("edge",), ("edge", "follow")), BOTH, [4, 4], [1, 0], [2, 2], [1, 1])
         + _same_for((("follow",),), BOTH, [-1, -1], [-1, -1], [0, 0], [0, 0])),
    # 8. agent 0 changes places with agent 1 while agent 3 steps onto the same cell; agent 3 thereby follows agent 1
    dict(name="vertex and edge at one step", map=_open(3, 3), agents_xy=[[1, 1], [1, 2], [2, 0], [0, 2]],
         targets_xy=[[0, 0], [2, 2], [2, 1], [0, 1]], is_active=[True] * 4,
         paths=[[(1, 2)], [(1, 1)], [(2, 0)], [(1, 2)]],
         checks=_same_for((VE,), BOTH, [1, 1, -1, 1], [1, 0, -1, 0], [3, 2, 0, 1], [2, 1, 0, 1])
         + _same_for((ALL,), BOTH, [1, 1, -1, 1], [1, 0, -1, 0], [3, 2, 0, 5], [2, 1, 0, 2])),
    # 9. cells are keys, not moves: a swap across the map is an edge
    dict(name="swap by a jump", map=_open(3, 3), agents_xy=[[0, 0], [2, 2]], targets_xy=[[0, 2], [2, 0]],
         is_active=[True, True],
         paths=[[(2, 2)], [(0, 0)]],
         checks=_same_for((VE, ALL), BOTH, [1, 1], [1, 0], [2, 2], [1, 1])),
    # 10. five cells apart: the edge is at step 3 = K
    dict(name="first conflict at step K", map=_open(2, 6), agents_xy=[[0, 0], [0, 5]], targets_xy=[[1, 0], [1, 5]],
         is_active=[True, True],
         paths=[[(0, 1), (0, 2), (0, 3)], [(0, 4), (0, 3), (0, 2)]],
         checks=_same_for((VE, ALL), BOTH, [3, 3], [1, 0], [2, 2], [1, 1])),
    # 11. forty agents step onto (6, 6) at once
    dict(name="forty on one cell", map=_open(7, 7), agents_xy=_CELLS40, targets_xy=_CELLS40[1:] + _CELLS40[:1],
         is_active=[True] * 40,
         paths=[[(6, 6)]] * 40,
         checks=_same_for((VE, ALL), BOTH, [1] * 40, [1] + [0] * 39, [1] * 40, [39] * 40)),
]


# The random inputs of the GPU suite, as tests/util.py's generate_instances takes them; tests/test_path_conflicts.py
# proves on the CPU that they are not vacuous.  `steps`: the forecast's K / the plan's horizon.
FORECAST_INPUTS = (dict(batch=16, size=12, agents=16, density=0.3, seed=26, steps=8),
                   dict(batch=4, size=24, agents=64, density=0.3, seed=27, steps=8))
PLAN_INPUT = dict(batch=4, size=16, agents=24, density=0.2, seed=28, steps=32)


def grid(rows):
    """The case's map as uint8 [H, W], 1 = obstacle."""
    return np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)


def paths_of(case, layout, batch=1):
    """The case's paths in a layout, `batch` copies: "cells" int16 [B, A, K, 2] or "plan" int32 [K, B, A, 2]."""
    cells = np.repeat(np.array(case["paths"], dtype=np.int16)[None], batch, 0)
    return cells if layout == "cells" else np.ascontiguousarray(cells.transpose(2, 0, 1, 3)).astype(np.int32)


def expected(chk):
    """The four arrays of a check: int32, int32, uint8, int32 [A]."""
    return (np.array(chk["first"], dtype=np.int32), np.array(chk["partner"], dtype=np.int32),
            np.array(chk["kind"], dtype=np.uint8), np.array(chk["count"], dtype=np.int32))
