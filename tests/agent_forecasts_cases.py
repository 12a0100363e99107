"""Hand-built cases of the agent forecasts (docs/SPEC.md S24), shared by the CPU and the GPU suite.  Every case is an
explicit map ('.' free, '#' obstacle), `agents_xy`, `targets_xy` (row, column), the radius (1 throughout: 3 x 3 windows)
and K = `steps`, with the expected arrays written out: per agent its K forecast cells and its K planes, a plane as its
three rows "abc/def/ghi".  `is_active` is the state the arrays are for; a case with `start_xy` and `actions` reaches it from
those start cells by one step under on_target="finish" (the agent that arrives is hidden), the others are installed as
they stand under on_target="nothing".  Test infrastructure only."""
import numpy as np

OPEN3 = ["...",
         "...",
         "..."]
ZERO = "000/000/000"

CASES = [
    # agent 0: right, right onto its target, then it waits; agent 1 stands on its target and waits from step 1.  Agent 1
    # sees 0's cells (0, 1), (0, 2), (0, 2) in its top row; agent 0 sees 1's cell (1, 1) in its corner
    dict(name="arrives at step 2 and waits", map=OPEN3, r=1, steps=3, agents_xy=[[0, 0], [1, 1]],
         targets_xy=[[0, 2], [1, 1]], is_active=[True, True],
         cells=[[(0, 1), (0, 2), (0, 2)], [(1, 1)] * 3],
         planes=[["000/000/001"] * 3,
                 ["010/000/000", "001/000/000", "001/000/000"]]),
    # the wall cuts agent 0 off from its target: it waits from step 1.  Agent 1 walks down through 0's cell (other agents
    # are not obstacles): 0 sees it on its own centre, then below it
    dict(name="unreachable target", map=[".#.",
                                         ".#.",
                                         ".#."], r=1, steps=3, agents_xy=[[1, 0], [0, 0]], targets_xy=[[1, 2], [2, 0]],
         is_active=[True, True],
         cells=[[(1, 0)] * 3, [(1, 0), (2, 0), (2, 0)]],
         planes=[["000/010/000", "000/000/010", "000/000/010"],
                 ["000/000/010"] * 3]),
    # agents 0 (down) and 1 (right) both stand on (1, 1) after one step, where agent 2 waits: one cell, one 1
    dict(name="two forecasts on one cell", map=OPEN3, r=1, steps=3, agents_xy=[[0, 1], [1, 0], [1, 1]],
         targets_xy=[[2, 1], [1, 2], [1, 1]], is_active=[True, True, True],
         cells=[[(1, 1), (2, 1), (2, 1)], [(1, 1), (1, 2), (1, 2)], [(1, 1)] * 3],
         planes=[["000/000/010", "000/000/011", "000/000/011"],
                 ["000/001/000", "000/001/001", "000/001/001"],
                 ["000/010/000", "000/001/010", "000/001/010"]]),
    # agent 0 waits on (1, 1): its window is rows 0..2, columns 0..2.  Agent 1 at (2, 2) has walls above and to its left:
    # right to column 3 (outside the window), up, up, then left to (0, 2): back inside at step 4.  Agent 2 at (2, 0) steps
    # down to row 3 and stays outside.  Both are visible now; neither is clamped to the edge
    dict(name="leaves the window, re-enters it", map=["....",
                                                       "..#.",
                                                       ".#..",
                                                       "...."], r=1, steps=4, agents_xy=[[1, 1], [2, 2], [2, 0]],
         targets_xy=[[1, 1], [0, 2], [3, 0]], is_active=[True, True, True],
         cells=[[(1, 1)] * 4, [(2, 3), (1, 3), (0, 3), (0, 2)], [(3, 0)] * 4],
         planes=[[ZERO, ZERO, ZERO, "001/000/000"],
                 ["100/000/000"] * 4,
                 ["001/000/000"] * 4]),
    # agent 1 stands two columns from agent 0 and steps into 0's window: it is not visible now, so it is not drawn
    dict(name="enters the window from outside", map=["...."] * 3, r=1, steps=3, agents_xy=[[1, 0], [1, 2]],
         targets_xy=[[1, 0], [1, 1]], is_active=[True, True],
         cells=[[(1, 0)] * 3, [(1, 1)] * 3],
         planes=[[ZERO] * 3, [ZERO] * 3]),
    # agent 0 steps right onto its target and is hidden: no forecast, zero planes, and agent 1, whose window holds it at
    # (0, 0), does not draw it.  Agent 1 draws agent 2's (2, 2); agent 2 draws agent 1's (1, 1), (1, 0), (1, 0)
    dict(name="inactive agent", map=OPEN3, r=1, steps=3, agents_xy=[[0, 1], [1, 2], [2, 1]],
         targets_xy=[[0, 1], [1, 0], [2, 2]], is_active=[False, True, True], start_xy=[[0, 0], [1, 2], [2, 1]],
         actions=[4, 0, 0],
         cells=[[(-1, -1)] * 3, [(1, 1), (1, 0), (1, 0)], [(2, 2)] * 3],
         planes=[[ZERO] * 3,
                 ["000/000/010"] * 3,
                 ["010/000/000", "100/000/000", "100/000/000"]]),
    # up and left are equally good for agent 0: up wins, which agent 1 sees in its corner (left would leave its window at
    # once); the second step is outside
    dict(name="up before left", map=OPEN3, r=1, steps=3, agents_xy=[[1, 1], [1, 2]], targets_xy=[[0, 0], [1, 2]],
         is_active=[True, True],
         cells=[[(0, 1), (0, 0), (0, 0)], [(1, 2)] * 3],
         planes=[["000/001/000"] * 3,
                 ["100/000/000", ZERO, ZERO]]),
]


def grid(rows):
    """The case's map as uint8 [H, W], 1 = obstacle."""
    return np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)


def expected(case, steps=None):
    """(planes uint8 [A, K, w, w], cells int16 [A, K, 2]) as the case states them; `steps` below the case's own: the
    first `steps` of them (a forecast's prefix is the shorter forecast)."""
    K = case["steps"] if steps is None else steps
    planes = np.array([[[[int(c) for c in row] for row in plane.split("/")] for plane in agent] for agent in case["planes"]],
                      dtype=np.uint8)
    return planes[:, :K], np.array(case["cells"], dtype=np.int16)[:, :K]
