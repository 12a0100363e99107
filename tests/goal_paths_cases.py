"""Hand-built cases of the path-to-goal planes (docs/SPEC.md S22), shared by the CPU and the GPU suite.  Every case is an
explicit map ('.' free, '#' obstacle), `agents_xy`, `targets_xy` (row, column), the radius and the cap, with the expected
arrays written out: per agent the (2r+1) x (2r+1) plane, the sub-goal's offset (dx, dy), the length, and what ended the
marked prefix ("target", "edge", "cap", or None for length 0).  `is_active` is the state the arrays are for; a case with
`start_xy` and `actions` reaches it from those start cells by one step under on_target="finish" (the agent that arrives
is hidden).  Test infrastructure only."""
import numpy as np

OPEN3 = ["...",
         "...",
         "..."]
OPEN4 = ["....",
         "....",
         "....",
         "...."]
WINDING = [".....",
           ".###.",
           ".#...",
           ".####",
           "....."]

CASES = [
    # D = x + y: up to (0, 1), where up is off the map and left reaches the target
    dict(name="open 3x3", map=OPEN3, r=1, steps=None, agents_xy=[[1, 1]], targets_xy=[[0, 0]], is_active=[True],
         planes=[[[1, 1, 0],
                  [0, 0, 0],
                  [0, 0, 0]]], subgoal=[[-1, -1]], length=[2], end=["target"]),
    # the wall at (1, 2) makes up and down equally good, 4 steps each: up wins, then right, then the window ends
    dict(name="two equally good moves", map=[".....",
                                             "..#..",
                                             "....."], r=1, steps=None, agents_xy=[[1, 1]], targets_xy=[[1, 3]],
         is_active=[True],
         planes=[[[0, 1, 1],
                  [0, 0, 0],
                  [0, 0, 0]]], subgoal=[[-1, 1]], length=[2], end=["edge"]),
    # the halo's first row and first column lie outside the map
    dict(name="map corner", map=["......"] * 4, r=1, steps=None, agents_xy=[[0, 0]], targets_xy=[[0, 5]], is_active=[True],
         planes=[[[0, 0, 0],
                  [0, 0, 1],
                  [0, 0, 0]]], subgoal=[[0, 1]], length=[1], end=["edge"]),
    dict(name="on the target", map=OPEN3, r=1, steps=None, agents_xy=[[1, 1]], targets_xy=[[1, 1]], is_active=[True],
         planes=[[[0, 0, 0]] * 3], subgoal=[[0, 0]], length=[0], end=[None]),
    dict(name="unreachable target", map=["..#..",
                                         "..#..",
                                         "..#.."], r=2, steps=None, agents_xy=[[1, 3]], targets_xy=[[1, 0]], is_active=[True],
         planes=[[[0, 0, 0, 0, 0]] * 5], subgoal=[[0, 0]], length=[0], end=[None]),
    # agent 0 steps right onto its target and is hidden; agent 1 stays: left to (2, 1), then the window ends
    dict(name="inactive agent", map=OPEN3, r=1, steps=None, agents_xy=[[0, 1], [2, 2]], targets_xy=[[0, 1], [2, 0]],
         is_active=[False, True], start_xy=[[0, 0], [2, 2]], actions=[4, 0],
         planes=[[[0, 0, 0]] * 3,
                 [[0, 0, 0],
                  [1, 0, 0],
                  [0, 0, 0]]], subgoal=[[0, 0], [0, -1]], length=[0, 1], end=[None, "edge"]),
    # the window of the agent at (2, 1) holds rows 1..3 and columns 0..2.  Up to (1, 1) either way; there the target on
    # the last window cell (1, 2) is one step to the right ...
    dict(name="target on the last window cell", map=OPEN4, r=1, steps=None, agents_xy=[[2, 1]], targets_xy=[[1, 2]],
         is_active=[True],
         planes=[[[0, 1, 1],
                  [0, 0, 0],
                  [0, 0, 0]]], subgoal=[[-1, 1]], length=[2], end=["target"]),
    # ... and with the target one cell beyond, at (0, 2), up is closer too, is the lower move and leaves the window: the
    # halo row decides (a walk that knew the window alone would turn right and mark (1, 2) as above)
    dict(name="target one cell beyond the window", map=OPEN4, r=1, steps=None, agents_xy=[[2, 1]], targets_xy=[[0, 2]],
         is_active=[True],
         planes=[[[0, 1, 0],
                  [0, 0, 0],
                  [0, 0, 0]]], subgoal=[[-1, 0]], length=[1], end=["edge"]),
    # 16 of the window's 25 cells: right, right, up, up, left x 4, down x 4, right x 4
    dict(name="winding corridor", map=WINDING, r=2, steps=None, agents_xy=[[2, 2]], targets_xy=[[4, 4]], is_active=[True],
         planes=[[[1, 1, 1, 1, 1],
                  [1, 0, 0, 0, 1],
                  [1, 0, 0, 1, 1],
                  [1, 0, 0, 0, 0],
                  [1, 1, 1, 1, 1]]], subgoal=[[2, 2]], length=[16], end=["target"]),
    dict(name="winding corridor, steps 3", map=WINDING, r=2, steps=3, agents_xy=[[2, 2]], targets_xy=[[4, 4]],
         is_active=[True],
         planes=[[[0, 0, 0, 0, 0],
                  [0, 0, 0, 0, 1],
                  [0, 0, 0, 1, 1],
                  [0, 0, 0, 0, 0],
                  [0, 0, 0, 0, 0]]], subgoal=[[-1, 2]], length=[3], end=["cap"]),
]


def grid(rows):
    """The case's map as uint8 [H, W], 1 = obstacle."""
    return np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)


def expected(case):
    """(planes uint8 [A, w, w], subgoal int8 [A, 2], length int32 [A]) as the case states them."""
    return (np.array(case["planes"], dtype=np.uint8), np.array(case["subgoal"], dtype=np.int8),
            np.array(case["length"], dtype=np.int32))
