"""Hand-built cases of plan repair (docs/SPEC.md S29), worked out on paper from the specification: each names a map
('#' = obstacle), the agents' cells and targets, which agents are planned, the given paths [K][A][2], the replan mask,
the priorities, the on_target mode and the five outputs.  tests/test_repair_plan.py proves the CPU reference on them,
tests/test_repair_plan_gpu.py runs them on the engine.  `start`, where a case has one, is how the engine gets into the
case's state: the cells to reset to and one joint action to step."""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
JUNK = [I32_MAX, -5]

# (d): one agent on (0,0) of a 3 x 3 map with an obstacle in the centre, target (0,2), `finish`, K = 3, replan = 0.
# Each of these given paths is no walk, so the agent is replanned -- alone: R_1 = {(0,0), (1,0), (0,1)}, the target is
# in R_2, and read back with the lowest action first the path is right, right.
NOT_WALKS = {
    "first cell not adjacent": [[2, 0], [2, 1], [2, 2]],
    "first cell diagonal": [[1, 1], [1, 2], [0, 2]],
    "jump mid-path": [[0, 1], [2, 1], [2, 2]],
    "step into an obstacle": [[1, 0], [1, 1], [1, 2]],
    "row below the map": [[1, 0], [2, 0], [3, 0]],
    "row above the map": [[0, 1], [-1, 1], [0, 1]],
    "column beyond the map": [[1, 0], [2, 0], [2, 3]],
    "INT32_MIN row": [[I32_MIN, 0], [0, 0], [0, 0]],
    "INT32_MAX column": [[0, I32_MAX], [0, 0], [0, 0]],
    "INT32_MIN column after a step right": [[0, 1], [0, I32_MIN], [0, 1]],
    "both extremes mid-path": [[0, 1], [I32_MAX, I32_MIN], [0, 1]],
}

CASES = [
    # (a) A corridor (row 1) with a bay at (0,1).  Agent 0 is kept and walks the corridor from right to left; agent 1
    # has to pass it the other way.  Its layers: R_1 = {(1,0), (1,1)}; at step 2 (1,1) is agent 0's and the move
    # (1,1) -> (1,2) is the reverse of agent 0's, so R_2 = {(1,0), (0,1)}; at step 3 (1,0) is agent 0's and (1,0) -> (1,1)
    # is the reverse of its move, so R_3 = {(0,1), (1,1)}: only the bay led on.  R_5 holds the target (1,3); read back
    # with the lowest action first: right, right from (1,1), which was entered from the bay (`down`), entered from (1,1)
    # (`up`), entered from (1,0).
    dict(name="(a) corridor with a bay", map=["#.##", "...."], agents=[[1, 3], [1, 0]], targets=[[1, 0], [1, 3]],
         on_target="nothing", priority=None, replan=[0, 1],
         paths=[[[1, 2], [0, 0]], [[1, 1], [0, 0]], [[1, 0], [0, 0]], [[1, 0], [0, 0]], [[1, 0], [0, 0]]],
         actions=[[3, 4], [3, 1], [3, 2], [0, 4], [0, 4]],
         path=[[[1, 2], [1, 1]], [[1, 1], [0, 1]], [[1, 0], [1, 1]], [[1, 0], [1, 2]], [[1, 0], [1, 3]]],
         arrival=[3, 5], failed=[0, 0], replanned=[0, 1]),
    # (b) Agent 0 is kept and steps from (0,1) onto agent 1's cell (0,0).  Agent 1 cannot stay (vertex) and cannot go
    # to its target (0,1): that cell is free at step 1, but the move is the reverse of agent 0's (edge).  R_1 = {(1,0)},
    # R_2 = {(1,0), (1,1)}; (1,1) is nearer to the target.
    dict(name="(b) head-on", map=["..", ".."], agents=[[0, 1], [0, 0]], targets=[[0, 0], [0, 1]], on_target="nothing",
         priority=None, replan=[0, 1], paths=[[[0, 0], JUNK], [[0, 0], JUNK]],
         actions=[[3, 2], [0, 4]], path=[[[0, 0], [1, 0]], [[0, 0], [1, 1]]],
         arrival=[1, -1], failed=[0, 0], replanned=[0, 1]),
    # (c) `finish`: agent 0 is kept, arrives on (0,3) at step 2 and reserves nothing afterwards; what `paths` holds for
    # it after that step is ignored.  Agent 1 follows one cell behind and stands on (0,3) at step 3.
    dict(name="(c) a kept agent arrives and vanishes", map=["....."], agents=[[0, 1], [0, 0]], targets=[[0, 3], [0, 4]],
         on_target="finish", priority=None, replan=[0, 1],
         paths=[[[0, 2], [0, 0]], [[0, 3], [0, 0]], [JUNK, [0, 0]], [[7, 7], [0, 0]]],
         actions=[[4, 4], [4, 4], [0, 4], [0, 4]],
         path=[[[0, 2], [0, 1]], [[0, 3], [0, 2]], [[0, 3], [0, 3]], [[0, 3], [0, 4]]],
         arrival=[2, 4], failed=[0, 0], replanned=[0, 1]),
    # the same under `nothing`: now the cell off the map at step 3 makes agent 0's path no walk, so both agents are
    # replanned, agent 0 first (equal priorities: index order).  Agent 0: R_2 holds (0,3); it walks there and keeps it.
    # Agent 1: (0,3) is taken from step 2 to the end of the window, the nearest cell of R_4 is (0,2), which it can
    # stand on from step 2 on ((0,2) is agent 0's at step 1).
    dict(name="(c') the same garbage under nothing", map=["....."], agents=[[0, 1], [0, 0]], targets=[[0, 3], [0, 4]],
         on_target="nothing", priority=None, replan=[0, 1],
         paths=[[[0, 2], [0, 0]], [[0, 3], [0, 0]], [JUNK, [0, 0]], [[7, 7], [0, 0]]],
         actions=[[4, 4], [4, 4], [0, 0], [0, 0]],
         path=[[[0, 2], [0, 1]], [[0, 3], [0, 2]], [[0, 3], [0, 2]], [[0, 3], [0, 2]]],
         arrival=[2, -1], failed=[0, 0], replanned=[1, 1]),
    # (d) given paths that are no walks, replan = 0
    *[dict(name=f"(d) {what}", map=["...", ".#.", "..."], agents=[[0, 0]], targets=[[0, 2]], on_target="finish",
           priority=None, replan=[0], paths=[[c] for c in given],
           actions=[[4], [4], [0]], path=[[[0, 1]], [[0, 2]], [[0, 2]]], arrival=[2], failed=[0], replanned=[1])
      for what, given in NOT_WALKS.items()],
    # ... and one that is a walk, if a roundabout one: it is kept as it stands
    dict(name="(d) a walk is kept", map=["...", ".#.", "..."], agents=[[0, 0]], targets=[[0, 2]], on_target="finish",
         priority=None, replan=None, paths=[[[1, 0]], [[2, 0]], [[2, 1]]],
         actions=[[2], [2], [4]], path=[[[1, 0]], [[2, 0]], [[2, 1]]], arrival=[-1], failed=[0], replanned=[0]),
    # (e) Everybody is kept -- the two even meet on (0,1) and then swap: conflicts among kept agents are not the
    # repair's business.  Nobody is served, every output is written.
    dict(name="(e) all kept", map=["..."], agents=[[0, 0], [0, 2]], targets=[[0, 2], [0, 0]], on_target="nothing",
         priority=[3, -3], replan=[0, 0], paths=[[[0, 1], [0, 1]], [[0, 2], [0, 0]]],
         actions=[[4, 3], [4, 3]], path=[[[0, 1], [0, 1]], [[0, 2], [0, 0]]],
         arrival=[2, 2], failed=[0, 0], replanned=[0, 0]),
    # (f) Agent 1 has finished and is not planned: its row of `paths` is ignored, it reserves nothing -- agent 0 walks
    # over its cell -- and keeps its cell in the output.
    dict(name="(f) an unplanned agent", map=["..."], agents=[[0, 0], [0, 1]], targets=[[0, 2], [0, 1]], active=[1, 0],
         on_target="finish", priority=None, replan=[1, 0], paths=[[[0, 0], JUNK], [[0, 0], [I32_MIN, I32_MIN]], [[0, 0], [9, 9]]],
         actions=[[4, 0], [4, 0], [0, 0]], path=[[[0, 1], [0, 1]], [[0, 2], [0, 1]], [[0, 2], [0, 1]]],
         arrival=[2, -1], failed=[0, 0], replanned=[1, 0],
         start=dict(agents=[[0, 0], [0, 2]], step=[0, 3])),
]

NAMES = ("actions", "path_xy", "arrival", "failed", "replanned")


def grid(rows):
    """The case's map as uint8 [H, W], 1 = obstacle."""
    return np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)


def active(case):
    return np.array(case.get("active", [1] * len(case["agents"])), dtype=bool)


def given(case):
    """The case's `paths` as int32 [K, A, 2]."""
    return np.array(case["paths"], dtype=np.int64).astype(np.int32)


def expected(case):
    """(actions int64 [K, A], path_xy int32 [K, A, 2], arrival, failed, replanned int32 [A])."""
    return (np.array(case["actions"], dtype=np.int64), np.array(case["path"], dtype=np.int32),
            np.array(case["arrival"], dtype=np.int32), np.array(case["failed"], dtype=np.int32),
            np.array(case["replanned"], dtype=np.int32))
