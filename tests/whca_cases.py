"""Hand-built cases of windowed cooperative A* (docs/SPEC.md S28), worked out on paper from the specification: each
names a map ('#' = obstacle), the agents' cells and targets, the priorities, the horizon, the on_target mode and the
four outputs.  tests/test_whca.py proves the CPU reference on them, tests/test_whca_gpu.py runs them on the engine."""
import numpy as np

CASES = [
    # Agent 0 (served first) walks through the corridor.  Agent 1 can only stay at step 1 ((0,1) is agent 0's), and at
    # step 2 its own cell is agent 0's and the move (0,2) -> (0,1) is the reverse of agent 0's: R_2 is empty.
    dict(name="corridor", map=["..."], agents=[[0, 0], [0, 2]], targets=[[0, 2], [0, 0]], priority=[1, 0], horizon=3,
         on_target="finish",
         actions=[[4, 0], [4, 0], [0, 0]],
         path=[[[0, 1], [0, 2]], [[0, 2], [0, 2]], [[0, 2], [0, 2]]],
         arrival=[2, -1], failed=[0, 1]),
    # The same under `nothing`: agent 0 ends on the cell of R_3 nearest to its target, the target, as early as it can.
    dict(name="corridor, nothing", map=["..."], agents=[[0, 0], [0, 2]], targets=[[0, 2], [0, 0]], priority=[1, 0],
         horizon=3, on_target="nothing",
         actions=[[4, 0], [4, 0], [0, 0]],
         path=[[[0, 1], [0, 2]], [[0, 2], [0, 2]], [[0, 2], [0, 2]]],
         arrival=[2, -1], failed=[0, 1]),
    # A crossing: agent 0 goes down through the centre, agent 1 has to cross it from left to right.  The centre is
    # agent 0's at step 1, so agent 1 waits one step (R_1 is its own cell alone) and then passes.
    dict(name="waiting", map=["#.#", "...", "#.#"], agents=[[0, 1], [1, 0]], targets=[[2, 1], [1, 2]], priority=None,
         horizon=4, on_target="finish",
         actions=[[2, 0], [2, 4], [0, 4], [0, 0]],
         path=[[[1, 1], [1, 0]], [[2, 1], [1, 1]], [[2, 1], [1, 2]], [[2, 1], [1, 2]]],
         arrival=[2, 3], failed=[0, 0]),
    # `finish`: agent 0 arrives on (0,2) at step 1 and reserves nothing afterwards, so agent 1 walks over that cell.
    dict(name="finish frees the cell", map=["...."], agents=[[0, 1], [0, 0]], targets=[[0, 2], [0, 3]], priority=[5, 0],
         horizon=4, on_target="finish",
         actions=[[4, 4], [0, 4], [0, 4], [0, 0]],
         path=[[[0, 2], [0, 1]], [[0, 2], [0, 2]], [[0, 2], [0, 3]], [[0, 2], [0, 3]]],
         arrival=[1, 3], failed=[0, 0]),
    # `nothing`: agent 0 keeps (0,2) for the whole window; agent 1 gets as near as it can, (0,1), at once, and waits.
    dict(name="nothing keeps the cell", map=["...."], agents=[[0, 1], [0, 0]], targets=[[0, 2], [0, 3]], priority=[5, 0],
         horizon=4, on_target="nothing",
         actions=[[4, 4], [0, 0], [0, 0], [0, 0]],
         path=[[[0, 2], [0, 1]], [[0, 2], [0, 1]], [[0, 2], [0, 1]], [[0, 2], [0, 1]]],
         arrival=[1, -1], failed=[0, 0]),
    # No path to the target: the Manhattan key keeps the agent where it is (R_3 holds (0,0) and (0,1)).
    dict(name="unreachable target", map=["..#."], agents=[[0, 0]], targets=[[0, 3]], priority=None, horizon=3,
         on_target="finish",
         actions=[[0], [0], [0]], path=[[[0, 0]], [[0, 0]], [[0, 0]]], arrival=[-1], failed=[0]),
    dict(name="unreachable target, nothing", map=["..#."], agents=[[0, 0]], targets=[[0, 3]], priority=None, horizon=3,
         on_target="nothing",
         actions=[[0], [0], [0]], path=[[[0, 0]], [[0, 0]], [[0, 0]]], arrival=[-1], failed=[0]),
    # Agents in opposite corners of a 3 x 4 map, horizon 6: the 13 x 13 box is larger than the map on every side.
    # Agent 0: the target enters R_5; read back with the lowest action first the last two moves are `down`, the first
    # three `right`.  Agent 1 cannot take the mirror image (it would meet agent 0 head-on in row 0 / column 3); its
    # backtrack prefers `up` over `left` as the last moves, which takes it along row 2 first: no cell and no move of
    # agent 0's is crossed, and it arrives at step 5 as well.
    dict(name="corners, box larger than the map", map=["....", "....", "...."], agents=[[0, 0], [2, 3]],
         targets=[[2, 3], [0, 0]], priority=None, horizon=6, on_target="finish",
         actions=[[4, 3], [4, 3], [4, 3], [2, 1], [2, 1], [0, 0]],
         path=[[[0, 1], [2, 2]], [[0, 2], [2, 1]], [[0, 3], [2, 0]], [[1, 3], [1, 0]], [[2, 3], [0, 0]], [[2, 3], [0, 0]]],
         arrival=[5, 5], failed=[0, 0]),
]


def grid(rows):
    """The case's map as uint8 [H, W], 1 = obstacle."""
    return np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)


def expected(case):
    """(actions int64 [K, A], path_xy int32 [K, A, 2], arrival int32 [A], failed int32 [A])."""
    return (np.array(case["actions"], dtype=np.int64), np.array(case["path"], dtype=np.int32),
            np.array(case["arrival"], dtype=np.int32), np.array(case["failed"], dtype=np.int32))
