"""CPU: the reference of the move outcomes (tests/move_outcomes_reference.py, docs/SPEC.md S17).  Its move phase equals
PogemaOracle.move_agents on random small states under every collision system; the table's properties hold (every stayed
mover is explained, FOLLOW never occurs under `soft`, the counts sum to the active agents); hand-written cases pin every
code and its blocker; the Python names of the codes are the header's."""
import os
import re

import numpy as np
import pytest

from move_outcomes_reference import (CONTESTED, FOLLOW, MOVED, NUM_OUTCOMES, OBSTACLE, OCCUPIED, STAY, SWAP,
                                     move_outcomes_one, move_outcomes_reference, move_phase)
from util import PogemaOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYSTEMS = [("priority", "lowest_index"), ("block_both", "lowest_index"), ("soft", "lowest_index"), ("soft", "all_stay")]


def _instance(rng):
    """A random small map with distinct start cells; targets are any free cells."""
    while True:
        H, W = int(rng.integers(3, 7)), int(rng.integers(3, 7))
        obst = (rng.random((H, W)) < 0.15).astype(np.uint8)
        free = np.argwhere(obst == 0)
        if len(free) >= 2:
            break
    A = int(rng.integers(2, min(13, len(free)) + 1))
    starts = free[rng.permutation(len(free))[:A]]
    targets = free[rng.integers(0, len(free), size=A)]
    return obst, starts, targets


@pytest.mark.parametrize("collision,soft_vertex", SYSTEMS)
def test_move_phase_equals_the_oracle_and_the_table_holds(collision, soft_vertex):
    rng = np.random.default_rng(len(collision) * 7 + len(soft_vertex))
    seen = set()
    shared_states = hidden_states = 0
    for episode in range(150):
        obst, starts, targets = _instance(rng)
        A = len(starts)
        env = PogemaOracle(obst, starts, targets, obs_radius=2, collision_system=collision, on_target="finish",
                           max_episode_steps=1000, auto_reset=False, soft_vertex_rule=soft_vertex)
        g = env.grid
        for i in range(A):
            if rng.random() < 0.15:
                g.hide_agent(i)
        for step in range(12):
            cur = g.unpadded_xy(g.positions_xy)
            active = [bool(g.is_active[i]) for i in range(A)]
            actions = rng.integers(0, 5, size=A)
            actions[rng.random(A) < 0.1] = rng.choice([-1, 5, 7, 100])
            nxt, outcome, blocker, counts = move_outcomes_one(obst.tolist(), cur, active, actions, collision, soft_vertex)
            env.step([int(a) for a in actions])
            what = f"{collision}/{soft_vertex} episode {episode} step {step}"
            assert nxt == g.unpadded_xy(g.positions_xy), what
            cells = [cur[i] for i in range(A) if active[i]]
            shared = len(set(cells)) != len(cells)
            shared_states += shared
            hidden_states += not all(active)
            assert sum(counts) == sum(active) and len(counts) == NUM_OUTCOMES, what
            for i in range(A):
                mover = active[i] and 1 <= actions[i] <= 4
                if not mover:
                    assert outcome[i] == STAY and blocker[i] == -1 and nxt[i] == cur[i], what
                elif nxt[i] != cur[i]:
                    assert outcome[i] == MOVED and blocker[i] == -1, what
                else:
                    assert outcome[i] >= OBSTACLE, what
                    assert (blocker[i] >= 0) == (outcome[i] >= SWAP) or (shared and outcome[i] == CONTESTED), what
                    if outcome[i] >= SWAP and blocker[i] >= 0:
                        assert blocker[i] != i and active[blocker[i]], what
                if active[i]:
                    seen.add(outcome[i])
            if collision == "soft":
                assert FOLLOW not in outcome, what
    assert hidden_states > 100
    want = {STAY, MOVED, OBSTACLE, SWAP, OCCUPIED, CONTESTED} | ({FOLLOW} if collision != "soft" else set())
    assert seen == want, (collision, sorted(seen))
    if collision != "soft":
        assert shared_states == 0      # `priority` and `block_both` keep agents on distinct cells


OPEN = np.zeros((5, 5), dtype=np.uint8)
WALL = OPEN.copy()
WALL[2, 2] = 1
ALL = ("priority", "block_both", "soft", "all_stay")
# name, map, cells, active, actions, {systems: (outcome, blocker)}; MOVES = noop, up, down, left, right
CASES = [
    ("head-on swap", OPEN, [(2, 1), (2, 2)], [1, 1], [4, 3], {ALL: ([SWAP, SWAP], [1, 0])}),
    ("chain behind a stayer", OPEN, [(2, 3), (2, 2), (2, 1)], [1, 1, 1], [0, 4, 4],
     {ALL: ([STAY, OCCUPIED, OCCUPIED], [-1, 0, 1])}),
    ("chain behind an agent facing the ring", OPEN, [(0, 2), (1, 2)], [1, 1], [1, 1], {ALL: ([OBSTACLE, OCCUPIED], [-1, 0])}),
    ("obstacle inside the map and the ring's corner", WALL, [(2, 1), (0, 0)], [1, 1], [4, 3],
     {ALL: ([OBSTACLE, OBSTACLE], [-1, -1])}),
    ("three-way contest", OPEN, [(1, 2), (2, 1), (3, 2)], [1, 1, 1], [2, 4, 1],
     {("priority", "soft"): ([MOVED, CONTESTED, CONTESTED], [-1, 0, 0]),
      ("block_both", "all_stay"): ([CONTESTED, CONTESTED, CONTESTED], [1, 0, 0])}),
    ("rotation cycle", OPEN, [(1, 1), (1, 2), (2, 2), (2, 1)], [1, 1, 1, 1], [4, 2, 3, 1],
     {("soft", "all_stay"): ([MOVED] * 4, [-1] * 4), ("priority", "block_both"): ([OCCUPIED] * 4, [1, 2, 3, 0])}),
    ("following a lower index", OPEN, [(2, 2), (2, 1)], [1, 1], [4, 4],
     {("priority", "soft", "all_stay"): ([MOVED, MOVED], [-1, -1]), ("block_both",): ([MOVED, FOLLOW], [-1, 0])}),
    ("following a higher index", OPEN, [(2, 1), (2, 2)], [1, 1], [4, 4],
     {("soft", "all_stay"): ([MOVED, MOVED], [-1, -1]), ("priority", "block_both"): ([FOLLOW, MOVED], [1, -1])}),
    ("a contest for a cell its agent leaves", OPEN, [(2, 2), (2, 1), (1, 2)], [1, 1, 1], [4, 4, 2],
     {("priority", "soft"): ([MOVED, MOVED, CONTESTED], [-1, -1, 1]),
      ("block_both", "all_stay"): ([MOVED, CONTESTED, CONTESTED], [-1, 2, 1])}),
    ("out-of-range actions", OPEN, [(2, 2), (2, 1), (4, 4), (0, 0)], [1, 1, 1, 1], [5, 4, -1, 100],
     {ALL: ([STAY, OCCUPIED, STAY, STAY], [-1, 0, -1, -1])}),
    ("an inactive agent on a wanted cell blocks nothing", OPEN, [(2, 2), (2, 1)], [0, 1], [3, 4],
     {ALL: ([STAY, MOVED], [-1, -1])}),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_written_cases(case):
    name, obst, cells, active, actions, expected = case
    checked = []
    for systems, (outcome, blocker) in expected.items():
        for system in systems:
            collision, soft_vertex = ("soft", "all_stay") if system == "all_stay" else (system, "lowest_index")
            nxt, got, who, counts = move_outcomes_one(obst.tolist(), cells, active, actions, collision, soft_vertex)
            assert (got, who) == (outcome, blocker), (name, system)
            for i, c in enumerate(cells):
                a = actions[i] if 0 <= actions[i] <= 4 else 0
                d = (c[0] + ((a == 2) - (a == 1)), c[1] + ((a == 4) - (a == 3)))
                assert nxt[i] == (d if got[i] == MOVED else c), (name, system, i)
            assert counts == [sum(1 for i, c in enumerate(got) if active[i] and c == k) for k in range(NUM_OUTCOMES)]
            checked.append(system)
    assert sorted(checked) == sorted(ALL), name


def test_every_code_has_a_hand_written_case_under_every_system_that_produces_it():
    seen = {s: set() for s in ALL}
    for _, _, _, _, _, expected in CASES:
        for systems, (outcome, _) in expected.items():
            for s in systems:
                seen[s] |= set(outcome)
    for s in ALL:
        assert seen[s] == set(range(NUM_OUTCOMES)) - ({FOLLOW} if s in ("soft", "all_stay") else set()), s


def test_batched_reference_stacks_the_envs():
    maps = np.stack([OPEN, WALL])
    pos = np.array([[(2, 1), (2, 2)], [(2, 1), (0, 0)]], dtype=np.int32)
    active = np.ones((2, 2), dtype=bool)
    actions = np.array([[4, 3], [4, 3]])
    next_xy, outcome, blocker, counts = move_outcomes_reference(maps, pos, active, actions, "priority")
    assert next_xy.dtype == np.int32 and outcome.dtype == np.uint8 and blocker.dtype == np.int32 and counts.dtype == np.int32
    assert np.array_equal(next_xy, pos)
    assert outcome.tolist() == [[SWAP, SWAP], [OBSTACLE, OBSTACLE]] and blocker.tolist() == [[1, 0], [-1, -1]]
    assert counts.tolist() == [[0, 0, 0, 2, 0, 0, 0], [0, 0, 2, 0, 0, 0, 0]]
    assert move_phase(OPEN.tolist(), [(2, 1)], [True], [4], "soft") == [(2, 2)]


def test_python_names_are_the_headers_constants():
    import pogema_amd
    from pogema_amd import _lib
    text = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    codes = {name: int(value) for name, value in re.findall(r"#define PGX_OUTCOME_([A-Z]+) (\d+)", text)}
    assert codes == {name: k for k, name in enumerate(_lib.OUTCOMES)}
    assert int(re.search(r"#define PGX_NUM_OUTCOMES (\d+)", text).group(1)) == _lib.NUM_OUTCOMES == len(_lib.OUTCOMES) == NUM_OUTCOMES
    assert pogema_amd.OUTCOMES is _lib.OUTCOMES
    assert codes == dict(STAY=STAY, MOVED=MOVED, OBSTACLE=OBSTACLE, SWAP=SWAP, OCCUPIED=OCCUPIED, FOLLOW=FOLLOW,
                         CONTESTED=CONTESTED)            # ... and the reference's
    assert "pgx_move_outcomes" in _lib.EXPORTED_SYMBOLS
