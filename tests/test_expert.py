"""CPU: the shortest-path expert's reference (tests/expert_reference.py) on hand-built cases, and the C-ABI entry point
pgx_expert_actions is declared and exported."""
import os
import re

import numpy as np

from expert_reference import expert_env, expert_reference
from pogema_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(grid, agents, targets, active=None, agents_as_obstacles=False):
    obst = np.array([[c == "#" for c in row] for row in grid], dtype=np.uint8)
    active = np.ones(len(agents), dtype=bool) if active is None else np.asarray(active)
    return expert_env(obst, np.array(agents), np.array(targets), active, agents_as_obstacles)


def test_corridor():
    grid = ["#####",
            "....#",
            "###.#",
            "#...."]
    a, d = _one(grid, [(1, 0)], [(3, 4)])
    assert d.tolist() == [6] and a.tolist() == [4]      # right along the corridor
    a, d = _one(grid, [(3, 4)], [(1, 0)])
    assert d.tolist() == [6] and a.tolist() == [3]      # and back: left first
    a, d = _one(grid, [(2, 3)], [(1, 0)])
    assert d.tolist() == [4] and a.tolist() == [1]


def test_unreachable_target():
    grid = ["..#..",
            "..#..",
            "..#.."]
    a, d = _one(grid, [(0, 0)], [(2, 4)])
    assert d.tolist() == [-1] and a.tolist() == [0]


def test_tie_break_prefers_up_down_left_right():
    grid = ["...",
            "...",
            "..."]
    # target diagonal down-right: down (2) and right (4) both lower the distance; down wins
    a, d = _one(grid, [(0, 0)], [(1, 1)])
    assert d.tolist() == [2] and a.tolist() == [2]
    # target up-left: up (1) before left (3)
    a, d = _one(grid, [(2, 2)], [(0, 0)])
    assert d.tolist() == [4] and a.tolist() == [1]
    # target straight left
    a, d = _one(grid, [(1, 2)], [(1, 0)])
    assert d.tolist() == [2] and a.tolist() == [3]


def test_on_target_and_inactive():
    grid = ["...",
            "..."]
    a, d = _one(grid, [(0, 0), (1, 2), (0, 2)], [(0, 0), (0, 0), (1, 0)], active=[True, False, True])
    assert d.tolist() == [0, -1, 3]
    assert a.tolist() == [0, 0, 2]


def test_agents_as_obstacles():
    grid = [".....",
            ".###.",
            "....."]
    agents = [(0, 0), (0, 2), (2, 2)]
    targets = [(0, 4), (0, 2), (2, 0)]
    a, d = _one(grid, agents, targets)
    assert d.tolist() == [4, 0, 2] and a.tolist() == [4, 0, 3]
    # agent 1 blocks the top row and agent 2 the bottom row: agent 0 has no way round
    a, d = _one(grid, agents, targets, agents_as_obstacles=True)
    assert d.tolist() == [-1, 0, 2] and a.tolist() == [0, 0, 3]
    # an inactive agent does not block
    a, d = _one(grid, agents, targets, active=[True, False, True], agents_as_obstacles=True)
    assert d.tolist() == [4, -1, 2]
    # an agent standing on another one's target does not block that target, nor its own cell
    a, d = _one(grid, [(0, 0), (0, 1)], [(0, 1), (2, 4)], agents_as_obstacles=True)
    assert d.tolist() == [1, 5] and a.tolist() == [4, 4]


def test_batched_reference_matches_per_env():
    rng = np.random.default_rng(3)
    obst = (rng.random((3, 9, 7)) < 0.25).astype(np.uint8)
    agents = np.stack([np.stack(np.nonzero(obst[b] == 0), 1)[:4] for b in range(3)]).astype(np.int32)
    targets = np.stack([np.stack(np.nonzero(obst[b] == 0), 1)[-4:] for b in range(3)]).astype(np.int32)
    active = np.ones((3, 4), dtype=bool)
    a, d = expert_reference(obst, agents, targets, active)
    for b in range(3):
        ab, db = expert_env(obst[b], agents[b], targets[b], active[b])
        assert (a[b] == ab).all() and (d[b] == db).all()


def test_header_declares_and_library_exports_expert(engine_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pogema_amd.h")).read(), flags=re.S)
    assert re.search(r"int\s+pgx_expert_actions\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+flags\s*,\s*void\s*\*\s*actions"
                     r"\s*,\s*int32_t\s+action_dtype\s*,\s*int32_t\s*\*\s*distance\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert "pgx_expert_actions" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_expert_actions")
    # refused without a handle, through the usual error path (no device needed)
    assert engine_lib.pgx_expert_actions(None, 0, None, 2, None, None) == -1
    assert b"pgx_expert_actions" in engine_lib.pgx_last_error()
