"""CPU: the cost-to-go reference (tests/cost_to_go_reference.py) on hand-built maps, its vectorised variant against the
queue BFS, and the C-ABI of the feature: pgx_cost_to_go / pgx_cost_to_go_bytes / pgx_cost_to_go_builds are declared and
exported, and the cache size follows the documented formula (no device needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cost_to_go_reference import cost_to_go_env, cost_to_go_reference, fields_packed, window
from expert_reference import bfs_from, expert_env
from pogema_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(rows):
    return np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)


def test_corridor_window():
    obst = _grid(["#####",
                  "....#",
                  "###.#",
                  "#...."])
    w = cost_to_go_env(obst, [(1, 0)], [(3, 4)], [True], r=1)[0]
    # rows 0..2, cols -1..1 around (1, 0): column -1 is outside the map
    assert w.tolist() == [[-1, -1, -1],
                          [-1, 6, 5],
                          [-1, -1, -1]]
    w = cost_to_go_env(obst, [(2, 3)], [(3, 4)], [True], r=2)[0]
    # columns 1..5: column 5 is outside the map, row 4 too
    assert w.tolist() == [[-1, -1, -1, -1, -1],
                          [5, 4, 3, -1, -1],
                          [-1, -1, 2, -1, -1],
                          [3, 2, 1, 0, -1],
                          [-1, -1, -1, -1, -1]]


def test_unreachable_pocket_and_inactive():
    obst = _grid(["..#..",
                  "..#..",
                  "..#.."])
    w = cost_to_go_env(obst, [(1, 1), (1, 4)], [(1, 0), (1, 0)], [True, False], r=2)
    assert w[0].tolist() == [[-1, -1, -1, -1, -1],
                             [-1, 1, 2, -1, -1],
                             [-1, 0, 1, -1, -1],
                             [-1, 1, 2, -1, -1],
                             [-1, -1, -1, -1, -1]]
    assert (w[1] == -1).all()
    # the right-hand pocket cannot reach a target on the left
    w = cost_to_go_env(obst, [(1, 4)], [(1, 0)], [True], r=1)[0]
    assert (w == -1).all()


def test_target_on_an_obstacle_is_all_unreachable():
    obst = _grid(["...",
                  ".#.",
                  "..."])
    w = cost_to_go_env(obst, [(0, 0)], [(1, 1)], [True], r=2)[0]
    assert (w == -1).all()
    f = fields_packed(obst[None], [(1, 1)])[0]
    assert (f == -1).all()


def test_windows_over_every_edge():
    rng = np.random.default_rng(5)
    obst = (rng.random((6, 7)) < 0.2).astype(np.uint8)
    obst[3, 3] = 0
    field = bfs_from(obst != 0, 3, 3)
    r = 4
    for x, y in [(0, 0), (0, 6), (5, 0), (5, 6), (2, 3)]:
        w = window(field, x, y, r)
        for u in range(2 * r + 1):
            for v in range(2 * r + 1):
                cx, cy = x - r + u, y - r + v
                want = field[cx, cy] if 0 <= cx < 6 and 0 <= cy < 7 else -1
                assert w[u, v] == want, (x, y, u, v)


def test_centre_equals_expert_distance():
    rng = np.random.default_rng(7)
    obst = (rng.random((12, 9)) < 0.3).astype(np.uint8)
    free = np.argwhere(obst == 0)
    agents = free[rng.choice(len(free), 6, replace=False)]
    targets = free[rng.choice(len(free), 6, replace=False)]
    active = np.array([1, 1, 0, 1, 1, 1], dtype=bool)
    r = 3
    w = cost_to_go_env(obst, agents, targets, active, r)
    _, d = expert_env(obst, agents, targets, active)
    assert (w[:, r, r] == d).all()
    assert (w[~active] == -1).all()


def test_packed_variant_matches_queue_bfs():
    rng = np.random.default_rng(11)
    for H, W in ((1, 5), (2, 2), (9, 33), (31, 64), (64, 64)):
        obst = (rng.random((20, H, W)) < 0.3).astype(np.uint8)
        t = np.stack([rng.integers(0, H, 20), rng.integers(0, W, 20)], 1)
        f = fields_packed(obst, t)
        for k in range(20):
            assert np.array_equal(f[k], bfs_from(obst[k] != 0, *t[k])), (H, W, k)


def test_batched_reference_matches_per_env():
    rng = np.random.default_rng(3)
    obst = (rng.random((3, 9, 7)) < 0.25).astype(np.uint8)
    agents = np.stack([np.stack(np.nonzero(obst[b] == 0), 1)[:4] for b in range(3)]).astype(np.int32)
    targets = np.stack([np.stack(np.nonzero(obst[b] == 0), 1)[-4:] for b in range(3)]).astype(np.int32)
    active = np.array([[1, 1, 1, 1], [1, 0, 1, 1], [0, 0, 0, 1]], dtype=bool)
    got = cost_to_go_reference(obst, agents, targets, active, r=2)
    for b in range(3):
        assert np.array_equal(got[b], cost_to_go_env(obst[b], agents[b], targets[b], active[b], r=2))


def test_header_declares_and_library_exports(engine_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pogema_amd.h")).read(), flags=re.S)
    assert re.search(r"int\s+pgx_cost_to_go\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+flags\s*,\s*int32_t\s*\*\s*out"
                     r"\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert re.search(r"int64_t\s+pgx_cost_to_go_bytes\s*\(\s*const\s+pgx_config\s*\*\s*cfg\s*\)", text)
    assert re.search(r"int64_t\s+pgx_cost_to_go_builds\s*\(\s*pgx_env\s*\*\s*env\s*,\s*void\s*\*\s*stream\s*\)", text)
    for name in ("pgx_cost_to_go", "pgx_cost_to_go_bytes", "pgx_cost_to_go_builds"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(engine_lib, name)
    # refused without a handle, through the usual error path (no device needed)
    assert engine_lib.pgx_cost_to_go(None, 0, None, None) == -1
    assert b"pgx_cost_to_go" in engine_lib.pgx_last_error()
    assert engine_lib.pgx_cost_to_go_builds(None, None) == -1
    assert b"pgx_cost_to_go_builds" in engine_lib.pgx_last_error()
    assert engine_lib.pgx_cost_to_go_bytes(None) == -1


def _cfg(batch, H, W, A, r):
    return _lib.PgxConfig(batch=batch, height=H, width=W, num_agents=A, obs_radius=r, max_episode_steps=64,
                          abi_version=_lib.PGX_ABI_VERSION)


def _formula(batch, H, W, A):
    cell = 2 if H * W <= 65536 else 4
    fields = batch * A * H * W * cell
    return 16 + (fields + 15) // 16 * 16 + 4 * batch * A + 4 * batch * H * ((W + 31) // 32)


@pytest.mark.parametrize("batch,H,W,A,r", [(1024, 16, 16, 8, 5), (8192, 32, 32, 16, 5), (8192, 64, 64, 64, 5),
                                           (4096, 256, 256, 256, 7), (1, 256, 256, 2, 1), (1, 257, 256, 2, 1),
                                           (1, 256, 257, 2, 1), (2, 1024, 600, 3, 2), (1, 1024, 1024, 2, 2),
                                           (3, 5, 7, 3, 1), (1, 2, 2, 1, 1)])
def test_cache_bytes_formula(engine_lib, batch, H, W, A, r):
    assert engine_lib.pgx_cost_to_go_bytes(C.byref(_cfg(batch, H, W, A, r))) == _formula(batch, H, W, A)


def test_cache_bytes_cell_width_switch(engine_lib):
    """2-byte cells up to 65536 cells per map, 4-byte cells above."""
    at = engine_lib.pgx_cost_to_go_bytes(C.byref(_cfg(1, 256, 256, 1, 1)))
    above = engine_lib.pgx_cost_to_go_bytes(C.byref(_cfg(1, 257, 256, 1, 1)))
    assert at == 16 + 2 * 65536 + 4 + 4 * 256 * 8
    assert above == 16 + 4 * 257 * 256 + 4 + 4 * 257 * 8
    # scale of the documented configurations: configs[1] ~4 MB, configs[2] ~4.3 GB, configs[4] ~137 GB
    assert 4.0e6 < engine_lib.pgx_cost_to_go_bytes(C.byref(_cfg(1024, 16, 16, 8, 5))) < 4.3e6
    assert 4.2e9 < engine_lib.pgx_cost_to_go_bytes(C.byref(_cfg(8192, 64, 64, 64, 5))) < 4.4e9
    assert 1.3e11 < engine_lib.pgx_cost_to_go_bytes(C.byref(_cfg(4096, 256, 256, 256, 7))) < 1.4e11


def test_cache_bytes_refuses_what_check_config_refuses(engine_lib):
    cfg = _cfg(4, 16, 16, 8, 16)                   # obs_radius above the engine's limit
    assert engine_lib.pgx_check_config(C.byref(cfg)) == -1
    assert engine_lib.pgx_cost_to_go_bytes(C.byref(cfg)) == -1
