"""CPU: the direction-to-goal reference (tests/goal_directions_reference.py, docs/SPEC.md S14) on cases worked by hand,
against a brute-force per-cell statement of the definition, and the identities that tie it to the cost-to-go windows;
the C-ABI of the feature: pgx_goal_directions is declared and exported, and its argument checks need no device."""
import ctypes as C
import os
import re

import numpy as np

from cost_to_go_reference import cost_to_go_reference
from expert_reference import MOVES, bfs_from, expert_env
from goal_directions_reference import bits_from_tiles, goal_directions_env, goal_directions_reference, halo_tile, planes
from pogema_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP, DOWN, LEFT, RIGHT = 1, 2, 4, 8   # bit a-1 of move a


def _grid(rows):
    return np.array([[c == "#" for c in row] for row in rows], dtype=np.uint8)


def test_open_3x3():
    obst = np.zeros((3, 3), dtype=np.uint8)
    # agent in the middle, target in the top-left corner: the window is the map
    d = goal_directions_env(obst, [(1, 1)], [(0, 0)], [True], r=1)[0]
    assert d.tolist() == [[0, LEFT, LEFT],
                          [UP, UP | LEFT, UP | LEFT],
                          [UP, UP | LEFT, UP | LEFT]]
    # r = 2: one ring of cells outside the map around it, all zero
    d = goal_directions_env(obst, [(1, 1)], [(0, 0)], [True], r=2)[0]
    assert (d[0] == 0).all() and (d[-1] == 0).all() and (d[:, 0] == 0).all() and (d[:, -1] == 0).all()
    assert d[1:4, 1:4].tolist() == [[0, LEFT, LEFT], [UP, UP | LEFT, UP | LEFT], [UP, UP | LEFT, UP | LEFT]]


def test_wall_makes_two_moves_equally_good():
    obst = _grid([".....",
                  "..#..",
                  "....."])
    # from (1, 1) to (1, 3) the wall at (1, 2) blocks the straight move: up and down are equally good
    d = goal_directions_env(obst, [(1, 1)], [(1, 3)], [True], r=1)[0]
    assert d[1, 1] == UP | DOWN
    assert d.tolist() == [[RIGHT, RIGHT, RIGHT],
                          [UP | DOWN | RIGHT, UP | DOWN, 0],
                          [RIGHT, RIGHT, RIGHT]]


def test_agent_in_a_map_corner_and_the_window_edge():
    obst = np.zeros((4, 6), dtype=np.uint8)
    # agent in the corner (0, 0), target far to the right at (0, 5): rows 0..1 and columns 0..1 of the map are in the window
    d = goal_directions_env(obst, [(0, 0)], [(0, 5)], [True], r=1)[0]
    assert d.tolist() == [[0, 0, 0],
                          [0, RIGHT, RIGHT],
                          [0, UP | RIGHT, UP | RIGHT]]
    # the edge column's RIGHT bit rests on column 2, which the window does not hold: a window-only rebuild from
    # cost_to_go() (the neighbour outside the window unknown, taken as undefined) loses exactly these bits
    ctg = cost_to_go_reference(obst[None], [[(0, 0)]], [[(0, 5)]], [[True]], 1)[0, 0]
    tile = np.full((5, 5), -1)
    tile[1:4, 1:4] = ctg
    inner = bits_from_tiles(tile[None])[0]
    assert inner[1, 2] == 0 and d[1, 2] == RIGHT and inner[2, 2] == UP and d[2, 2] == UP | RIGHT
    assert np.array_equal(inner[:, :2], d[:, :2])


def test_obstacle_target_and_inactive_agent():
    obst = _grid(["...",
                  ".#.",
                  "..."])
    d = goal_directions_env(obst, [(0, 0), (2, 2)], [(1, 1), (0, 0)], [True, False], r=2)
    assert (d == 0).all()
    d = goal_directions_reference(obst[None], [[(0, 0), (2, 2)]], [[(1, 1), (0, 0)]], [[True, False]], r=2)
    assert (d == 0).all()


def test_unreachable_component():
    obst = _grid(["..#..",
                  "..#..",
                  "..#.."])
    # target on the left; the agent on the right sees both halves: only the left one points anywhere
    d = goal_directions_env(obst, [(1, 3)], [(1, 0)], [True], r=2)[0]
    # window columns are map columns 1..5 (5 is outside), rows -1..3 (first and last outside)
    assert d.tolist() == [[0, 0, 0, 0, 0],
                          [LEFT | DOWN, 0, 0, 0, 0],
                          [LEFT, 0, 0, 0, 0],
                          [LEFT | UP, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0]]


def _brute(obst, ax, ay, tx, ty, r):
    """The definition of docs/SPEC.md S14, cell by cell."""
    H, W = obst.shape
    D = bfs_from(obst != 0, tx, ty)

    def defined(x, y):
        return 0 <= x < H and 0 <= y < W and D[x, y] >= 0

    w = 2 * r + 1
    out = np.zeros((4, w, w), dtype=np.uint8)
    for u in range(w):
        for v in range(w):
            cx, cy = ax - r + u, ay - r + v
            for a in range(1, 5):
                nx, ny = cx + MOVES[a][0], cy + MOVES[a][1]
                if defined(cx, cy) and defined(nx, ny) and D[nx, ny] < D[cx, cy]:
                    out[a - 1, u, v] = 1
    return out


def test_reference_matches_the_brute_force_definition():
    rng = np.random.default_rng(14)
    for H, W, r in ((2, 2, 1), (5, 9, 2), (9, 5, 3), (12, 12, 5), (7, 70, 2)):
        B, A = 3, 5
        obst = (rng.random((B, H, W)) < 0.25).astype(np.uint8)
        agents = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)
        targets = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)  # obstacle targets included
        active = rng.random((B, A)) < 0.8
        got = goal_directions_reference(obst, agents, targets, active, r)
        assert got.max() < 16
        for b in range(B):
            assert np.array_equal(got[b], goal_directions_env(obst[b], agents[b], targets[b], active[b], r))
            for i in range(A):
                want = _brute(obst[b], *agents[b, i], *targets[b, i], r)
                assert np.array_equal(planes(got[b, i]), want if active[b, i] else np.zeros_like(want)), (H, W, b, i)
    only = goal_directions_reference(obst, agents, targets, active, r, envs=[1])
    assert np.array_equal(only[1], got[1]) and (only[[0, 2]] == 0).all()


def test_identities_with_cost_to_go_windows():
    rng = np.random.default_rng(15)
    B, H, W, A, r = 4, 14, 11, 6, 3
    obst = (rng.random((B, H, W)) < 0.3).astype(np.uint8)
    free = [np.argwhere(o == 0) for o in obst]
    agents = np.stack([f[rng.choice(len(f), A, replace=False)] for f in free])
    targets = np.stack([f[rng.choice(len(f), A, replace=False)] for f in free])
    active = rng.random((B, A)) < 0.8
    bits = goal_directions_reference(obst, agents, targets, active, r)
    ctg = cost_to_go_reference(obst, agents, targets, active, r)
    # cells with a positive cost-to-go have a way down, the others (target, -1) have none
    assert ((bits != 0) == (ctg > 0)).all()
    # the interior of the window follows from the cost-to-go window alone
    for a, (dx, dy) in enumerate(MOVES[1:]):
        c = ctg[:, :, 1:-1, 1:-1]
        n = ctg[:, :, 1 + dx:2 * r + dx, 1 + dy:2 * r + dy]
        assert np.array_equal((bits[:, :, 1:-1, 1:-1] >> a) & 1, ((c >= 0) & (n >= 0) & (n < c)).astype(np.uint8))
    # the lowest bit at the centre is the expert's action
    for b in range(B):
        act, _ = expert_env(obst[b], agents[b], targets[b], active[b])
        centre = bits[b, :, r, r].astype(np.int64)
        lowest = np.where(centre != 0, np.log2(np.maximum(centre & -centre, 1)).astype(np.int64) + 1, 0)
        assert np.array_equal(lowest, act)


def test_halo_tile_over_every_edge():
    field = np.arange(6 * 7).reshape(6, 7)
    for x, y in [(0, 0), (0, 6), (5, 0), (5, 6), (2, 3)]:
        t = halo_tile(field, x, y, 2)
        assert t.shape == (7, 7)
        for u in range(7):
            for v in range(7):
                cx, cy = x - 3 + u, y - 3 + v
                assert t[u, v] == (field[cx, cy] if 0 <= cx < 6 and 0 <= cy < 7 else -1)


def test_header_declares_and_library_exports(engine_lib):
    src = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+pgx_goal_directions\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+flags\s*,\s*void\s*\*\s*out\s*,"
                     r"\s*int32_t\s+format\s*,\s*void\s*\*\s*stream\s*\)", text)
    for name, code in (("F32", 0), ("U8", 1), ("BITS", 2)):
        assert re.search(rf"#define\s+PGX_DIRECTIONS_{name}\s+{code}\b", text)
    assert _lib.DIRECTIONS_FORMATS == {"float32": 0, "uint8": 1, "bits": 2}
    assert "pgx_goal_directions" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_goal_directions")


def test_invalid_arguments_need_no_device(engine_lib):
    """PGX_E_INVALID for non-zero flags, a NULL out, an unknown format and a misaligned float32 out: checked before the
    handle, so a NULL handle is never reached (a well-formed call on a NULL handle is refused too)."""
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf)
    base += -base % 16
    call = engine_lib.pgx_goal_directions

    def refused(needle, *args):
        assert call(*args) == -1
        assert needle in engine_lib.pgx_last_error().decode()

    refused("out is null", None, 0, None, 0, None)
    refused("flags", None, 1, base, 0, None)
    for fmt in (-1, 3, 99):
        refused("format", None, 0, base, fmt, None)
    for off in (1, 2, 3):
        refused("4-byte aligned", None, 0, base + off, 0, None)
    # one-byte formats take any address: the refusal that remains is the NULL handle's
    for fmt in (1, 2):
        refused("null handle", None, 0, base + 1, fmt, None)
    refused("null handle", None, 0, base, 0, None)
