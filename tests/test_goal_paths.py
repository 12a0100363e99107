"""CPU: the path-to-goal reference (tests/goal_paths_reference.py, docs/SPEC.md S22) on the hand-built cases of tests/
goal_paths_cases.py, against an independent brute force that descends the BFS field directly, and the identities that
tie it to the cost-to-go windows; the C-ABI of the feature: pgx_goal_paths is declared and exported, and its argument
checks need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cost_to_go_reference import cost_to_go_reference
from expert_reference import MOVES, bfs_from
from goal_paths_cases import CASES, expected, grid
from goal_paths_reference import goal_paths_reference, rows
from pogema_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference(case):
    return goal_paths_reference(grid(case["map"])[None], [case["agents_xy"]], [case["targets_xy"]], [case["is_active"]],
                                case["r"], steps=case["steps"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_built_cases(case):
    planes, subgoal, length = (v[0] for v in _reference(case))
    want_planes, want_subgoal, want_length = expected(case)
    assert planes.tolist() == want_planes.tolist()
    assert subgoal.tolist() == want_subgoal.tolist() and subgoal.dtype == np.int8
    assert length.tolist() == want_length.tolist() and length.dtype == np.int32
    assert (planes.sum((-1, -2)) == length).all() and (planes[:, case["r"], case["r"]] == 0).all()


def _end_kind(case, i, length, subgoal):
    """What ended agent i's prefix, from the outputs and the definitions alone."""
    if length == 0:
        return None
    x, y = case["agents_xy"][i]
    if [x + int(subgoal[0]), y + int(subgoal[1])] == list(case["targets_xy"][i]):
        return "target"
    return "cap" if length == case["steps"] else "edge"


def test_cases_cover_every_end_and_a_long_path():
    seen, longest = set(), 0
    for case in CASES:
        _, subgoal, length = (v[0] for v in _reference(case))
        for i, end in enumerate(case["end"]):
            assert _end_kind(case, i, int(length[i]), subgoal[i]) == end, case["name"]
            seen.add(end)
            longest = max(longest, int(length[i]) - 2 * case["r"])
    assert seen == {None, "target", "edge", "cap"}
    assert longest > 0, "no path is longer than 2r: nothing winds inside a window"


def _brute(obst, ax, ay, tx, ty, r, steps):
    """The definition of docs/SPEC.md S22 on the BFS field itself."""
    H, W = obst.shape
    D = bfs_from(obst != 0, tx, ty)
    w = 2 * r + 1
    cap = w * w - 1 if steps is None else min(steps, w * w - 1)
    plane = np.zeros((w, w), dtype=np.uint8)
    x, y, n = ax, ay, 0
    while n < cap and D[x, y] >= 0:
        for dx, dy in MOVES[1:]:
            nx, ny = x + dx, y + dy
            if 0 <= nx < H and 0 <= ny < W and 0 <= D[nx, ny] < D[x, y]:
                break
        else:
            break                            # the target: nothing is closer
        if abs(nx - ax) > r or abs(ny - ay) > r:
            break                            # the next cell lies outside the window
        x, y, n = nx, ny, n + 1
        plane[x - ax + r, y - ay + r] = 1
    return plane, (x - ax, y - ay), n


def test_reference_matches_the_brute_force_definition():
    rng = np.random.default_rng(22)
    ends = set()
    for H, W, r, steps in ((2, 2, 1, None), (5, 9, 2, None), (9, 5, 3, 4), (12, 12, 5, None), (7, 70, 2, 1), (16, 16, 1, 3)):
        B, A = 3, 5
        obst = (rng.random((B, H, W)) < 0.25).astype(np.uint8)
        agents = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)
        targets = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)  # obstacle targets included
        obst[np.arange(B)[:, None], agents[..., 0], agents[..., 1]] = 0                   # agents stand on free cells
        active = rng.random((B, A)) < 0.8
        planes, subgoal, length = goal_paths_reference(obst, agents, targets, active, r, steps=steps)
        ctg = cost_to_go_reference(obst, agents, targets, active, r)[:, :, r, r]
        for b in range(B):
            for i in range(A):
                if active[b, i]:
                    want = _brute(obst[b], *agents[b, i], *targets[b, i], r, steps)
                else:
                    want = (np.zeros((2 * r + 1, 2 * r + 1), np.uint8), (0, 0), 0)
                assert np.array_equal(planes[b, i], want[0]) and tuple(subgoal[b, i]) == want[1] and length[b, i] == want[2]
        # length <= the cost at the centre, equal iff the prefix ended on the target
        on = length > 0
        assert (length[on] <= ctg[on]).all() and (length[~on] == 0).all()
        hit = ((agents + subgoal) == targets).all(-1) & on
        assert np.array_equal(hit, (length == ctg) & on)
        ends |= {"target"} if hit.any() else set()
        ends |= {"edge"} if (on & ~hit & (length != (steps or -1))).any() else set()
    assert ends == {"target", "edge"}
    only = goal_paths_reference(obst, agents, targets, active, r, steps=steps, envs=[1])
    assert all(np.array_equal(o[1], g[1]) and not o[[0, 2]].any() for o, g in zip(only, (planes, subgoal, length)))


def test_rows_pack_the_planes():
    planes, _, _ = _reference(CASES[-2])     # the winding corridor
    assert rows(planes)[0, 0].tolist() == [0b11111, 0b10001, 0b11001, 0b00001, 0b11111]
    assert rows(planes).dtype == np.int32
    full = np.ones((31, 31), dtype=np.uint8)
    assert (rows(full) == 2**31 - 1).all(), "W <= 31: the sign bit is never set"


def test_header_declares_and_library_exports(engine_lib):
    src = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+pgx_goal_paths\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+flags\s*,\s*int32_t\s+steps\s*,"
                     r"\s*int32_t\s+format\s*,\s*void\s*\*\s*planes\s*,\s*int8_t\s*\*\s*subgoal\s*,\s*int32_t\s*\*\s*length\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", text)
    for name, code in (("F32", 0), ("U8", 1), ("ROWS", 2)):
        assert re.search(rf"#define\s+PGX_PATHS_{name}\s+{code}\b", text)
    assert re.search(r"#define\s+PGX_MAX_PATH_STEPS\s+960\b", text)
    assert _lib.PATHS_FORMATS == {"float32": 0, "uint8": 1, "rows": 2}
    assert _lib.MAX_PATH_STEPS == 960 == (2 * _lib.MAX_OBS_RADIUS + 1) ** 2 - 1
    assert "pgx_goal_paths" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_goal_paths")


def test_invalid_arguments_need_no_device(engine_lib):
    """PGX_E_INVALID when all three outputs are NULL, for non-zero flags, an unknown format, steps outside 0..960, a
    misaligned float32 or rows `planes` and a misaligned `length`: checked before the handle, so a NULL handle is never
    reached (a well-formed call on a NULL handle is refused too)."""
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf)
    base += -base % 16
    call = engine_lib.pgx_goal_paths

    def refused(needle, *args):
        assert call(*args) == -1
        assert needle in engine_lib.pgx_last_error().decode()

    refused("planes, subgoal and length are all null", None, 0, 0, 0, None, None, None, None)
    refused("flags", None, 1, 0, 0, base, base, base, None)
    for fmt in (-1, 3, 99):
        refused("format", None, 0, 0, fmt, base, base, base, None)
    refused("format", None, 0, 0, 3, None, base, base, None)          # checked without planes too
    for steps in (-1, 961):
        refused("steps", None, 0, steps, 0, base, base, base, None)
    for fmt in (0, 2):
        for off in (1, 2, 3):
            refused("4-byte aligned", None, 0, 0, fmt, base + off, base, base, None)
    refused("length is not 4-byte aligned", None, 0, 0, 1, base, base, base + 2, None)
    # uint8 planes and the sub-goals take any address, any one output is enough, 0 and 960 are steps: the refusal that
    # remains is the NULL handle's
    refused("null handle", None, 0, 0, 1, base + 1, base + 1, base, None)
    refused("null handle", None, 0, 960, 0, base, None, None, None)
    refused("null handle", None, 0, 1, 2, None, base, None, None)
    refused("null handle", None, 0, 0, 0, None, None, base, None)
