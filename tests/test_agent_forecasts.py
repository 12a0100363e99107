"""CPU: the agent-forecast reference (tests/agent_forecasts_reference.py, docs/SPEC.md S24) on the hand-built cases of
tests/agent_forecasts_cases.py and the identities that tie it to the distance fields and the expert; the C-ABI of the
feature: pgx_agent_forecasts is declared and exported, and its argument checks need no device; the Python parsers refuse
what the section says, without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from agent_forecasts_cases import CASES, expected, grid
from agent_forecasts_reference import agent_forecasts_reference, rows
from expert_reference import MOVES, bfs_from, expert_reference
from pogema_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference(case, steps=None):
    return agent_forecasts_reference(grid(case["map"])[None], [case["agents_xy"]], [case["targets_xy"]], [case["is_active"]],
                                     case["r"], case["steps"] if steps is None else steps)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_built_cases(case):
    for steps in (None, 1):
        planes, cells = (v[0] for v in _reference(case, steps))
        want_planes, want_cells = expected(case, steps)
        assert cells.tolist() == want_cells.tolist() and cells.dtype == np.int16
        assert planes.tolist() == want_planes.tolist() and planes.dtype == np.uint8
    # a longer forecast starts with the shorter one
    long_planes, long_cells = (v[0] for v in _reference(case, 8))
    want_planes, want_cells = expected(case)
    K = case["steps"]
    assert np.array_equal(long_planes[:, :K], want_planes) and np.array_equal(long_cells[:, :K], want_cells)


def test_cases_cover_what_the_section_lists():
    names = {c["name"] for c in CASES}
    assert len(names) == len(CASES) == 7
    by = {c["name"]: c for c in CASES}
    c = by["arrives at step 2 and waits"]
    assert c["cells"][0][1] == tuple(c["targets_xy"][0]) == c["cells"][0][2] != c["cells"][0][0]
    c = by["unreachable target"]
    assert bfs_from(grid(c["map"]) != 0, *c["targets_xy"][0])[tuple(c["agents_xy"][0])] < 0
    c = by["two forecasts on one cell"]
    assert c["cells"][0][0] == c["cells"][1][0] and expected(c)[0][2, 0].sum() == 1
    c = by["leaves the window, re-enters it"]
    inside = [max(abs(x - 1), abs(y - 1)) <= 1 for x, y in [tuple(c["agents_xy"][1])] + c["cells"][1]]
    assert inside == [True, False, False, False, True]
    assert all(max(abs(x - 1), abs(y - 1)) > 1 for x, y in c["cells"][2])
    c = by["enters the window from outside"]
    assert abs(c["agents_xy"][1][1] - c["agents_xy"][0][1]) == 2 and abs(c["cells"][1][0][1] - c["agents_xy"][0][1]) == 1
    assert not expected(c)[0].any()
    c = by["inactive agent"]
    assert c["is_active"] == [False, True, True] and max(abs(a - b) for a, b in zip(c["agents_xy"][0], c["agents_xy"][1])) <= 1
    c = by["up before left"]
    assert c["cells"][0][0] == (0, 1)


def test_reference_identities_on_random_instances():
    """D_j[q_j(s)] = max(D_j[p0_j] - s, 0) for agents with a path; q_j(s) = p0_j for those without; cells[..., 0] is the
    cell the expert moves to; the planes hold exactly the cells of the visible others that fall into the window."""
    rng = np.random.default_rng(24)
    moves = np.array(MOVES)
    waited = moved = 0
    for r, K in ((1, 1), (2, 3), (5, 8), (3, 4)):
        B, A, H, W = 3, 7, 12, 12
        obst = (rng.random((B, H, W)) < 0.25).astype(np.uint8)
        agents = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)
        targets = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)  # obstacle targets included
        obst[np.arange(B)[:, None], agents[..., 0], agents[..., 1]] = 0                   # agents stand on free cells
        active = rng.random((B, A)) < 0.8
        planes, cells = agent_forecasts_reference(obst, agents, targets, active, r, K)
        actions, _ = expert_reference(obst, agents, targets, active)
        assert planes.shape == (B, A, K, 2 * r + 1, 2 * r + 1) and cells.shape == (B, A, K, 2)
        for b in range(B):
            for j in range(A):
                if not active[b, j]:
                    assert (cells[b, j] == -1).all() and not planes[b, j].any()
                    continue
                D = bfs_from(obst[b] != 0, *targets[b, j])
                d0 = D[tuple(agents[b, j])]
                for s in range(1, K + 1):
                    q = tuple(cells[b, j, s - 1])
                    if d0 < 0:
                        assert q == tuple(agents[b, j])
                        waited += 1
                    else:
                        assert D[q] == max(d0 - s, 0)
                        moved += 1
                assert tuple(cells[b, j, 0]) == tuple(agents[b, j] + moves[actions[b, j]])
                # the planes, from the cells alone
                want = np.zeros_like(planes[b, j])
                for k in range(A):
                    if k != j and active[b, k] and np.abs(agents[b, k] - agents[b, j]).max() <= r:
                        for s in range(K):
                            u, v = cells[b, k, s] - agents[b, j] + r
                            if 0 <= u <= 2 * r and 0 <= v <= 2 * r:
                                want[s, u, v] = 1
                assert np.array_equal(planes[b, j], want)
    assert waited and moved
    only = agent_forecasts_reference(obst, agents, targets, active, r, K, envs=[1])
    assert all(np.array_equal(o[1], g[1]) and not o[[0, 2]].any() for o, g in zip(only, (planes, cells)))


def test_rows_pack_the_planes():
    planes, _ = _reference(CASES[2])         # two forecasts on one cell
    assert rows(planes)[0, 2].tolist() == [[0, 0b010, 0], [0, 0b100, 0b010], [0, 0b100, 0b010]]
    assert rows(planes).dtype == np.int32 and rows(planes).shape == planes.shape[:-1]
    full = np.ones((31, 31), dtype=np.uint8)
    assert (rows(full) == 2**31 - 1).all(), "W <= 31: the sign bit is never set"


def test_header_declares_and_library_exports(engine_lib):
    src = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+pgx_agent_forecasts\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+steps\s*,\s*int32_t\s+format\s*,"
                     r"\s*int32_t\s+flags\s*,\s*void\s*\*\s*planes\s*,\s*int16_t\s*\*\s*cells\s*,\s*void\s*\*\s*stream\s*\)", text)
    for name, code in (("F32", 0), ("U8", 1), ("ROWS", 2)):
        assert re.search(rf"#define\s+PGX_FORECAST_{name}\s+{code}\b", text)
    assert re.search(r"#define\s+PGX_MAX_FORECAST_STEPS\s+8\b", text)
    assert re.search(r"#define\s+PGX_ABI_VERSION\s+6\b", text), "the entry point is additive"
    assert _lib.FORECAST_FORMATS == {"float32": 0, "uint8": 1, "rows": 2}
    assert _lib.MAX_FORECAST_STEPS == 8
    assert "pgx_agent_forecasts" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_agent_forecasts")


def test_invalid_arguments_need_no_device(engine_lib):
    """PGX_E_INVALID for a NULL `cells`, steps outside 1..8, an unknown format, non-zero flags, a misaligned float32 or
    rows `planes` and an odd `cells` address: checked before the handle, so a NULL handle is never reached (a well-formed
    call on a NULL handle is refused too)."""
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf)
    base += -base % 16
    call = engine_lib.pgx_agent_forecasts   # (env, steps, format, flags, planes, cells, stream)

    def refused(needle, *args):
        assert call(*args) == -1
        assert needle in engine_lib.pgx_last_error().decode()

    refused("cells is null", None, 3, 0, 0, base, None, None)
    refused("cells is null", None, 3, 0, 0, None, None, None)
    for steps in (0, -1, 9, 960):
        refused("steps", None, steps, 0, 0, base, base, None)
    for fmt in (-1, 3, 99):
        refused("format", None, 3, fmt, 0, base, base, None)
    refused("format", None, 3, 3, 0, None, base, None)                # checked without planes too
    refused("flags", None, 3, 0, 1, base, base, None)
    for fmt in (0, 2):
        for off in (1, 2, 3):
            refused("planes is not 4-byte aligned", None, 3, fmt, 0, base + off, base, None)
    refused("cells is not 2-byte aligned", None, 3, 1, 0, base, base + 1, None)
    # uint8 planes take any address, cells any even one, planes may be NULL, 1 and 8 are steps: the refusal that remains is
    # the NULL handle's
    refused("null handle", None, 1, 1, 0, base + 1, base + 2, None)
    refused("null handle", None, 8, 0, 0, base, base, None)
    refused("null handle", None, 3, 2, 0, None, base + 6, None)


def test_parsers_need_no_gpu():
    from pogema_amd.queries import parse_forecast_format, parse_forecast_steps
    import torch
    for ok in (1, 3, 8, np.int64(2), np.int16(8)):
        got = parse_forecast_steps(ok)
        assert got == int(ok) and type(got) is int
    assert parse_forecast_steps() == 3
    for bad in (0, -1, 9, 960, 2.0, True, False, "3", None, (3,)):
        with pytest.raises(ValueError, match=r"1\.\.8"):
            parse_forecast_steps(bad)
    assert parse_forecast_format() == (0, torch.float32, False)
    assert parse_forecast_format("uint8") == (1, torch.uint8, False)
    assert parse_forecast_format("rows") == (2, torch.int32, True)
    for bad in ("bits", "float16", "", None, 0, torch.float32):
        with pytest.raises(ValueError, match=r"\['float32', 'rows', 'uint8'\]"):
            parse_forecast_format(bad)
