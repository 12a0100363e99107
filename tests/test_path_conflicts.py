"""CPU: the path-conflict reference (tests/path_conflicts_reference.py, docs/SPEC.md S26) on the hand-built cases of
tests/path_conflicts_cases.py and the identities of the section on random paths; the Python parsers' refusals; the C-ABI
of the feature: pgx_path_conflicts is declared with its exact prototype and exported, and its argument checks need no
device; the resources of the kernel's instances; and the proof that the GPU suite's random inputs hold what it is about."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from agent_forecasts_reference import agent_forecasts_reference
from path_conflicts_cases import ALL, CASES, FORECAST_INPUTS, PLAN_INPUT, expected, grid, paths_of
from path_conflicts_reference import KINDS, incidences, path_conflicts_reference
from pibt_plan_reference import pibt_plan_reference
from pogema_amd import _lib
from util import generate_instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference(case, layout, kinds, arrived):
    H, W = grid(case["map"]).shape
    return tuple(v[0] for v in path_conflicts_reference(paths_of(case, layout), [case["agents_xy"]], [case["targets_xy"]],
                                                        [case["is_active"]], H, W, kinds, arrived == "vanish"))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_built_cases(case):
    for chk in case["checks"]:
        for layout in ("cells", "plan"):
            got = _reference(case, layout, chk["kinds"], chk["arrived"])
            for name, g, w in zip(("first_step", "partner", "kind", "count"), got, expected(chk)):
                assert g.dtype == w.dtype and g.tolist() == w.tolist(), (case["name"], chk["kinds"], chk["arrived"], layout, name)


def test_cases_cover_what_the_section_lists():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(CASES) == 13
    by = {c["name"]: c for c in CASES}
    for name, dist, kind in (("head on, odd distance: edge", 3, 2), ("head on, even distance: vertex", 4, 1),
                             ("first conflict at step K", 5, 2)):
        c = by[name]
        assert abs(c["agents_xy"][0][1] - c["agents_xy"][1][1]) == dist
        assert c["checks"][0]["first"] == [(dist + 1) // 2] * 2 and c["checks"][0]["kind"] == [kind] * 2
    assert by["first conflict at step K"]["checks"][0]["first"][0] == len(by["first conflict at step K"]["paths"][0])
    assert sum(len(c["paths"][0]) == 1 for c in CASES) >= 3, "K = 1"
    assert by["three reach one cell"]["checks"][0]["count"] == [2, 2, 2]
    assert by["forty on one cell"]["checks"][0]["count"] == [39] * 40
    c = by["follow chain"]
    assert {chk["kinds"]: chk["count"] for chk in c["checks"]}[("vertex", "edge")] == [0, 0, 0]
    c = by["crosses a target after the arrival"]
    assert c["paths"][1][1] == tuple(c["targets_xy"][1]) == c["paths"][0][3]
    assert {chk["arrived"]: chk["first"] for chk in c["checks"]} == {"stay": [4, 4], "vanish": [-1, -1]}
    c = by["stands on its target"]
    assert c["agents_xy"][0] == c["targets_xy"][0] and c["is_active"][0]
    assert by["inactive agent"]["is_active"] == [False, True]
    assert (-1, -1) in by["a cell outside the map"]["paths"][0][1:-1]
    c = by["vertex and edge at one step"]["checks"][0]
    assert c["kind"][0] == 3 and c["partner"][0] == 1
    c = by["swap by a jump"]
    assert abs(c["agents_xy"][0][0] - c["paths"][0][0][0]) > 1


def _random_paths(rng, B, A, H, W, K, p_out=0.05):
    """Random walks with waits, a few cells outside the map, inactive agents and agents that start on their targets."""
    moves = np.array([(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)])
    agents = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)
    targets = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)
    targets[:, 0] = agents[:, 0]                                         # agent 0 stands on its target
    active = rng.random((B, A)) < 0.85
    pos, steps = agents.copy(), []
    for _ in range(K):
        pos = np.clip(pos + moves[rng.integers(0, 5, (B, A))], 0, [H - 1, W - 1])
        steps.append(np.where(rng.random((B, A, 1)) < p_out, -1, pos))
    return np.stack(steps).astype(np.int32), agents, targets, active     # the plan layout


def test_reference_identities_on_random_paths():
    """Per env the vertex and the edge incidences are symmetric (so their sums are even); the three kinds exclude each
    other; a path's first K' steps give the result of the path cut to K' for every agent whose first_step <= K', and count
    grows with K; both layouts give one result."""
    rng = np.random.default_rng(26)
    seen = dict.fromkeys(KINDS, 0)
    for B, A, H, W, K in ((4, 12, 4, 4, 6), (3, 30, 5, 6, 4), (2, 5, 3, 3, 9)):
        paths, agents, targets, active = _random_paths(rng, B, A, H, W, K)
        cells = np.ascontiguousarray(paths.transpose(1, 2, 0, 3)).astype(np.int16)
        for vanish in (False, True):
            vertex, edge, follow = incidences(paths, agents, targets, active, H, W, vanish)
            assert np.array_equal(vertex, vertex.transpose(0, 1, 3, 2)) and np.array_equal(edge, edge.transpose(0, 1, 3, 2))
            assert (vertex.sum((0, 2, 3)) % 2 == 0).all() and (edge.sum((0, 2, 3)) % 2 == 0).all()
            assert not (vertex & edge).any() and not (vertex & follow).any() and not (edge & follow).any()
            assert not any(m[:, ~active].any() or m.transpose(0, 1, 3, 2)[:, ~active].any() for m in (vertex, edge, follow))
            for name, m in zip(KINDS, (vertex, edge, follow)):
                seen[name] += int(m.sum())
            full = path_conflicts_reference(paths, agents, targets, active, H, W, ALL, vanish)
            assert all(np.array_equal(a, b) for a, b in
                       zip(full, path_conflicts_reference(cells, agents, targets, active, H, W, ALL, vanish)))
            assert (full[3] == (vertex | edge | follow).sum((0, 3))).all()
            assert ((full[0] == -1) == (full[3] == 0)).all() and ((full[1] == -1) == (full[0] == -1)).all()
            assert (full[0][~active] == -1).all() and (full[2][~active] == 0).all()
            for cut in range(1, K):
                short = path_conflicts_reference(paths[:cut], agents, targets, active, H, W, ALL, vanish)
                early = (full[0] >= 1) & (full[0] <= cut)
                assert all(np.array_equal(s[early], f[early]) for s, f in zip(short[:3], full[:3]))
                assert (short[0][~early] == -1).all() and (short[3] <= full[3]).all()
    assert all(seen.values()), seen


def test_parsers_need_no_gpu():
    from pogema_amd.queries import parse_conflict_arrived, parse_conflict_kinds
    import pogema_amd
    assert pogema_amd.CONFLICT_KINDS is _lib.CONFLICT_KINDS and _lib.CONFLICT_KINDS == {"vertex": 1, "edge": 2, "follow": 4} == KINDS
    assert parse_conflict_kinds() == 3
    assert parse_conflict_kinds(["follow"]) == 4 and parse_conflict_kinds(("edge", "follow", "vertex")) == 7
    for bad in ((), [], "vertex", None, 3, ("vertex", "vertex"), ("vertex", "swap"), ("edge", 2), {"vertex"}):
        with pytest.raises(ValueError, match=r"'vertex', 'edge', 'follow'"):
            parse_conflict_kinds(bad)
    assert parse_conflict_arrived() == 0 and parse_conflict_arrived("stay") == 8 and parse_conflict_arrived("vanish") == 16
    for bad in ("finish", "", 0, True, ("stay",)):
        with pytest.raises(ValueError, match=r"None, 'stay' or 'vanish'"):
            parse_conflict_arrived(bad)


def test_header_declares_and_library_exports(engine_lib):
    src = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+pgx_path_conflicts\s*\(\s*pgx_env\s*\*\s*env\s*,\s*const\s+void\s*\*\s*paths\s*,\s*int32_t\s+layout\s*,"
                     r"\s*int32_t\s+steps\s*,\s*int32_t\s+flags\s*,\s*int32_t\s*\*\s*first_step\s*,\s*int32_t\s*\*\s*partner\s*,"
                     r"\s*uint8_t\s*\*\s*kind\s*,\s*int32_t\s*\*\s*count\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    for name, code in (("PATHS_PLAN", 0), ("PATHS_CELLS", 1), ("VERTEX", 1), ("EDGE", 2), ("FOLLOW", 4), ("STAY", 8), ("VANISH", 16)):
        assert re.search(rf"#define\s+PGX_CONFLICT_{name}\s+{code}\b", text)
    assert re.search(r"#define\s+PGX_MAX_CONFLICT_STEPS\s+256\b", text) and re.search(r"#define\s+PGX_MAX_PLAN_HORIZON\s+256\b", text)
    assert re.search(r"#define\s+PGX_ABI_VERSION\s+6\b", text), "the entry point is additive"
    assert _lib.MAX_CONFLICT_STEPS == _lib.MAX_PLAN_HORIZON == 256
    assert (_lib.CONFLICT_PATHS_PLAN, _lib.CONFLICT_PATHS_CELLS) == (0, 1)
    assert _lib.CONFLICT_ARRIVED == {None: 0, "stay": 8, "vanish": 16}
    assert "pgx_path_conflicts" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_path_conflicts")


def test_invalid_arguments_need_no_device(engine_lib):
    """Every PGX_E_INVALID of the section is answered before the handle is looked at, with the argument's name in
    pgx_last_error(); a well-formed call on a NULL handle is refused for the handle."""
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf)
    base += -base % 16
    call = engine_lib.pgx_path_conflicts   # (env, paths, layout, steps, flags, first_step, partner, kind, count, stream)

    def refused(needle, *args):
        assert call(None, *args, None) == -1
        assert needle in engine_lib.pgx_last_error().decode(), engine_lib.pgx_last_error().decode()

    outs = (base, base, base, base)
    refused("paths is null", None, 0, 3, 3, *outs)
    refused("every output is null", base, 0, 3, 3, None, None, None, None)
    for steps in (0, -1, 257, 2 ** 31 - 1):
        refused("steps", base, 0, steps, 3, *outs)
    for layout in (-1, 2, 99):
        refused("layout", base, layout, 3, 3, *outs)
    for flags in (0, 8, 16):
        refused("no conflict kind", base, 0, 3, flags, *outs)
    refused("PGX_CONFLICT_STAY and PGX_CONFLICT_VANISH", base, 0, 3, 1 | 8 | 16, *outs)
    for flags in (32, 1 | 64, -1, 3 | 1 << 30):
        refused("unknown flags", base, 0, 3, flags, *outs)
    for off in (1, 2, 3):
        refused("plan-layout paths is not 4-byte aligned", base + off, 0, 3, 3, *outs)
        refused("first_step is not 4-byte aligned", base, 0, 3, 3, base + off, base, base, base)
        refused("partner is not 4-byte aligned", base, 0, 3, 3, base, base + off, base, base)
        refused("count is not 4-byte aligned", base, 0, 3, 3, base, base, base, base + off)
    for off in (1, 3):
        refused("cells-layout paths is not 2-byte aligned", base + off, 1, 3, 3, *outs)
    # cells-layout paths take any even address, kind any address, any one output is enough, 1 and 256 are steps, every
    # kind subset and either arrival flag: the refusal that remains is the NULL handle's
    refused("null handle", base + 2, 1, 1, 3, base, base, base + 1, base)
    refused("null handle", base + 6, 1, 256, 4 | 8, None, None, base + 3, None)
    refused("null handle", base, 0, 256, 7 | 16, None, None, None, base)
    refused("null handle", base + 4, 0, 8, 2, base, None, None, None)


# ---- kernel resources --------------------------------------------------------------------------------------------------
# (lanes, layout) -> (TotalSGPRs, VGPRs, LDS bytes) of path_conflicts_kernel as built for gfx950; layout 0 = plan, 1 = cells
RECORDED_BUDGET = {(256, 0): (72, 40, 10240), (256, 1): (72, 40, 10240),
                   (1024, 0): (72, 40, 40960), (1024, 1): (72, 40, 40960)}


def test_kernels_have_no_scratch_and_stay_inside_their_budget():
    """Every instance of pgx_path_conflicts.hip's kernel: no scratch, no spills, the recorded register budget (measured at
    build time: 66 SGPRs and 37 VGPRs for the plan layout, 64 and 36 for the cells layout, with 256 and with 1024 lanes:
    8 waves per SIMD), and an LDS block of 40 bytes per lane -- the largest, 1024 lanes, is 40 KB of the CU's 160 KB and
    within the 64 KB a static allocation may have."""
    hipcc = shutil.which("hipcc") or next((c for c in ("/opt/rocm/bin/hipcc",) if os.path.exists(c)), None)
    if hipcc is None:  # an environment reason, as in tests/test_kernel_resources.py
        pytest.skip("no hipcc on this box: the gfx950 resource remarks cannot be produced")
    src = os.path.join(ROOT, "pogema_amd", "csrc", "pgx_path_conflicts.hip")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-x", "hip",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    kernels, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", ln)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?:\s+(\d+)", ln)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    seen = set()
    assert kernels, p.stderr[-2000:]
    for name, u in kernels.items():           # every kernel of the file, whatever it is called
        print(name, u)
        assert u["ScratchSize"] == 0 and u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (name, u)
        m = re.search(r"path_conflicts_kernelILi(\d+)ELi(\d+)EE", name)
        assert m, name
        key = (int(m.group(1)), int(m.group(2)))
        seen.add(key)
        sgpr, vgpr, lds = RECORDED_BUDGET[key]
        assert u["TotalSGPRs"] <= sgpr and u["VGPRs"] <= vgpr and u["LDS Size"] == lds, (name, u, RECORDED_BUDGET[key])
        assert u["LDS Size"] == 40 * key[0] and u["LDS Size"] <= 64 * 1024
        assert u["Occupancy"] >= 8, (name, u)
    assert seen == set(RECORDED_BUDGET)


# ---- the GPU suite's random inputs are not vacuous ---------------------------------------------------------------------
def _counts(paths, agents, targets, active, size, vanish):
    return [int(m.sum()) for m in incidences(paths, agents, targets, active, size, size, vanish)]


@pytest.mark.parametrize("inp", FORECAST_INPUTS, ids=[f"{i['size']}x{i['size']}" for i in FORECAST_INPUTS])
def test_forecast_inputs_hold_every_kind(inp):
    """Each forecast input of the GPU suite holds, on its reset state, at least one vertex, one edge and one follow
    incidence, an agent whose first conflict comes after step 1 and an agent whose result differs between "stay" and
    "vanish" -- and, with K = 3 (the lane-layout tests' K), still a conflict."""
    B, size, A, K = inp["batch"], inp["size"], inp["agents"], inp["steps"]
    obstacles, agents, targets = generate_instances(B, size, size, A, inp["density"], inp["seed"])
    active = np.ones((B, A), dtype=bool)
    _, cells = agent_forecasts_reference(obstacles, agents, targets, active, 1, K)
    stay = _counts(cells, agents, targets, active, size, False)
    print(inp, "stay (vertex, edge, follow):", stay, "vanish:", _counts(cells, agents, targets, active, size, True))
    assert min(stay) >= 1, stay
    a = path_conflicts_reference(cells, agents, targets, active, size, size, ALL, False)
    b = path_conflicts_reference(cells, agents, targets, active, size, size, ALL, True)
    assert (a[0] > 1).any() and (b[0] > 1).any()
    assert any((x != y).any() for x, y in zip(a, b))
    assert sum(_counts(cells[:, :, :3], agents, targets, active, size, False)) >= 1


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_plan_input_holds_follows_and_nothing_else(on_target):
    """The plan input of the GPU suite: the reference planner's paths have no vertex and no edge incidence, judged the way
    they were made, and at least one follow incidence."""
    inp = PLAN_INPUT
    B, size, A, K = inp["batch"], inp["size"], inp["agents"], inp["steps"]
    obstacles, agents, targets = generate_instances(B, size, size, A, inp["density"], inp["seed"])
    active = np.ones((B, A), dtype=bool)
    path = pibt_plan_reference(obstacles, agents, targets, active, K, on_target=on_target)[1]
    vertex, edge, follow = _counts(path, agents, targets, active, size, on_target == "finish")
    print(on_target, "vertex, edge, follow:", vertex, edge, follow)
    assert vertex == 0 and edge == 0 and follow >= 1
