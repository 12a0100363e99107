"""CPU: the neighbour-list reference (tests/visible_agents_reference.py, docs/SPEC.md S12) on hand-built cases, the C-ABI
of the feature (pgx_visible_agents declared with its exact prototype, exported, refused without a handle; no device
needed) and the register / scratch / occupancy budget of its kernels (hipcc cross-compiles gfx950)."""
import os
import re
import subprocess

import numpy as np
import pytest

from visible_agents_reference import visible_agents_env, visible_agents_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lists(agents, active, r, k):
    """Per agent: [(j, dx, dy), ...] of the filled entries, and the counts."""
    index, offset, count = visible_agents_env(np.array(agents), np.array(active, dtype=bool), r, k)
    assert index.dtype == np.int32 and offset.dtype == np.int8 and count.dtype == np.int32
    assert index.shape == (len(agents), k) and offset.shape == (len(agents), k, 2) and count.shape == (len(agents),)
    out = []
    for i in range(len(agents)):
        n = min(int(count[i]), k)
        assert (index[i, :n] >= 0).all() and (index[i, n:] == -1).all() and (offset[i, n:] == 0).all()
        out.append([(int(index[i, s]), int(offset[i, s, 0]), int(offset[i, s, 1])) for s in range(n)])
    return out, count.tolist()


def test_equal_distance_is_broken_by_window_row_then_column():
    # around agent 0 at (5, 5): four partners at distance 1, listed in the order of the loop below: up (dx = -1) first,
    # then the two of row dx = 0 by column, then down -- whatever their indices are
    agents = [(5, 5), (6, 5), (5, 6), (5, 4), (4, 5)]
    lists, count = _lists(agents, [1] * 5, r=2, k=8)
    assert lists[0] == [(4, -1, 0), (3, 0, -1), (2, 0, 1), (1, 1, 0)]
    assert count[0] == 4
    # a nearer agent comes before all of them, a farther one after: (1, 1) has squared distance 2
    lists, _ = _lists(agents + [(6, 6)], [1] * 6, r=2, k=8)
    assert lists[0] == [(4, -1, 0), (3, 0, -1), (2, 0, 1), (1, 1, 0), (5, 1, 1)]
    # seen from agent 1 at (6, 5): (5, 5) at distance 1, then (6, 6) at 1, then the diagonal ones
    assert lists[1] == [(0, -1, 0), (5, 0, 1), (3, -1, -1), (2, -1, 1), (4, -2, 0)]


def test_two_agents_on_one_cell_are_ordered_by_index():
    lists, count = _lists([(3, 3), (4, 4), (4, 4)], [1, 1, 1], r=1, k=4)
    assert lists[0] == [(1, 1, 1), (2, 1, 1)]
    assert lists[1] == [(2, 0, 0), (0, -1, -1)] and lists[2] == [(1, 0, 0), (0, -1, -1)]
    assert count == [2, 2, 2]


def test_window_edge_is_visible_and_one_cell_beyond_is_not():
    r = 3
    agents = [(10, 10), (13, 10), (10, 7), (14, 10), (10, 6), (13, 13), (7, 14)]
    lists, count = _lists(agents, [1] * 7, r=r, k=8)
    # |dx| = r and |dy| = r: visible (the window is a square: the corner too); r + 1: not
    assert lists[0] == [(2, 0, -3), (1, 3, 0), (5, 3, 3)]
    assert count[0] == 3


def test_inactive_neighbour_is_absent_and_inactive_observer_sees_nobody():
    agents = [(2, 2), (2, 3), (3, 2)]
    lists, count = _lists(agents, [1, 0, 1], r=2, k=4)
    assert lists == [[(2, 1, 0)], [], [(0, -1, 0)]]
    assert count == [1, 0, 1]
    index, offset, _ = visible_agents_env(np.array(agents), np.array([1, 0, 1], dtype=bool), 2, 4)
    assert (index[1] == -1).all() and (offset[1] == 0).all()


def test_count_is_not_capped_by_k_but_the_list_is():
    agents = [(4, 4)] + [(4 + dx, 4 + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx, dy) != (0, 0)]
    lists, count = _lists(agents, [1] * 9, r=1, k=3)
    assert count[0] == 8
    # the three nearest: distance 1 in window order (up, left, right); `down` no longer fits
    assert lists[0] == [(2, -1, 0), (4, 0, -1), (5, 0, 1)]


def test_k_larger_than_the_other_agents_pads_with_minus_one():
    index, offset, count = visible_agents_env(np.array([(0, 0), (0, 1)]), np.array([True, True]), 1, 5)
    assert index.tolist() == [[1, -1, -1, -1, -1], [0, -1, -1, -1, -1]]
    assert offset[0].tolist() == [[0, 1], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert offset[1].tolist() == [[0, -1], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert count.tolist() == [1, 1]
    # a single agent: nobody to see
    index, _, count = visible_agents_env(np.array([(3, 3)]), np.array([True]), 5, 2)
    assert index.tolist() == [[-1, -1]] and count.tolist() == [0]


def test_batched_reference_matches_per_env():
    rng = np.random.default_rng(12)
    xy = rng.integers(0, 9, size=(4, 7, 2))
    active = rng.random((4, 7)) < 0.8
    got = visible_agents_reference(xy, active, 3, 4)
    for b in range(4):
        for g, w in zip(got, visible_agents_env(xy[b], active[b], 3, 4)):
            assert np.array_equal(g[b], w)


def test_header_declares_and_library_exports(engine_lib):
    from pogema_amd import _lib
    raw = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+pgx_visible_agents\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+k\s*,\s*int32_t\s+flags\s*,"
                     r"\s*int32_t\s*\*\s*index\s*,\s*int8_t\s*\*\s*offset\s*,\s*int32_t\s*\*\s*count\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", text)
    m = re.search(r"#define\s+PGX_MAX_NEIGHBOURS\s+(\d+)\s", text)
    assert m and int(m.group(1)) == 32
    assert _lib.MAX_NEIGHBOURS == int(m.group(1))
    assert "pgx_visible_agents" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_visible_agents")
    # the ABI number did not move: the entry point is an addition
    assert re.search(r"#define\s+PGX_ABI_VERSION\s+6\s", text) and engine_lib.pgx_abi_version() == 6
    # refused without a handle through the shared entry prologue (no device needed)
    assert engine_lib.pgx_visible_agents(None, 8, 0, None, None, None, None) == -1
    assert b"pgx_visible_agents" in engine_lib.pgx_last_error()


# (sgpr, vgpr) of visible_agents_kernel<KT> as built when the kernels were written: the recorded budget.  KT registers
# hold the list; a count above these means the list left the registers or the sweep grew.
RECORDED_BUDGET = {8: (35, 36), 16: (35, 36), 32: (35, 67)}


def _hipcc():
    import shutil
    return shutil.which("hipcc") or next((c for c in ("/opt/rocm/bin/hipcc",) if os.path.exists(c)), None)


def test_kernels_have_no_scratch_and_keep_four_waves_per_simd():
    hipcc = _hipcc()
    if hipcc is None:  # an environment reason, as in tests/test_kernel_resources.py
        pytest.skip("no hipcc on this box: the gfx950 resource remarks cannot be produced")
    src = os.path.join(ROOT, "pogema_amd", "csrc", "pgx_neighbours.hip")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-x", "hip",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    kernels = {}
    name = None
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
    for name, u in kernels.items():  # every kernel of the file, whatever it is called
        print(name, u)
        assert u["ScratchSize"] == 0 and u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (name, u)
        assert u["Occupancy"] >= 4, (name, u)
        m = re.search(r"visible_agents_kernelILi(\d+)E", name)
        if m:
            kt = int(m.group(1))
            seen.add(kt)
            sgpr, vgpr = RECORDED_BUDGET[kt]
            assert u["TotalSGPRs"] <= sgpr and u["VGPRs"] <= vgpr, (name, u, RECORDED_BUDGET[kt])
    assert seen == set(RECORDED_BUDGET)
