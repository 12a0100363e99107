"""CPU: the reference of collision shielding (tests/shield_reference.py, docs/SPEC.md S15) -- equal to the planner's
reference when the scores say nothing, S13's guarantees for any scores, the order of NaN, infinities and signed zeros on
cases worked by hand -- the coverage the inputs of tests/test_shield_gpu.py must have, and the C-ABI of the feature
(pgx_shield_actions declared with its exact prototype, exported, argument checks answered without a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pibt_reference import check_invariants, pibt_env
from shield_inputs import crowd_scores, crowd_state, random_scores, special_scores
from shield_reference import shield_env, shield_reference
from util import generate_instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STAY, UP, DOWN, LEFT, RIGHT = 0, 1, 2, 3, 4
NAN, INF = float("nan"), float("inf")


def _grid(text):
    return np.array([[c == "#" for c in row] for row in text.split()], dtype=np.uint8)


def _plan(text, agents, targets, scores, active=None, priority=None, tie_break=None):
    active = [1] * len(agents) if active is None else active
    actions, next_xy, overridden, failed = shield_env(_grid(text), agents, targets, active, np.array(scores, dtype=np.float32),
                                                      priority, tie_break)
    assert actions.dtype == np.int64 and next_xy.dtype == np.int32 and overridden.dtype == np.uint8
    return actions.tolist(), [tuple(v) for v in next_xy.tolist()], overridden.tolist(), failed


def _instances(seed, cases, packed=False):
    """Small instances with inactive agents and priorities: (obstacles, pos, tgt, active, prio, rng) per case, from the
    host generator; `packed`: hand-placed instead, on most of the free cells, so that pushes fail."""
    rng = np.random.default_rng(seed)
    for case in range(cases):
        size = int(rng.integers(4, 8))
        if packed:
            obst = (rng.random((size, size)) < 0.2).astype(np.uint8)
            free = np.argwhere(obst == 0)
            A = max(1, int(len(free) * rng.uniform(0.5, 0.95)))
            pos = free[rng.permutation(len(free))[:A]].astype(np.int32)
            tgt = free[rng.integers(0, len(free), size=A)].astype(np.int32)
        else:
            A = int(rng.integers(1, size * size // 2))
            obst, pos, tgt = (v[0] for v in generate_instances(1, size, size, A, 0.2, seed + case))
        yield obst, pos, tgt, rng.random(A) < 0.9, (None if case % 3 == 0 else rng.integers(-2, 3, size=A)), rng


def test_constant_scores_with_distance_tie_break_are_the_planner():
    pushed = 0
    for obst, pos, tgt, active, prio, rng in _instances(15, 30):
        for step in range(6):
            want_a, want_n = pibt_env(obst, pos, tgt, active, prio)
            for value in (0.0, -2.5, INF, NAN):
                a, n, o, _ = shield_env(obst, pos, tgt, active, np.full((len(pos), 5), value, dtype=np.float32), prio, "distance")
                assert np.array_equal(a, want_a) and np.array_equal(n, want_n), (step, value)
                assert np.array_equal(o, (want_a != 0) & active)      # the argmax of equal scores is action 0
            pushed += int(((want_a != 0) & active).sum())
            pos = want_n
    assert pushed > 300


def test_guarantees_hold_for_any_scores():
    """Random, adversarial (every agent scores the same direction highest), constant and special-valued scores, both
    tie-break modes, along episodes in which every planned agent moves to its next cell (what a `soft` step does)."""
    failed = overridden = kept = 0
    for obst, pos, tgt, active, prio, rng in _instances(2025, 24, packed=True):
        A = len(pos)
        for step in range(8):
            kind = step % 4
            if kind == 0:
                scores = random_scores(rng, 1, A)[0]
            elif kind == 1:
                scores = np.zeros((A, 5), dtype=np.float32)
                scores[:, 1 + (step // 4 + A) % 4] = 1.0
            elif kind == 2:
                scores = np.full((A, 5), 0.5, dtype=np.float32)
            else:
                scores = special_scores(rng, 1, A)[0]
            for tie_break in (None, "distance"):
                a, n, o, f = shield_env(obst, pos, tgt, active, scores, prio, tie_break)
                assert check_invariants(obst, pos, active, n) == [], (step, tie_break)
                assert (a[~active] == 0).all() and (n[~active] == pos[~active]).all() and (o[~active] == 0).all()
                failed += f
                overridden += int(o.sum())
                kept += int((o[active] == 0).sum())
            pos = n
    assert failed > 20 and overridden > 200 and kept > 200, (failed, overridden, kept)


def test_higher_score_first_then_lower_action():
    # alone in the open: the argmax is taken, nothing is overridden
    assert _plan("... ... ...", [(1, 1)], [(0, 0)], [[0, 1, 5, 2, 3]]) == ([DOWN], [(2, 1)], [0], 0)
    # equal scores: the lowest action, which is to stay
    assert _plan("... ... ...", [(1, 1)], [(0, 0)], [[2, 2, 2, 2, 2]]) == ([STAY], [(1, 1)], [0], 0)
    assert _plan("... ... ...", [(1, 1)], [(0, 0)], [[0, 2, 2, 2, 2]]) == ([UP], [(0, 1)], [0], 0)
    # ... unless distance breaks the tie: down and right both lead towards (2, 2), down is the lower action
    assert _plan("... ... ...", [(1, 1)], [(2, 2)], [[0, 2, 2, 2, 2]], tie_break="distance") == ([DOWN], [(2, 1)], [1], 0)


def test_the_shield_is_the_action_mask():
    # in the corner (0, 0): up and left leave the map whatever their score, down is an obstacle
    assert _plan(".. #.", [(0, 0)], [(1, 1)], [[0, 9, 8, 7, 1]]) == ([RIGHT], [(0, 1)], [1], 0)
    assert _plan(".. #.", [(0, 0)], [(1, 1)], [[0, INF, INF, INF, -INF]]) == ([STAY], [(0, 0)], [1], 0)


def test_nan_ranks_below_minus_infinity_and_zeros_are_equal():
    open3 = "... ... ..."
    # NaN is the worst score: -inf beats it
    assert _plan(open3, [(1, 1)], [(0, 0)], [[NAN, NAN, -INF, NAN, NAN]]) == ([DOWN], [(2, 1)], [0], 0)
    # +inf beats everything finite; NaN does not count as large
    assert _plan(open3, [(1, 1)], [(0, 0)], [[1e30, NAN, 3, INF, NAN]]) == ([LEFT], [(1, 0)], [0], 0)
    # all NaN: equal, the lowest action; the argmax of five NaN is action 0
    assert _plan(open3, [(1, 1)], [(0, 0)], [[NAN] * 5]) == ([STAY], [(1, 1)], [0], 0)
    # -0.0 == +0.0: the lower action wins the tie, in either order of the signs
    assert _plan(open3, [(1, 1)], [(0, 0)], [[-1, -0.0, 0.0, -1, -1]]) == ([UP], [(0, 1)], [0], 0)
    assert _plan(open3, [(1, 1)], [(0, 0)], [[-1, 0.0, -0.0, -1, -1]]) == ([UP], [(0, 1)], [0], 0)
    assert _plan(open3, [(1, 1)], [(0, 0)], [[-1, -1e-45, -0.0, 0.0, -1]]) == ([DOWN], [(2, 1)], [0], 0)
    # the argmax over all five actions counts blocked ones too: up leaves the map, so the choice was overridden
    assert _plan(open3, [(0, 1)], [(0, 0)], [[NAN, -INF, NAN, NAN, NAN]]) == ([STAY], [(0, 1)], [1], 0)


def test_scores_replace_distance_in_pushes_and_failures():
    # both want to go right; 1 is pushed on by 0 (its own cell is reserved by then), nobody is overridden
    right = [0, 0, 0, 0, 1]
    assert _plan("....", [(0, 0), (0, 1)], [(0, 0), (0, 0)], [right, right]) == ([RIGHT, RIGHT], [(0, 1), (0, 2)], [0, 0], 0)
    # 1 at the end of the row cannot move on: its call fails, it keeps its cell, 0 falls back to staying
    assert _plan("..", [(0, 0), (0, 1)], [(0, 0), (0, 0)], [right, right]) == ([STAY, STAY], [(0, 0), (0, 1)], [1, 1], 1)
    # head on: 0 plans first and takes 1's cell, 1 may not swap and retreats; with the priorities reversed 0 retreats
    want = [[0, 0, 0, -1, 1], [0, 0, 0, 1, -1]]
    assert _plan("....", [(0, 1), (0, 2)], [(0, 0), (0, 0)], want) == ([RIGHT, RIGHT], [(0, 2), (0, 3)], [0, 1], 0)
    assert _plan("....", [(0, 1), (0, 2)], [(0, 0), (0, 0)], want, priority=[0, 5]) == ([LEFT, LEFT], [(0, 0), (0, 1)], [1, 0], 0)
    # an inactive agent is ignored: no action, no cell, never overridden
    assert _plan("...", [(0, 0), (0, 1)], [(0, 2), (0, 1)], [right, right], active=[1, 0]) == \
        ([RIGHT, STAY], [(0, 1), (0, 1)], [0, 0], 0)


# ---- the inputs of tests/test_shield_gpu.py do exercise what they are there for -------------------------------------
def test_crowd_input_backtracks_in_every_env():
    """At least one PIBT call returns False in every env, at the start and along six steps in which every agent moves to
    its next cell."""
    obst, pos, tgt = crowd_state()
    active = np.ones(pos.shape[:2], dtype=bool)
    scores = crowd_scores()
    moved = 0
    for step in range(6):
        a, n, o, failed = shield_reference(obst, pos, tgt, active, scores)
        assert (failed >= 1).all(), (step, failed)
        for b in range(2):
            assert check_invariants(obst[b], pos[b], active[b], n[b]) == [], (step, b)
        a2, n2, o2, failed2 = shield_reference(obst, pos, tgt, active, scores, tie_break="distance")
        assert np.array_equal(a, a2) and np.array_equal(n, n2)      # distinct scores: the tie-break has no say
        moved += int((a != 0).sum())
        pos = n
    assert moved > 100


@pytest.mark.parametrize("agents,size,batch", [(1, 6, 40), (2, 6, 40), (3, 7, 40), (8, 10, 40), (16, 12, 37), (33, 14, 9),
                                               (65, 18, 5)])
def test_random_scores_are_partly_overridden(agents, size, batch):
    """The mean of `overridden` lies strictly between 0 and 1 on generated instances of the lane-layout shapes."""
    rng = np.random.default_rng(agents)
    obst, pos, tgt = generate_instances(batch, size, size, agents, 0.1, agents + 1)
    active = np.ones((batch, agents), dtype=bool)
    _, n, o, _ = shield_reference(obst, pos, tgt, active, random_scores(rng, batch, agents))
    assert 0.0 < o.mean() < 1.0, o.mean()
    for b in range(batch):
        assert check_invariants(obst[b], pos[b], active[b], n[b]) == []


# ---- the C-ABI ---------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports(engine_lib):
    from pogema_amd import _lib
    raw = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+pgx_shield_actions\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+flags\s*,\s*const\s+void\s*\*\s*scores\s*,"
                     r"\s*int32_t\s+score_dtype\s*,\s*const\s+int32_t\s*\*\s*priority\s*,\s*void\s*\*\s*actions\s*,"
                     r"\s*int32_t\s+action_dtype\s*,\s*int32_t\s*\*\s*next_xy\s*,\s*uint8_t\s*\*\s*overridden\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", text)
    for name, value in (("PGX_SCORES_F32", 0), ("PGX_SCORES_F16", 1), ("PGX_SCORES_BF16", 2), ("PGX_SHIELD_TIE_DISTANCE", 1)):
        assert re.search(rf"#define\s+{name}\s+{value}\s", text), name
    assert "pgx_shield_actions" in _lib.EXPORTED_SYMBOLS and hasattr(engine_lib, "pgx_shield_actions")
    assert _lib.SHIELD_TIE_BREAKS == {None: 0, "distance": 1}
    # the ABI number did not move: the entry point is an addition
    assert re.search(r"#define\s+PGX_ABI_VERSION\s+6\s", text) and engine_lib.pgx_abi_version() == 6


def test_argument_checks_need_no_device(engine_lib):
    """PGX_E_INVALID (-1) with a message naming the argument; the checks run before the handle is looked at."""
    call = engine_lib.pgx_shield_actions
    buf = C.create_string_buffer(64)
    ptr = (C.addressof(buf) + 15) // 16 * 16       # a 16-byte aligned address that is never dereferenced
    #          flags scores  sdt prio  actions adt next  overridden
    for args, word in (((0, None, 0, None, ptr, 2, None, None), b"scores"),
                       ((0, ptr, 0, None, None, 2, None, None), b"actions"),
                       ((2, ptr, 0, None, ptr, 2, None, None), b"flags"),
                       ((-8, ptr, 0, None, ptr, 2, None, None), b"flags"),
                       ((0, ptr, 3, None, ptr, 2, None, None), b"score_dtype"),
                       ((1, ptr, -1, None, ptr, 2, None, None), b"score_dtype"),
                       ((0, ptr, 0, None, ptr, 3, None, None), b"action_dtype"),
                       ((0, ptr + 2, 0, None, ptr, 2, None, None), b"scores"),
                       ((0, ptr + 1, 1, None, ptr, 2, None, None), b"scores"),
                       ((0, ptr + 1, 2, None, ptr, 2, None, None), b"scores"),
                       ((0, ptr, 0, None, ptr + 4, 2, None, None), b"actions"),
                       ((0, ptr, 0, ptr + 2, ptr, 0, None, None), b"priority"),
                       ((1, ptr, 0, None, ptr, 0, ptr + 1, None), b"next_xy")):
        assert call(None, *args, None) == -1, args
        msg = engine_lib.pgx_last_error()
        assert b"pgx_shield_actions" in msg and word in msg, (args, msg)
    # valid arguments (2-byte aligned f16 scores, any `overridden` address), no handle: refused by the shared entry prologue
    for flags in (0, 1):
        assert call(None, flags, ptr + 2, 1, None, ptr, 2, None, ptr + 1, None) == -1
        assert b"pgx_shield_actions" in engine_lib.pgx_last_error() and b"handle" in engine_lib.pgx_last_error()


def test_python_argument_checks_need_no_engine():
    """What VecPogema.shield_actions refuses before the engine is called, on a stand-in without a device."""
    import torch
    from pogema_amd.queries import QueryMixin

    class Stub(QueryMixin):
        batch, num_agents, device = 2, 3, torch.device("cpu")
        _ACTION_CODE = {torch.int8: 0, torch.int32: 1, torch.int64: 2}

    env = Stub()
    good = torch.zeros((2, 3, 5))
    with pytest.raises(TypeError, match="scores"):
        env.shield_actions([[0.0] * 5] * 3)
    for dtype in (torch.float64, torch.int32):
        with pytest.raises(TypeError, match="scores"):
            env.shield_actions(good.to(dtype))
    for bad in (torch.zeros((2, 3, 4)), torch.zeros((2, 3)), torch.zeros((3, 2, 5)), torch.zeros((2, 3, 5), device="meta")):
        with pytest.raises(ValueError, match="scores"):
            env.shield_actions(bad)
    with pytest.raises(ValueError, match="tie_break"):
        env.shield_actions(good, tie_break="score")
    with pytest.raises(TypeError, match="priority"):
        env.shield_actions(good, priority=torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="out"):
        env.shield_actions(good, out=(torch.zeros((2, 3), dtype=torch.int64),))


def test_shield_kernel_has_no_scratch():
    """Every instance of pgx_shield.hip's kernel: no scratch, no spills, the planner's LDS (hipcc cross-compiles gfx950).
    The occupant of a sorted candidate is picked with compile-time indices only, so nothing may leave the registers."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or next((c for c in ("/opt/rocm/bin/hipcc",) if os.path.exists(c)), None)
    if hipcc is None:  # an environment reason, as in tests/test_kernel_resources.py
        pytest.skip("no hipcc on this box: the gfx950 resource remarks cannot be produced")
    src = os.path.join(ROOT, "pogema_amd", "csrc", "pgx_shield.hip")
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
    shield = {n: u for n, u in kernels.items() if "shield_kernel" in n}
    assert len(shield) == 18, sorted(kernels)         # 256 / 1024 lanes x 3 score types x (no field, 16- / 32-bit fields)
    for n, u in shield.items():
        print(n, u)
        assert u["ScratchSize"] == 0 and u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (n, u)
        assert u["LDS Size"] in (40 * 256 + 256, 40 * 1024 + 256), (n, u)     # 40 bytes per lane + 256, as the planner
