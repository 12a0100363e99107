"""CPU: the reference of the multi-step planner with the swap operation (tests/pibt_swap_plan_reference.py, docs/SPEC.md
S27) on the hand-built instances and on the states the GPU suite installs, its relation to the one-step reference and to
the plain plan, the C-ABI of the feature (pgx_pibt_swap_plan declared with its exact prototype, exported, argument checks
answered without a device), the Python keywords, and the resources of the kernel's instances."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pibt_plan_reference import pibt_plan_env, pibt_plan_reference
from pibt_reference import check_invariants
from pibt_swap_cases import CLEAR, DEAD_END, DEAD_END_INSIDE, RING, grid, head_on_instances, solve_suite
from pibt_swap_plan_cases import LATE_MIN, agreement_case, case_counts, meets, plan_case
from pibt_swap_plan_reference import late, pibt_swap_plan_env, pibt_swap_plan_reference
from pibt_swap_reference import COUNTERS, pibt_swap_env
from test_visible_agents_gpu import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))


# ---- hand-built instances ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_target", ["finish", "nothing"])
@pytest.mark.parametrize("name,instance,first", [("dead end", DEAD_END, 1), ("dead end, inside", DEAD_END_INSIDE, 0)])
def test_dead_end_plans_arrive_where_the_plain_plan_does_not(name, instance, first, on_target):
    """K = 9: both agents arrive, in steps 9 and 8 -- what run_policy needs nine steps for
    (test_pibt_swap.py::test_dead_end_is_solved_in_nine_steps...) -- and the lists are reversed at the steps after the
    first: 1..3 from the mouth of the dead end, 0..3 from inside it."""
    rows, agents, targets = instance
    actions, path, arrival, prio, planned, count = pibt_swap_plan_env(grid(rows), agents, targets, [1, 1], 9,
                                                                       on_target=on_target)
    assert actions.dtype == np.int64 and path.dtype == np.int32 and arrival.dtype == np.int32 and prio.dtype == np.int32
    assert arrival.tolist() == [9, 8]
    assert pibt_plan_env(grid(rows), agents, targets, [1, 1], 9, on_target=on_target)[2].tolist() == [-1, -1]
    steps = [1 if first <= h <= 3 else 0 for h in range(9)]
    assert count["reversed"].tolist() == count["usual"].tolist() == count["pulled"].tolist() == steps
    assert count["clear"].tolist() == [0] * 9
    assert actions.tolist() == [[4, 0] if first else [3, 3], [3, 3], [3, 3], [3, 3], [4, 1], [4, 2], [4, 3], [4, 3], [4, 0]]
    assert [tuple(v) for v in path[-1].tolist()] == list(targets) and prio.tolist() == [0, 0]
    assert set(count) == set(COUNTERS) and all(v.shape == (9,) for v in count.values())


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_clear_livelocks_through_a_plan(on_target):
    """S23's documented livelock: the pusher steps aside and back for ever, where the plain plan arrives."""
    rows, agents, targets = CLEAR
    out = pibt_swap_plan_env(grid(rows), agents, targets, [1, 1], 6, on_target=on_target)
    assert out[2].tolist() == [-1, -1] and out[0].tolist() == [[1, 0], [2, 0]] * 3
    assert out[5]["clear"].tolist() == [1, 0] * 3 and out[5]["pulled"].tolist() == [0] * 6
    plain = pibt_plan_env(grid(rows), agents, targets, [1, 1], 6, on_target=on_target)
    assert plain[2].tolist() == ([1, 4] if on_target == "finish" else [1, -1])


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_ring_equals_the_plain_plan(on_target):
    rows, agents, targets = RING
    out = pibt_swap_plan_env(grid(rows), agents, targets, [1, 1, 1], 6, on_target=on_target)
    assert int(out[5]["reversed"].sum()) == 0 and int(out[5]["longest_walk"].max()) > 0
    assert _equal(out, pibt_plan_env(grid(rows), agents, targets, [1, 1, 1], 6, on_target=on_target))
    assert out[2].tolist() == [1, 3, 4]


# ---- properties ----------------------------------------------------------------------------------------------------
def test_horizon_one_is_the_one_step_reference():
    obstacles, agents, targets, _ = head_on_instances(12, 10, 8, seed=5)
    rng = np.random.default_rng(5)
    active = rng.random(agents.shape[:2]) < 0.85
    differ = 0
    for b in range(12):
        prio = None if b % 3 == 0 else rng.integers(-2, 3, size=8)
        a, n, count = pibt_swap_env(obstacles[b], agents[b], targets[b], active[b], prio)
        out = pibt_swap_plan_env(obstacles[b], agents[b], targets[b], active[b], 1, prio)
        assert np.array_equal(out[0][0], a) and np.array_equal(out[1][0], n)
        assert all(int(out[5][name][0]) == count[name] for name in COUNTERS)
        assert np.array_equal(out[4][0], active[b])
        differ += int(count["reversed"] > 0)
    assert differ >= 5, differ


def test_guarantees_at_every_step_and_plain_equality_without_a_reversal():
    """Random corridor instances under all three modes and both priority rules: S13's guarantees at every step on the
    positions and planned flags of that step, unplanned agents stay, `planned` follows S16, arrival restated; an env in
    which no list is reversed at any step equals the plain plan."""
    quiet = loud = late_loud = 0
    for case, (obstacles, pos, tgt) in enumerate(solve_suite(n=45, size=12, density=0.35, agents=12, seed=4, min_cells=30)):
        rng = np.random.default_rng(case)
        active = rng.random(12) < 0.9
        prio = None if case % 3 == 0 else rng.integers(-2, 3, size=12)
        mode, growing, K = ("finish", "nothing", "restart")[case % 3], case % 4 != 3, 12
        out = pibt_swap_plan_env(obstacles, pos, tgt, active, K, prio, on_target=mode, growing=growing)
        actions, path, arrival, prio_out, planned, count = out
        assert np.array_equal(planned[0], active)
        cur = pos
        for h in range(K):
            assert check_invariants(obstacles, cur, planned[h], path[h]) == [], (case, h)
            idle = ~planned[h]
            assert (actions[h][idle] == 0).all() and (path[h][idle] == cur[idle]).all()
            want = planned[h] & ~(path[h] == tgt).all(axis=1) if mode == "finish" else planned[h]
            assert np.array_equal(planned[h + 1], want)
            cur = path[h]
        trace = np.concatenate([pos[None].astype(np.int32), path])
        for i in range(12):
            on = [h for h in range(K + 1) if active[i] and tuple(trace[h, i]) == tuple(tgt[i])]
            assert arrival[i] == (on[0] if on else -1), (case, i)
        plain = pibt_plan_env(obstacles, pos, tgt, active, K, prio, on_target=mode, growing=growing)
        if int(count["reversed"].sum()) == 0:
            quiet += 1
            assert _equal(out, plain), case
        else:
            loud += 1
            late_loud += late(count, "reversed") > 0
            h = int(np.argmax(count["reversed"] > 0))       # up to the first reversal the two plans are one
            assert np.array_equal(actions[:h], plain[0][:h]) and np.array_equal(planned[:h + 1], plain[4][:h + 1])
    assert quiet >= 8 and loud >= 8 and late_loud >= 5, (quiet, loud, late_loud)


def test_batched_wrapper():
    obstacles, pos, tgt = agreement_case()
    active = np.ones(pos.shape[:2], dtype=bool)
    prio = np.random.default_rng(1).integers(-3, 4, size=pos.shape[:2])
    for p in (None, prio):
        out = pibt_swap_plan_reference(obstacles, pos, tgt, active, 5, p, on_target="nothing")
        assert [v.shape for v in out[:5]] == [(5, 24, 8), (5, 24, 8, 2), (24, 8), (24, 8), (6, 24, 8)]
        assert set(out[5]) == set(COUNTERS) and all(v.shape == (5, 24) for v in out[5].values())
        for b in (0, 7, 23):
            one = pibt_swap_plan_env(obstacles[b], pos[b], tgt[b], active[b], 5, None if p is None else p[b], "nothing")
            assert all(np.array_equal(o[:, b] if k in (0, 1, 4) else o[b], w) for k, (o, w) in enumerate(zip(out[:5], one)))
            assert all(np.array_equal(out[5][name][:, b], one[5][name]) for name in COUNTERS)
        quiet = out[5]["reversed"].sum(axis=0) == 0
        plain = pibt_plan_reference(obstacles, pos, tgt, active, 5, p, on_target="nothing")
        assert quiet.any() and not quiet.all()
        assert np.array_equal(out[0][:, quiet], plain[0][:, quiet]) and np.array_equal(out[3][quiet], plain[3][quiet])


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_agreement_states_reverse_lists_late(on_target):
    """The corridor states of the GPU suite's agreement test: the reference alone reverses lists at steps h >= 1."""
    obstacles, pos, tgt = agreement_case()
    out = pibt_swap_plan_reference(obstacles, pos, tgt, np.ones(pos.shape[:2], dtype=bool), 12, on_target=on_target)
    assert late(out[5], "reversed") >= 5 and late(out[5], "pulled") >= 5


@pytest.mark.parametrize("agents,size,batch", [row for row in LAYOUTS if row[0] <= 200])
def test_layout_states_exercise_the_rule_late(agents, size, batch):
    """The states the GPU suite installs per lane layout, up to 200 agents (the larger ones were counted once, see
    LATE_MIN): the reference alone reports exactly the recorded late counts, and every state fits the case's limits."""
    for obstacles, pos, tgt, prio, side, r, K in plan_case(agents, size, batch):
        assert pos.shape[0] <= 24 and pos.shape[1] == agents and obstacles.shape[1:] == (side, side) and K >= 6
        assert prio.dtype == np.int32 and prio.shape == pos.shape[:2]
    total = case_counts(agents, size, batch)
    assert meets(total, agents) == [], (total, LATE_MIN[agents])
    assert all(total[name] == least for name, least in LATE_MIN[agents].items()), (total, LATE_MIN[agents])
    if agents == 1:
        assert total["reversed"] == 0 and total["first"]["reversed"] == 0


def test_every_layout_has_a_minimum():
    assert set(LATE_MIN) == {row[0] for row in LAYOUTS}
    assert all(LATE_MIN[a].get("reversed", 0) >= 1 for a in LATE_MIN if a > 1)


# ---- C-ABI -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports(engine_lib):
    from pogema_amd import _lib
    raw = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+pgx_pibt_swap_plan\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+flags\s*,\s*int32_t\s+horizon\s*,"
                     r"\s*const\s+int32_t\s*\*\s*priority\s*,\s*void\s*\*\s*actions\s*,\s*int32_t\s+action_dtype\s*,"
                     r"\s*int32_t\s*\*\s*path_xy\s*,\s*int32_t\s*\*\s*arrival\s*,\s*int32_t\s*\*\s*priority_out\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert "pgx_pibt_swap_plan" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_pibt_swap_plan")
    assert engine_lib.pgx_pibt_swap_plan.argtypes is not None and len(engine_lib.pgx_pibt_swap_plan.argtypes) == 10
    assert list(engine_lib.pgx_pibt_swap_plan.argtypes) == list(engine_lib.pgx_pibt_plan.argtypes)
    # the ABI number did not move: the entry point is an addition
    assert re.search(r"#define\s+PGX_ABI_VERSION\s+6\s", text) and engine_lib.pgx_abi_version() == 6


def test_argument_checks_need_no_device(engine_lib):
    """tests/test_pibt_plan.py's table against the new name: PGX_E_INVALID (-1) with a message naming the entry point
    and the argument; the checks run before the handle is looked at."""
    call = engine_lib.pgx_pibt_swap_plan
    buf = C.create_string_buffer(64)
    ptr = (C.addressof(buf) + 15) // 16 * 16       # a 16-byte aligned address that is never dereferenced
    N = None
    for args, word in (((N, 0, 4, N, N, 2, N, N, N, N), b"actions"),
                       ((N, 2, 4, N, ptr, 2, N, N, N, N), b"flags"),
                       ((N, -8, 4, N, ptr, 2, N, N, N, N), b"flags"),
                       ((N, 0, 0, N, ptr, 2, N, N, N, N), b"horizon"),
                       ((N, 1, -1, N, ptr, 2, N, N, N, N), b"horizon"),
                       ((N, 0, 257, N, ptr, 2, N, N, N, N), b"horizon"),
                       ((N, 0, 4, N, ptr, 3, N, N, N, N), b"action_dtype"),
                       ((N, 0, 4, N, ptr, -1, N, N, N, N), b"action_dtype"),
                       ((N, 0, 4, N, ptr + 4, 2, N, N, N, N), b"actions"),
                       ((N, 0, 4, ptr + 2, ptr, 0, N, N, N, N), b"priority"),
                       ((N, 0, 4, N, ptr, 0, ptr + 1, N, N, N), b"path_xy"),
                       ((N, 0, 4, N, ptr, 0, N, ptr + 2, N, N), b"arrival"),
                       ((N, 0, 4, N, ptr, 0, N, N, ptr + 3, N), b"priority_out")):
        assert call(*args) == -1, args
        msg = engine_lib.pgx_last_error()
        assert b"pgx_pibt_swap_plan" in msg and word in msg, (args, msg)
    # valid arguments (both ends of the horizon's range, the flag), no handle: refused by the shared entry prologue
    for flags, horizon in ((0, 1), (1, 256)):
        assert call(N, flags, horizon, N, ptr, 2, N, N, N, N) == -1
        assert b"pgx_pibt_swap_plan" in engine_lib.pgx_last_error() and b"handle" in engine_lib.pgx_last_error()


# ---- Python ----------------------------------------------------------------------------------------------------------
def test_swap_is_a_keyword_with_default_false():
    from pogema_amd import PibtPolicy, Pogema, VecPogema
    sig = inspect.signature(VecPogema.pibt_plan)
    assert sig.parameters["swap"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["swap"].default is False
    assert list(sig.parameters)[:6] == ["self", "horizon", "priority", "growing", "dtype", "out"]
    assert inspect.signature(Pogema.pibt_plan).parameters["swap"].default is False
    assert list(inspect.signature(Pogema.pibt_plan).parameters) == ["self", "horizon", "priority", "swap"]
    p = inspect.signature(PibtPolicy.plan).parameters["swap"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_swap_must_be_a_bool():
    from pogema_amd.queries import QueryMixin

    class NoEngine(QueryMixin):
        batch, num_agents, window, device = 3, 5, 7, torch.device("cpu")
        _ACTION_CODE = {torch.int8: 0, torch.int32: 1, torch.int64: 2}

    for bad in (1, 0, "yes", None):
        with pytest.raises(TypeError, match="swap"):
            NoEngine().pibt_plan(4, swap=bad)
    with pytest.raises(TypeError):
        NoEngine().pibt_plan(4, None, True, torch.int64, None, True)       # keyword-only
    with pytest.raises(ValueError, match="horizon"):                       # the other checks are still made
        NoEngine().pibt_plan(0, swap=True)
    for swap in (True, False, np.bool_(True)):
        with pytest.raises(AttributeError, match="_lib"):                  # fitting arguments reach the library
            NoEngine().pibt_plan(4, swap=swap)


class _Env:
    """What PibtPolicy reads of an env, with a pibt_plan that records its keywords."""
    batch, num_agents, device = 2, 3, torch.device("cpu")

    def pibt_plan(self, horizon, priority=None, growing=True, dtype=torch.int64, out=None, **keywords):
        self.seen = (horizon, priority.clone(), dtype, out, keywords)
        return "actions", "path", "arrival", priority + horizon


@pytest.mark.parametrize("built_with", [False, True])
def test_policy_plan_passes_swap_through_and_keeps_the_priorities(built_with):
    from pogema_amd import PibtPolicy
    for swap in (True, False):
        env = _Env()
        policy = PibtPolicy(env, swap=built_with)
        policy.priority += 2
        assert policy.plan(5, dtype=torch.int8, swap=swap) == ("actions", "path", "arrival")
        assert env.seen[0] == 5 and env.seen[2] == torch.int8 and env.seen[3] is None and env.seen[4] == {"swap": swap}
        assert torch.equal(env.seen[1], torch.full((2, 3), 2, dtype=torch.int32))
        assert torch.equal(policy.priority, torch.full((2, 3), 7, dtype=torch.int32))
    with pytest.raises(TypeError, match="swap"):
        PibtPolicy(_Env(), swap=built_with).plan(5, swap=1)


def test_policy_plan_without_the_keyword():
    """A plain policy passes no `swap` keyword (an env whose pibt_plan has none plans as before); a policy built with
    swap=True still refuses, and says what to call."""
    from pogema_amd import PibtPolicy
    env = _Env()
    assert PibtPolicy(env).plan(3) == ("actions", "path", "arrival") and env.seen[4] == {}
    env = _Env()
    with pytest.raises(ValueError, match=r"multi-step planner.*no swap rule.*plan\(horizon, swap=True\)"):
        PibtPolicy(env, swap=True).plan(3)
    assert not hasattr(env, "seen")


# ---- kernel resources --------------------------------------------------------------------------------------------------
# (lanes, field type) -> (TotalSGPRs, VGPRs, LDS bytes, waves per SIMD) of pibt_swap_horizon_kernel as built for gfx950;
# `t` 16-bit, `j` 32-bit fields.  Measured: 100 SGPRs, 78 VGPRs, 6 waves per SIMD in all four.
RECORDED_BUDGET = {(256, "t"): (102, 80, 13312, 6), (256, "j"): (102, 80, 13312, 6),
                   (1024, "t"): (102, 80, 52480, 6), (1024, "j"): (102, 80, 52480, 6)}


def test_kernels_have_no_scratch_and_stay_inside_their_budget():
    """Every instance of pgx_pibt_swap_horizon.hip's kernel: no scratch, no spills, the recorded register budget, and the
    LDS block the file's header states -- 51 bytes per lane + 256, pibt_swap_kernel's; the largest, 1024 lanes, is
    51.25 KB of the CU's 160 KB and within the 64 KB a static allocation may have."""
    hipcc = shutil.which("hipcc") or next((c for c in ("/opt/rocm/bin/hipcc",) if os.path.exists(c)), None)
    if hipcc is None:  # an environment reason, as in tests/test_kernel_resources.py
        pytest.skip("no hipcc on this box: the gfx950 resource remarks cannot be produced")
    src = os.path.join(ROOT, "pogema_amd", "csrc", "pgx_pibt_swap_horizon.hip")
    header = open(src).read().split("#include", 1)[0]
    m = re.search(r"LDS: 51 bytes per lane \+ 256 \((\d+) B / (\d+) B\), static", header)
    assert m and (int(m.group(1)), int(m.group(2))) == (51 * 256 + 256, 51 * 1024 + 256), "the header's LDS figures"
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
        m = re.search(r"pibt_swap_horizon_kernelILi(\d+)E([tj])E", name)
        assert m, name
        key = (int(m.group(1)), m.group(2))
        seen.add(key)
        sgpr, vgpr, lds, waves = RECORDED_BUDGET[key]
        assert u["TotalSGPRs"] <= sgpr and u["VGPRs"] <= vgpr and u["LDS Size"] == lds, (name, u, RECORDED_BUDGET[key])
        assert u["LDS Size"] == 51 * key[0] + 256 and u["LDS Size"] <= 64 * 1024
        assert u["Occupancy"] >= waves, (name, u)
    assert seen == set(RECORDED_BUDGET)
