"""CPU: the multi-step planner's reference (tests/pibt_plan_reference.py, docs/SPEC.md S16) on cases worked by hand, the
guarantees of S13 on every step of random lookaheads, the C-ABI of the feature (pgx_pibt_plan and its two constants
declared, exported and bound; argument checks answered without a device) and the Python argument checks that need no
engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from pibt_plan_reference import pibt_plan_env
from pibt_reference import check_invariants, pibt_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STAY, UP, DOWN, LEFT, RIGHT = 0, 1, 2, 3, 4
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def _grid(text):
    return np.array([[c == "#" for c in row] for row in text.split()], dtype=np.uint8)


def _plan(text, agents, targets, horizon, active=None, **kw):
    active = [1] * len(agents) if active is None else active
    actions, path, arrival, prio, planned = pibt_plan_env(_grid(text), agents, targets, active, horizon, **kw)
    A = len(agents)
    assert actions.dtype == np.int64 and actions.shape == (horizon, A)
    assert path.dtype == np.int32 and path.shape == (horizon, A, 2)
    assert arrival.dtype == np.int32 and prio.dtype == np.int32 and planned.shape == (horizon + 1, A)
    return actions.tolist(), [[tuple(v) for v in row] for row in path.tolist()], arrival.tolist(), prio.tolist(), planned


def test_head_on_corridor_with_a_bay_resolves_within_the_horizon():
    """tests/test_pibt_gpu.py's corridor (L = 9 cells in row 2, one bay above its cell 6), its bound restated for the
    lookahead: the priorities stay equal until agent 0 arrives, so 0 plans first and moves right in every step and
    stands on its target after exactly L - 1 = 8 steps; agent 1 then needs at most L more."""
    L = 9
    text = "#" * L + " ######.## " + "." * L
    agents, targets = [(2, 0), (2, L - 1)], [(2, L - 1), (2, 0)]
    K = 2 * L - 1
    actions, path, arrival, prio, planned = _plan(text, agents, targets, K)
    assert [a[0] for a in actions[:L - 1]] == [RIGHT] * (L - 1)
    assert arrival[0] == L - 1 and L - 1 < arrival[1] <= K
    assert path[arrival[1] - 1][1] == (2, 0) and path[K - 1] == [(2, L - 1), (2, 0)]
    assert (1, 6) in [p[1] for p in path], "agent 1 never used the bay"
    assert planned[:L - 1, 0].all() and not planned[L - 1:, 0].any()          # finish: 0 is hidden once it has arrived
    assert planned[:arrival[1], 1].all() and not planned[arrival[1]:, 1].any()
    assert prio == [0, 0]
    pos = np.array(agents)
    for h in range(K):
        assert check_invariants(_grid(text), pos, planned[h], np.array(path[h])) == [], h
        pos = np.array(path[h])
    # a horizon that ends before the meeting is resolved: nobody has arrived, the priorities have grown in step
    _, _, arrival, prio, _ = _plan(text, agents, targets, 5)
    assert arrival == [-1, -1] and prio == [5, 5]


def test_an_arrived_agent_frees_its_cell_for_a_follower_under_finish():
    agents, targets = [(0, 1), (0, 0)], [(0, 2), (0, 2)]       # 1 follows 0 to the same target
    actions, path, arrival, prio, planned = _plan("...", agents, targets, 3, on_target="finish")
    assert actions == [[RIGHT, RIGHT], [STAY, RIGHT], [STAY, STAY]]
    assert path == [[(0, 2), (0, 1)], [(0, 2), (0, 2)], [(0, 2), (0, 2)]]
    assert arrival == [1, 2] and prio == [0, 0]
    assert planned.tolist() == [[True, True], [False, True], [False, False], [False, False]]
    # nothing / restart: 0 stays planned on the target and cannot be pushed off it (its only other cell is its
    # caller's), so 1 waits next to it and its priority keeps growing
    for mode in ("nothing", "restart"):
        actions, path, arrival, prio, planned = _plan("...", agents, targets, 3, on_target=mode)
        assert actions == [[RIGHT, RIGHT], [STAY, STAY], [STAY, STAY]], mode
        assert path == [[(0, 2), (0, 1)]] * 3
        assert arrival == [1, -1] and prio == [0, 3] and planned.all()


def test_arrival_counts_from_the_current_cell_and_skips_unplanned_agents():
    # 0 stands on its target already; 1 is inactive (on its target or not); 2 walks two cells
    agents, targets = [(0, 0), (1, 1), (2, 0)], [(0, 0), (1, 1), (2, 2)]
    actions, path, arrival, prio, planned = _plan("... ... ...", agents, targets, 3, active=[1, 0, 1], on_target="nothing",
                                                  priority=[4, 4, 4])
    assert arrival == [0, -1, 2]
    assert [row[1] for row in actions] == [STAY] * 3 and [row[1] for row in path] == [(1, 1)] * 3
    assert prio == [0, 0, 0]                                    # on the target, not planned, arrived
    assert planned[:, 0].all() and not planned[:, 1].any()


def test_horizon_one_is_the_one_step_planner():
    rng = np.random.default_rng(5)
    for case in range(30):
        H, W = (int(v) for v in rng.integers(3, 9, size=2))
        obstacles = (rng.random((H, W)) < 0.2).astype(np.uint8)
        free = np.argwhere(obstacles == 0)
        if len(free) < 2:
            continue
        A = int(rng.integers(1, min(len(free), 12) + 1))
        pos = free[rng.permutation(len(free))[:A]]
        tgt = free[rng.integers(0, len(free), size=A)]
        active = rng.random(A) < 0.85
        prio = None if case % 3 == 0 else rng.integers(-5, 6, size=A)
        want_a, want_n = pibt_env(obstacles, pos, tgt, active, prio)
        for mode in ("finish", "nothing"):
            actions, path, _, _, planned = pibt_plan_env(obstacles, pos, tgt, active, 1, prio, on_target=mode)
            assert np.array_equal(actions[0], want_a) and np.array_equal(path[0], want_n), (case, mode)
            assert np.array_equal(planned[0], active)


def test_memoised_fields_are_bfs_from():
    """The reference's shared distance fields (all targets of a map in one pass) against expert_reference.bfs_from."""
    import pibt_plan_reference as R
    from expert_reference import bfs_from
    rng = np.random.default_rng(8)
    for case in range(12):
        H, W = (int(v) for v in rng.integers(1, 12, size=2))
        blocked = rng.random((H, W)) < 0.3
        targets = [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(6)]    # obstacles among them
        R._prefill(blocked, targets[:4])
        for x, y in targets:                                     # four from the pass, two computed on demand
            got = R._bfs_memo(blocked, x, y)
            want = bfs_from(blocked, x, y)
            assert got.dtype == want.dtype and np.array_equal(got, want), (case, x, y)


def test_priorities_grow_reset_and_wrap():
    run = lambda K, **kw: _plan(".....", [(0, 0)], [(0, 4)], K, **kw)[3]
    assert run(1) == [1] and run(3) == [3]
    assert run(4) == [0] and run(6) == [0]                       # the fourth step's next cell is the target
    assert run(3, priority=[-7]) == [-4]
    assert run(1, priority=[I32_MAX]) == [I32_MIN]               # two's-complement wrap
    assert run(2, priority=[I32_MAX]) == [I32_MIN + 1]
    assert run(3, priority=[9], growing=False) == [9] and run(6, priority=[9], growing=False) == [9]
    assert run(2, priority=[9], active=[0]) == [0]               # not planned
    assert run(2, priority=[9], active=[0], growing=False) == [9]
    # "nothing": the agent keeps standing on its target with priority 0 (it is reset in every step, not once)
    assert run(8, on_target="nothing") == [0]
    # the priorities decide inside the lookahead as they do in one step: 1 outranks 0 from the second step on
    # because 0 reached its own target (reset to 0) while 1 was held up
    actions, path, arrival, prio, _ = _plan("...", [(0, 1), (0, 0)], [(0, 2), (0, 2)], 2, on_target="nothing", priority=[3, 0])
    assert prio == [0, 2] and arrival == [1, -1]


def test_guarantees_on_every_step_of_random_lookaheads():
    rng = np.random.default_rng(2025)
    moved = arrived = 0
    for case in range(40):
        H, W = (int(v) for v in rng.integers(3, 10, size=2))
        obstacles = (rng.random((H, W)) < 0.25).astype(np.uint8)
        free = np.argwhere(obstacles == 0)
        if len(free) < 2:
            continue
        A = int(rng.integers(1, min(len(free), 19) + 1))
        pos = free[rng.permutation(len(free))[:A]].copy()
        tgt = free[rng.permutation(len(free))[:A]]
        active = rng.random(A) < 0.9
        prio = None if case % 3 == 0 else rng.integers(-2, 3, size=A)
        mode = ("finish", "nothing", "restart")[case % 3]
        K = 12
        actions, path, arrival, prio_out, planned = pibt_plan_env(obstacles, pos, tgt, active, K, prio, on_target=mode,
                                                                  growing=case % 4 != 3)
        assert np.array_equal(planned[0], active)
        cur = pos
        for h in range(K):
            assert check_invariants(obstacles, cur, planned[h], path[h]) == [], (case, h)
            idle = ~planned[h]
            assert (actions[h][idle] == 0).all() and (path[h][idle] == cur[idle]).all()
            if mode == "finish":
                assert np.array_equal(planned[h + 1], planned[h] & ~(path[h] == tgt).all(axis=1))
            else:
                assert np.array_equal(planned[h + 1], planned[h])
            moved += int((actions[h] != 0).sum())
            cur = path[h]
        # arrival restated: the first h whose position is the target
        trace = np.concatenate([pos[None].astype(np.int32), path])
        for i in range(A):
            on = [h for h in range(K + 1) if active[i] and tuple(trace[h, i]) == tuple(tgt[i])]
            assert arrival[i] == (on[0] if on else -1), (case, i)
        arrived += int((arrival > 0).sum())
    assert moved > 500 and arrived > 50, (moved, arrived)


def test_header_declares_and_library_exports(engine_lib):
    from pogema_amd import _lib
    raw = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+pgx_pibt_plan\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+flags\s*,\s*int32_t\s+horizon\s*,"
                     r"\s*const\s+int32_t\s*\*\s*priority\s*,\s*void\s*\*\s*actions\s*,\s*int32_t\s+action_dtype\s*,"
                     r"\s*int32_t\s*\*\s*path_xy\s*,\s*int32_t\s*\*\s*arrival\s*,\s*int32_t\s*\*\s*priority_out\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"#define\s+PGX_PLAN_FIXED_PRIORITY\s+1\s", text)
    assert re.search(r"#define\s+PGX_MAX_PLAN_HORIZON\s+256\s", text)
    assert _lib.MAX_PLAN_HORIZON == 256 and _lib.PLAN_FIXED_PRIORITY == 1
    assert "pgx_pibt_plan" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_pibt_plan")
    assert engine_lib.pgx_pibt_plan.argtypes is not None and len(engine_lib.pgx_pibt_plan.argtypes) == 10
    # the ABI number did not move: the entry point is an addition
    assert re.search(r"#define\s+PGX_ABI_VERSION\s+6\s", text) and engine_lib.pgx_abi_version() == 6


def test_argument_checks_need_no_device(engine_lib):
    """PGX_E_INVALID (-1) with a message naming the argument; the checks run before the handle is looked at."""
    call = engine_lib.pgx_pibt_plan
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
        assert b"pgx_pibt_plan" in msg and word in msg, (args, msg)
    # valid arguments (both ends of the horizon's range, the flag), no handle: refused by the shared entry prologue
    for flags, horizon in ((0, 1), (1, 256)):
        assert call(N, flags, horizon, N, ptr, 2, N, N, N, N) == -1
        assert b"pgx_pibt_plan" in engine_lib.pgx_last_error() and b"handle" in engine_lib.pgx_last_error()


class _NoEngine:
    """A QueryMixin without an engine behind it: whatever reaches the library fails on the missing attributes."""
    batch, num_agents, window, device = 3, 5, 7, torch.device("cpu")
    _ACTION_CODE = {torch.int8: 0, torch.int32: 1, torch.int64: 2}


def _no_engine():
    from pogema_amd.queries import QueryMixin
    return type("NoEngine", (_NoEngine, QueryMixin), {})()


def _outs(K=4, B=3, A=5, dtype=torch.int64):
    return [torch.zeros((K, B, A), dtype=dtype), torch.zeros((K, B, A, 2), dtype=torch.int32),
            torch.zeros((B, A), dtype=torch.int32), torch.zeros((B, A), dtype=torch.int32)]


@pytest.mark.parametrize("horizon", [0, -1, 257, 2.0, "4", None, True, np.float32(3)])
def test_a_bad_horizon_is_refused(horizon):
    with pytest.raises(ValueError, match="horizon must be an integer in 1..256"):
        _no_engine().pibt_plan(horizon)


def test_python_argument_checks_need_no_engine():
    env = _no_engine()
    names = r"\(actions, path_xy, arrival, priority\)"
    for n in (1, 2, 3, 5):
        with pytest.raises(ValueError, match="out must be " + names):
            env.pibt_plan(4, out=tuple(_outs()[:1] * n))
    for k, name in enumerate(("actions", "path_xy", "arrival", "priority")):
        out = _outs()
        out[k] = None
        with pytest.raises(ValueError, match=rf"out\[{name}\] is None"):
            env.pibt_plan(4, out=tuple(out))
    bad = {
        "actions": [torch.zeros((4, 3, 5), dtype=torch.float32), torch.zeros((3, 3, 5), dtype=torch.int64),
                    torch.zeros((3, 5), dtype=torch.int64), torch.zeros((4, 3, 10), dtype=torch.int64)[..., ::2]],
        "path_xy": [torch.zeros((4, 3, 5, 2), dtype=torch.int64), torch.zeros((4, 3, 5), dtype=torch.int32),
                    torch.zeros((3, 5, 2), dtype=torch.int32)],
        "arrival": [torch.zeros((3, 5), dtype=torch.int64), torch.zeros((4, 3, 5), dtype=torch.int32)],
        "priority": [torch.zeros((3, 5), dtype=torch.int16), torch.zeros((5, 3), dtype=torch.int32)],
    }
    for k, name in enumerate(("actions", "path_xy", "arrival", "priority")):
        for t in bad[name]:
            out = _outs()
            out[k] = t
            with pytest.raises(ValueError, match=rf"out\[{name}\] must be a contiguous"):
                env.pibt_plan(4, out=tuple(out))
    with pytest.raises(ValueError, match="dtype"):
        env.pibt_plan(4, dtype=torch.float32)
    with pytest.raises(ValueError, match="priority"):
        env.pibt_plan(4, priority=torch.zeros((3, 6), dtype=torch.int32))
    with pytest.raises(TypeError, match="priority"):
        env.pibt_plan(4, priority=torch.zeros((3, 5), dtype=torch.float32))
    # every check passed: the call reaches for the library, which this stand-in does not have
    for dtype in (torch.int8, torch.int32, torch.int64):
        with pytest.raises(AttributeError, match="_lib"):
            env.pibt_plan(4, out=tuple(_outs(dtype=dtype)))
    with pytest.raises(AttributeError, match="_lib"):
        env.pibt_plan(np.int64(256), priority=torch.zeros((3, 5), dtype=torch.int64), growing=False)


def test_policy_plan_passes_and_keeps_the_priorities():
    """PibtPolicy.plan hands `self.priority` to pibt_plan and stores the priorities the lookahead ends with."""
    from pogema_amd import PibtPolicy

    class Env:
        batch, num_agents, device = 2, 3, torch.device("cpu")

        def pibt_plan(self, horizon, priority=None, growing=True, dtype=torch.int64, out=None):
            self.seen = (horizon, priority.clone(), growing, dtype, out)
            return "actions", "path", "arrival", priority + horizon

    env = Env()
    policy = PibtPolicy(env)
    policy.priority += 2
    assert policy.plan(5, dtype=torch.int8) == ("actions", "path", "arrival")
    assert env.seen[0] == 5 and env.seen[2] is True and env.seen[3] == torch.int8 and env.seen[4] is None
    assert torch.equal(env.seen[1], torch.full((2, 3), 2, dtype=torch.int32))
    assert torch.equal(policy.priority, torch.full((2, 3), 7, dtype=torch.int32))


def test_horizon_kernel_has_no_scratch():
    """Every instance of pgx_pibt_horizon.hip's kernel: no scratch, no spills (hipcc cross-compiles gfx950) -- what the
    lanes carry from step to step stays in registers."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or next((c for c in ("/opt/rocm/bin/hipcc",) if os.path.exists(c)), None)
    if hipcc is None:  # an environment reason, as in tests/test_kernel_resources.py
        pytest.skip("no hipcc on this box: the gfx950 resource remarks cannot be produced")
    src = os.path.join(ROOT, "pogema_amd", "csrc", "pgx_pibt_horizon.hip")
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
    plan = {n: u for n, u in kernels.items() if "pibt_horizon_kernel" in n}
    assert len(plan) == 4, sorted(kernels)            # 256 / 1024 lanes x 16- / 32-bit fields
    for n, u in plan.items():
        print(n, u)
        assert u["ScratchSize"] == 0 and u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (n, u)
        assert u["LDS Size"] <= 64 * 1024, (n, u)     # static LDS: fits every device default, no opt-in needed
