"""CPU: the agent-token reference (tests/agent_tokens_reference.py, docs/SPEC.md S21) on hand-built cases; the C-ABI of
the feature (both prototypes declared exactly, the constants equal in the header, _lib and pogema_amd.TOKENS, the length
helper, refusal without a handle; no device needed); the argument checks of VecPogema.agent_tokens() on a QueryMixin
without an engine; TokenHistory on CPU tensors; and the register / scratch / occupancy budget of the kernels (hipcc
cross-compiles gfx950)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from agent_tokens_reference import (ACTION0, ACTION_NONE, BLOCKED, CLIP, GREEDY0, HISTORY, NUM_TOKENS, PAD, SLOT_LEN,
                                    agent_tokens_reference, token_length)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _rows(obstacles, agents, targets, active, r, **kw):
    if kw.get("history") is not None:
        kw["history"] = np.asarray(kw["history"])[None]
    out = agent_tokens_reference(np.asarray(obstacles)[None], np.asarray(agents)[None], np.asarray(targets)[None],
                                 np.asarray(active, dtype=bool)[None], r, **kw)
    assert out.dtype == np.uint8 and out.max() < NUM_TOKENS
    return out[0]


# ---- the reference on hand-built cases -------------------------------------------------------------------------
def test_window_and_goal_entries_clip_at_both_ends():
    """An open 40 x 40 map: the cost to (0, 0) is x + y, the cost to (39, 39) is 78 - x - y, so a window cell (du, dv) is
    du + dv above, or below, the centre -- up to 30 at r = 15."""
    r, w = 15, 31
    rows = _rows(np.zeros((40, 40), int), [(24, 24), (15, 15)], [(0, 0), (39, 39)], [1, 1], r, slots=2)
    assert rows.shape == (2, w * w + 20)
    d = np.arange(w) - r
    rel = d[:, None] + d[None, :]
    assert np.array_equal(rows[0, :w * w].reshape(w, w), np.clip(rel, -20, 20) + 20)
    assert np.array_equal(rows[1, :w * w].reshape(w, w), np.clip(-rel, -20, 20) + 20)
    assert rows[0, 0] == 0 and rows[0, w * w - 1] == 40 and rows[0, r * w + r] == 20
    # slot 0: the agent's own goal, (-24, -24) -> 0 and (+24, +24) -> 40; slot 1: the other's goal seen from here
    assert rows[0, w * w:w * w + 4].tolist() == [20, 20, 0, 0]
    assert rows[1, w * w:w * w + 4].tolist() == [20, 20, 40, 40]
    assert rows[0, w * w + 10:w * w + 14].tolist() == [20 - 9, 20 - 9, 20 + 15, 20 + 15]   # target (39, 39) - (24, 24)
    assert rows[1, w * w + 10:w * w + 14].tolist() == [20 + 9, 20 + 9, 20 - 15, 20 - 15]   # target (0, 0) - (15, 15)


def test_small_case_entry_by_entry():
    """3 x 4, one obstacle, r = 1, three agents, the middle one inactive."""
    grid = [[0, 0, 0, 0],
            [0, 1, 0, 0],
            [0, 0, 0, 0]]
    agents = [(0, 0), (0, 1), (1, 0)]
    targets = [(2, 1), (0, 3), (1, 0)]
    rows = _rows(grid, agents, targets, [1, 0, 1], 1, slots=3, length=9 + 30 + 4,
                 history=[[0, 4, 5, -1, 127], [1, 1, 1, 1, 1], [-128, 2, 3, 1, 0]])
    assert rows.shape == (3, 43)
    # agent 0 at (0, 0), target (2, 1): distances around it  . . .   own = 3; (0, 1) is 4, (1, 0) is 2, (1, 1) an obstacle
    #                                                         . 3 4
    #                                                         . 2 #
    assert rows[0, :9].tolist() == [BLOCKED, BLOCKED, BLOCKED, BLOCKED, 20, 21, BLOCKED, 19, BLOCKED]
    # slot 0: itself; goal (2, 1) - (0, 0); history 0, 4, then three that are no actions; greedy: down only (bit 1)
    assert rows[0, 9:19].tolist() == [20, 20, 22, 21, ACTION0, ACTION0 + 4, ACTION_NONE, ACTION_NONE, ACTION_NONE, GREEDY0 + 2]
    # slot 1: agent 2 at (+1, 0) -- the inactive agent 1, though nearer in the key order, is absent; its goal is its own
    # cell (1, 0), seen from (0, 0); it stands on its target: mask 0
    assert rows[0, 19:29].tolist() == [21, 20, 21, 20, ACTION_NONE, ACTION0 + 2, ACTION0 + 3, ACTION0 + 1, ACTION0, GREEDY0]
    # slot 2: nobody; then the tail
    assert (rows[0, 29:] == PAD).all()
    # the inactive agent: all PAD
    assert (rows[1] == PAD).all()
    # agent 2 on its target: own = 0, every reachable window cell is its distance; mask 0
    assert rows[2, :9].tolist() == [BLOCKED, 21, 22, BLOCKED, 20, BLOCKED, BLOCKED, 21, 22]
    assert rows[2, 9:19].tolist() == [20, 20, 20, 20, ACTION_NONE, ACTION0 + 2, ACTION0 + 3, ACTION0 + 1, ACTION0, GREEDY0]
    assert rows[2, 19:29].tolist() == [19, 20, 21, 21, ACTION0, ACTION0 + 4, ACTION_NONE, ACTION_NONE, ACTION_NONE, GREEDY0 + 2]
    assert (rows[2, 29:] == PAD).all()


def test_one_slot_has_no_neighbour_part_and_none_history_records_nothing():
    grid = np.zeros((3, 3), int)
    rows = _rows(grid, [(1, 1), (1, 2)], [(1, 2), (1, 1)], [1, 1], 1, slots=1)
    assert rows.shape == (2, 9 + 10) and token_length(1, 1) == 19
    # agent 0: target to the right, own = 1
    assert rows[0, :9].tolist() == [22, 21, 20, 21, 20, 19, 22, 21, 20]
    assert rows[0, 9:].tolist() == [20, 20, 20, 21] + [ACTION_NONE] * 5 + [GREEDY0 + 8]
    assert rows[1, 9:].tolist() == [20, 20, 20, 19] + [ACTION_NONE] * 5 + [GREEDY0 + 4]
    same = _rows(grid, [(1, 1), (1, 2)], [(1, 2), (1, 1)], [1, 1], 1, slots=1, history=np.full((2, 5), -1))
    assert np.array_equal(rows, same)


def test_unreachable_target_blocks_the_window_but_not_the_goal():
    grid = [[0, 1, 0],
            [0, 1, 0],
            [0, 1, 0]]
    rows = _rows(grid, [(1, 0)], [(0, 2)], [1], 1, slots=2, length=32)
    assert (rows[0, :9] == BLOCKED).all()
    assert rows[0, 9:19].tolist() == [20, 20, 19, 22] + [ACTION_NONE] * 5 + [GREEDY0]
    assert (rows[0, 19:] == PAD).all() and rows.shape == (1, 32)


def test_vocabulary_is_the_documented_one():
    assert (CLIP, BLOCKED, ACTION_NONE, ACTION0, GREEDY0, PAD, NUM_TOKENS, HISTORY, SLOT_LEN) == (20, 41, 42, 43, 48, 64, 65, 5, 10)
    assert token_length(5, 13) == 251


# ---- header, library, package ------------------------------------------------------------------------------------
HEADER_CONSTANTS = {"PGX_TOKEN_CLIP": ("TOKEN_CLIP", "CLIP", 20), "PGX_TOKEN_BLOCKED": ("TOKEN_BLOCKED", "BLOCKED", 41),
                    "PGX_TOKEN_ACTION_NONE": ("TOKEN_ACTION_NONE", "ACTION_NONE", 42),
                    "PGX_TOKEN_ACTION0": ("TOKEN_ACTION0", "ACTION0", 43), "PGX_TOKEN_GREEDY0": ("TOKEN_GREEDY0", "GREEDY0", 48),
                    "PGX_TOKEN_PAD": ("TOKEN_PAD", "PAD", 64), "PGX_NUM_TOKENS": ("NUM_TOKENS", "NUM_TOKENS", 65),
                    "PGX_TOKEN_HISTORY": ("TOKEN_HISTORY", "HISTORY", 5), "PGX_TOKEN_SLOT_LEN": ("TOKEN_SLOT_LEN", "SLOT_LEN", 10),
                    "PGX_MAX_TOKEN_SLOTS": ("MAX_TOKEN_SLOTS", "MAX_SLOTS", 32),
                    "PGX_MAX_TOKEN_LENGTH": ("MAX_TOKEN_LENGTH", "MAX_LENGTH", 2048)}


def test_header_declares_and_library_exports(engine_lib):
    import pogema_amd
    from pogema_amd import _lib
    raw = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+pgx_agent_tokens\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+slots\s*,\s*int32_t\s+length\s*,"
                     r"\s*int32_t\s+flags\s*,\s*const\s+int8_t\s*\*\s*history\s*,\s*uint8_t\s*\*\s*tokens\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", text)
    assert re.search(r"int64_t\s+pgx_agent_tokens_length\s*\(\s*int32_t\s+obs_radius\s*,\s*int32_t\s+slots\s*\)\s*;", text)
    for name, (lib_name, key, value) in HEADER_CONSTANTS.items():
        m = re.search(rf"#define\s+{name}\s+(\d+)\s", text)
        assert m and int(m.group(1)) == value, name
        assert getattr(_lib, lib_name) == value and pogema_amd.TOKENS[key] == value, name
    assert set(pogema_amd.TOKENS) == {key for _, key, _ in HEADER_CONSTANTS.values()}
    for sym in ("pgx_agent_tokens", "pgx_agent_tokens_length"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(engine_lib, sym)
    # the ABI number did not move: the entry points are additions
    assert re.search(r"#define\s+PGX_ABI_VERSION\s+6\s", text) and engine_lib.pgx_abi_version() == 6
    # refused without a handle (no device needed)
    assert engine_lib.pgx_agent_tokens(None, 13, 256, 0, None, None, None) == -1
    assert b"pgx_agent_tokens" in engine_lib.pgx_last_error()


def test_length_helpers_agree(engine_lib):
    import pogema_amd
    for r in range(1, 16):
        for slots in (1, 13, 32):
            want = (2 * r + 1) ** 2 + 10 * slots
            assert pogema_amd.token_length(r, slots) == engine_lib.pgx_agent_tokens_length(r, slots) == want
            assert want <= 2048
    for r, slots in ((0, 13), (16, 13), (5, 0), (5, 33)):
        assert engine_lib.pgx_agent_tokens_length(r, slots) == -1
        assert b"pgx_agent_tokens_length" in engine_lib.pgx_last_error()
        with pytest.raises(ValueError, match=r"1\.\."):
            pogema_amd.token_length(r, slots)
    for bad in (True, 2.0, "5"):
        with pytest.raises(ValueError):
            pogema_amd.token_length(bad, 13)
        with pytest.raises(ValueError):
            pogema_amd.token_length(5, bad)


# ---- argument checks without an engine ---------------------------------------------------------------------------
def _no_engine():
    from pogema_amd.queries import QueryMixin

    class NoEngine(QueryMixin):
        """A QueryMixin without an engine behind it: whatever reaches the library fails on the missing attributes."""
        batch, num_agents, window, device = 3, 5, 7, CPU

    return NoEngine()


L0 = 49 + 130   # window 7, 13 slots


def test_fitting_arguments_reach_the_library():
    with pytest.raises(AttributeError):
        _no_engine().agent_tokens()
    with pytest.raises(AttributeError):
        _no_engine().agent_tokens(slots=32, length=2048, history=torch.zeros((3, 5, 5), dtype=torch.int8),
                                  out=torch.zeros((3, 5, 2048), dtype=torch.uint8))


@pytest.mark.parametrize("slots", [0, 33, True, 2.0])
def test_bad_slots(slots):
    with pytest.raises(ValueError, match=r"slots.*1\.\.32"):
        _no_engine().agent_tokens(slots=slots)


@pytest.mark.parametrize("length", [L0 - 1, 2049, 256.0, True])
def test_bad_length(length):
    with pytest.raises(ValueError, match=rf"length.*{L0}\.\.2048.*L0 = {L0}"):
        _no_engine().agent_tokens(length=length)


@pytest.mark.parametrize("why,history,error", [
    ("dtype", lambda: torch.zeros((3, 5, 5), dtype=torch.int32), TypeError),
    ("float", lambda: torch.zeros((3, 5, 5)), TypeError),
    ("shape", lambda: torch.zeros((3, 5, 4), dtype=torch.int8), ValueError),
    ("rank", lambda: torch.zeros((3, 25), dtype=torch.int8), ValueError),
    ("device", lambda: torch.zeros((3, 5, 5), dtype=torch.int8, device="meta"), ValueError),
    ("numpy", lambda: np.zeros((3, 5, 5), dtype=np.int8), TypeError),
    ("list", lambda: [[[0] * 5] * 5] * 3, TypeError),
])
def test_bad_history(why, history, error):
    with pytest.raises(error, match="history"):
        _no_engine().agent_tokens(history=history())


@pytest.mark.parametrize("why,out", [
    ("dtype", lambda: torch.zeros((3, 5, L0), dtype=torch.int8)),
    ("shape", lambda: torch.zeros((3, 5, L0 + 1), dtype=torch.uint8)),
    ("stride", lambda: torch.zeros((3, 5, 2 * L0), dtype=torch.uint8)[..., ::2]),
    ("numpy", lambda: np.zeros((3, 5, L0), dtype=np.uint8)),
])
def test_bad_out(why, out):
    with pytest.raises(ValueError, match=r"out must be a contiguous uint8 tensor of shape \(3, 5, 179\)"):
        _no_engine().agent_tokens(out=out())
    with pytest.raises(ValueError, match=r"shape \(3, 5, 256\)"):
        _no_engine().agent_tokens(length=256, out=torch.zeros((3, 5, L0), dtype=torch.uint8))


# ---- TokenHistory --------------------------------------------------------------------------------------------------
class _Shape:
    batch, num_agents, device = 3, 2, CPU


def test_token_history_order_clearing_and_reset():
    from pogema_amd import TokenHistory
    h = TokenHistory(_Shape())
    t = h.tensor
    assert t.dtype == torch.int8 and tuple(t.shape) == (3, 2, 5) and bool((t == -1).all())
    for step in range(7):
        h.push(torch.full((3, 2), step % 5, dtype=torch.int64))
    assert h.tensor is t, "push() must keep the tensor a captured call reads"
    # most recent first: steps 6, 5, 4, 3, 2 -> actions 1, 0, 4, 3, 2
    assert t[1, 1].tolist() == [1, 0, 4, 3, 2]
    # per-agent values land in their rows; a value that is no action is recorded as -1
    h.push(torch.tensor([[0, 1], [2, 3], [4, 9]], dtype=torch.int32))
    assert t[:, :, 0].tolist() == [[0, 1], [2, 3], [4, -1]] and t[0, 0].tolist() == [0, 1, 0, 4, 3]
    # an env whose episode ended starts over, the others go on
    h.push(torch.ones((3, 2), dtype=torch.int8), episode_done=torch.tensor([0, 1, 0], dtype=torch.uint8))
    assert bool((t[1] == -1).all()) and t[0, 1].tolist() == [1, 1, 1, 0, 4] and t[2, 1].tolist() == [1, -1, 1, 0, 4]
    h.push(torch.zeros((3, 2), dtype=torch.int64), episode_done=torch.tensor([False, False, False]))
    assert t[1].tolist() == [[0, -1, -1, -1, -1]] * 2
    h.reset()
    assert h.tensor is t and bool((t == -1).all())
    with pytest.raises(ValueError, match="actions"):
        h.push(torch.zeros((3, 3), dtype=torch.int64))
    with pytest.raises(TypeError, match="actions"):
        h.push(torch.zeros((3, 2)))
    with pytest.raises(ValueError, match="episode_done"):
        h.push(torch.zeros((3, 2), dtype=torch.int64), episode_done=torch.zeros(2, dtype=torch.bool))


# ---- kernel resources --------------------------------------------------------------------------------------------
# (sgpr, vgpr) of agent_tokens_kernel<T, KT> (T: t = 2-byte fields, j = 4-byte) as the gfx950 cross-compile gave them
# when the kernel was written: the recorded budget.  KT registers hold the list; a count above these means the list left
# the registers or the row assembly grew.
RECORDED_BUDGET = {("t", 8): (88, 73), ("t", 16): (89, 81), ("t", 32): (89, 97),
                   ("j", 8): (88, 73), ("j", 16): (89, 81), ("j", 32): (89, 97)}


def _hipcc():
    import shutil
    return shutil.which("hipcc") or next((c for c in ("/opt/rocm/bin/hipcc",) if os.path.exists(c)), None)


def test_kernels_have_no_scratch_and_keep_four_waves_per_simd():
    hipcc = _hipcc()
    if hipcc is None:  # an environment reason, as in tests/test_kernel_resources.py
        pytest.skip("no hipcc on this box: the gfx950 resource remarks cannot be produced")
    src = os.path.join(ROOT, "pogema_amd", "csrc", "pgx_agent_tokens.hip")
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
        m = re.search(r"agent_tokens_kernelI([tj])Li(\d+)E", name)
        if m:
            key = (m.group(1), int(m.group(2)))
            seen.add(key)
            sgpr, vgpr = RECORDED_BUDGET[key]
            assert u["TotalSGPRs"] <= sgpr and u["VGPRs"] <= vgpr, (name, u, RECORDED_BUDGET[key])
    assert seen == set(RECORDED_BUDGET)
