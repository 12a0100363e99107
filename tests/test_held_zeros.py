"""CPU: held zeros (pgx_step_held) -- the new kernel instances' register budget, a NumPy model of the skip predicate
against brute force, and the trust bookkeeping of RecyclingOutputs on CPU tensors."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_held_instances_keep_eight_waves_per_simd_and_do_not_spill():
    """no scratch, at most 64 VGPRs, eight waves per SIMD -- for every step_held<G, MW> instance; the
    one configs[2] runs (G = 64, MW) must be among them."""
    hipcc = next((c for c in ("/opt/rocm/bin/hipcc",) if os.path.exists(c)), None)
    if hipcc is None:
        import shutil
        hipcc = shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("no hipcc on this box: the gfx950 resource remarks cannot be produced")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "step_held"], capture_output=True,
                       text=True, cwd=ROOT, timeout=900)
    rows = re.findall(r"step_heldILi(\d+)ELb(\d)\S*\s+sgpr\s+(\d+) vgpr\s+(\d+) scratch\s+(\d+) occ (\d+)", p.stdout)
    assert rows, p.stdout[-2000:] + p.stderr[-2000:]
    assert ("64", "1") in {(g, mw) for g, mw, *_ in rows}
    for g, mw, sgpr, vgpr, scratch, occ in rows:
        assert int(scratch) == 0 and int(vgpr) <= 64 and int(occ) == 8, (g, mw, sgpr, vgpr, scratch, occ)


# ---- the skip predicate ----------------------------------------------------------------------------------------------
def kernel_model(base_bytes, envs_per_slice, agents, W, was, now, unit=128):
    """What step_held decides for one workgroup's slice, restated: -> bool per float of the slice, True = written.
    `base_bytes`: address of the slice's first float (a multiple of 4); was / now: flat target index per agent of the slice
    (was: 255 = unknown).  The <= 3 floats in front of / behind the 16-byte aligned part are always written; a float4 is left
    out iff the bit of its aligned `unit` is set; the bit is set iff the unit lies wholly inside one agent's target plane, the
    agent's old index is known, and the unit holds neither the old nor the new index."""
    nag = envs_per_slice * agents
    n = nag * 3 * W * W
    head = min(n, (4 - (base_bytes // 4) % 4) % 4)
    nvec = (n - head) // 4
    ub = base_bytes // unit
    skip = set()
    for la in range(nag):
        if was[la] >= W * W:
            continue
        plane = base_bytes + (la * 3 + 2) * W * W * 4
        uw, un = (plane + was[la] * 4) // unit - ub, (plane + now[la] * 4) // unit - ub
        for u in range((plane + unit - 1) // unit - ub, (plane + W * W * 4) // unit - ub):
            if u != uw and u != un:
                skip.add(u)
    written = np.ones(n, bool)
    a0 = (base_bytes + head * 4) // 16 - ub * (unit // 16)
    for q in range(nvec):
        if (q + a0) // (unit // 16) in skip:
            written[head + 4 * q: head + 4 * q + 4] = False
    return written


def brute_force_may_skip(base_bytes, nag, W, was, now):
    """The issue's correctness predicate per 16-byte store, from first principles: a store at an absolute 16-byte aligned
    address may be left out iff all its floats belong to ONE agent's target plane, that agent's old index is known, and
    none of them is the old or the new index."""
    n = nag * 3 * W * W
    may = np.zeros(n, bool)
    for e in range(n):
        addr = base_bytes + 4 * e
        lo = (addr // 16 * 16 - base_bytes) // 4
        cells = range(lo, lo + 4)
        if lo < 0 or lo + 4 > n:
            continue
        owners = {c // (W * W) for c in cells}
        if len(owners) != 1:
            continue
        item = owners.pop()
        la, ch = divmod(item, 3)
        if ch != 2 or was[la] >= W * W:
            continue
        idx = {c - item * W * W for c in cells}
        may[e] = was[la] not in idx and now[la] not in idx
    return may


@pytest.mark.parametrize("W", [7, 11, 15])
@pytest.mark.parametrize("unit", [16, 64, 128])
@pytest.mark.parametrize("agents,envs,env0", [(64, 1, 3), (3, 5, 7), (8, 2, 1), (100, 1, 2)])
def test_skip_predicate_against_brute_force(W, unit, agents, envs, env0):
    rng = np.random.default_rng(W * 1000 + unit + agents)
    nag = envs * agents
    base = 4096 + env0 * nag * 3 * W * W * 4  # A = 3, W = 7: slices start at bytes that are no multiple of 16
    n = nag * 3 * W * W
    for case in ("same", "moved", "unknown", "mixed"):
        was = rng.integers(0, W * W, nag)
        now = was.copy() if case == "same" else rng.integers(0, W * W, nag)
        if case == "unknown":
            was[:] = 255
        if case == "mixed":
            was[rng.random(nag) < 0.3] = 255
        written = kernel_model(base, envs, agents, W, was, now, unit)
        may = brute_force_may_skip(base, nag, W, was, now)
        assert not (~written & ~may).any(), f"{case}: a store was left out that the predicate does not allow"
        if case == "unknown":
            assert written.all()
        # writing the unskipped floats of the new tensor over the old one gives the new one bit for bit
        old, new = np.zeros(n, np.float32), np.zeros(n, np.float32)
        planes = (np.arange(nag) * 3 + 2) * W * W
        known = was < W * W
        old[planes[known] + was[known]] = 1.0
        unknown = np.flatnonzero(~known)
        for la in unknown:  # an unknown plane holds anything
            old[planes[la]: planes[la] + W * W] = np.nan
        other = np.ones(n, bool)
        for la in range(nag):
            other[planes[la]: planes[la] + W * W] = False
        old[other] = rng.integers(0, 2, int(other.sum()))
        new[planes + now] = 1.0
        new[other] = rng.integers(0, 2, int(other.sum()))
        old[written] = new[written]
        assert np.array_equal(old.view(np.uint32), new.view(np.uint32)), case
        if unit == 128 and W == 11 and agents == 64 and case in ("same", "moved"):
            # the headline shape: a 484-byte plane holds 2.8 whole 128-byte lines on average, of 1452 bytes per agent; the 1.0
            # costs one of them with probability 0.74 (same cell), two independent ones 1.3 on average
            left_out = 1.0 - written.mean()
            assert (0.16 < left_out < 0.20) if case == "same" else (0.10 < left_out < 0.16), (case, left_out)


# ---- who vouches for a set -------------------------------------------------------------------------------------------
def test_trust_bookkeeping_of_the_recycler():
    import torch
    from pogema_amd.buffers import RecyclingOutputs
    assert RecyclingOutputs.available()
    B, A = 4, 3
    rec = RecyclingOutputs([torch.zeros((B, A, 3, 7, 7)) for _ in range(2)], B, A)
    seen = {}
    for _ in range(2):  # first use of either set: nothing is known about it
        outs, held, trusted, i = rec.take_for_step()
        assert not trusted and held.dtype == torch.uint8 and tuple(held.shape) == (B, A) and int(held.min()) == 255
        rec.vouch(i)  # the engine has written it with pgx_step_held
        seen[i] = held
        del outs
    assert len(seen) == 2 and seen[0].data_ptr() != seen[1].data_ptr()
    outs, held, trusted, i = rec.take_for_step()
    assert trusted and held is seen[i], "a held write makes the set trusted"
    rec.vouch(i)
    outs[0][1:3].view(-1)[5:9].mul_(2)  # an in-place operation through a view of the handed-out tensor
    del outs
    j = rec.take_for_step()
    assert j[2] and j[3] != i  # (the other set is still fine)
    rec.vouch(j[3])
    del j
    outs, _, trusted, i2 = rec.take_for_step()
    assert i2 == i and not trusted, "an in-place op through a view makes the set untrusted"
    rec.vouch(i2)
    del outs
    outs, _, trusted, k = rec.take_for_step(with_obs=False)  # no observation written: the record stays
    assert outs[0] is None and not trusted
    del outs
    plain = rec.take()  # somebody else may write it now
    idx = [n for n, (m, _, _) in enumerate(rec._sets) if m[0].data_ptr() == plain[0].data_ptr()][0]
    del plain
    for _ in range(2):
        outs, _, trusted, n = rec.take_for_step()
        assert trusted == (n != idx), "plain take() makes the set untrusted"
        rec.vouch(n)
        del outs
    a, b = rec.take_for_step(), rec.take_for_step()
    assert rec.take_for_step() is None and rec.misses == 1
    del a, b
    outs, _, trusted, n = rec.take_for_step()  # taken for a step that then never vouched (a failed launch): untrusted
    assert not trusted
