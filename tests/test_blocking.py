"""CPU: the blocking reference (tests/blocking_reference.py, docs/SPEC.md S25) on the hand-built cases of
tests/blocking_cases.py; the exact shortcut of the section against the reference on random maps; the random inputs of
the GPU suite are not vacuous; the C-ABI of the feature: pgx_blocking is declared and exported, and its argument checks
need no device; the Python signatures and parsers, without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from blocking_cases import (CASES, MANY, RADIUS, SQUARE_GROUPS, WIDE, grid, instances, many_instance, square_instance,
                            wide_instance)
from blocking_reference import (CUT_OFF, DETOUR, FREE, NO_PATH, SAME_CELL, blocking_reference, filter_dismisses,
                                path_length, searched_pairs)
from expert_reference import bfs_from
from pogema_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference(case, inflation, blockers, is_active=None, kinds=None):
    count, blocked_by = blocking_reference(grid(case["map"])[None], [case["agents_xy"]], [case["targets_xy"]],
                                           [case["is_active"] if is_active is None else is_active], case["r"], inflation,
                                           blockers, kinds=kinds)
    return count[0], blocked_by[0]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_built_cases(case):
    assert len(case["map"]) <= 5 and all(len(row) <= 7 for row in case["map"]) and case["r"] in (1, 2)
    for (inflation, blockers), (want_count, want_by) in case["expect"].items():
        count, blocked_by = _reference(case, inflation, blockers)
        assert count.dtype == blocked_by.dtype == np.int32
        assert count.tolist() == want_count and blocked_by.tolist() == want_by, (inflation, blockers)
        assert sum(want_count) == sum(want_by)


def test_cases_cover_what_the_section_lists():
    by = {c["name"]: c for c in CASES}
    assert len(by) == len(CASES) == 11

    def kinds_of(case, inflation, **kw):
        kinds = {}
        _reference(case, inflation, "all", kinds=kinds, **kw)
        return {(i, j): v for (_, i, j), v in kinds.items()}

    assert all(kinds_of(by["corridor, cut off"], k)[(0, 1)] == CUT_OFF for k in (1, 10, 64))
    assert set(kinds_of(by["open 3 x 3, nobody blocked"], 1).values()) == {FREE}
    # the detours are exactly 2 and 4 steps: blocked at the inflation that equals them, free one above
    for name, detour in (("detour of 2", 2), ("detour of 4, one more wall", 4)):
        c = by[name]
        blocked = grid(c["map"]) != 0
        d0 = path_length(blocked, c["agents_xy"][1], c["targets_xy"][1])
        blocked[tuple(c["agents_xy"][0])] = True
        assert path_length(blocked, c["agents_xy"][1], c["targets_xy"][1]) - d0 == detour
        assert kinds_of(c, detour)[(0, 1)] == DETOUR and kinds_of(c, detour + 1)[(0, 1)] == FREE
        assert kinds_of(c, 1)[(0, 1)] == DETOUR
    walls = grid(by["detour of 4, one more wall"]["map"]) - grid(by["detour of 2"]["map"])
    assert walls.sum() == 1 and walls.min() == 0, "the same map with one more wall"
    c = by["on the other's target"]
    assert c["agents_xy"][0] == c["targets_xy"][1] and kinds_of(c, 64)[(0, 1)] == CUT_OFF
    assert kinds_of(by["unreachable target"], 1)[(0, 1)] == NO_PATH
    c = by["outside the window"]
    assert (0, 1) not in kinds_of(c, 1) and (1, 0) not in kinds_of(c, 1) and abs(c["agents_xy"][0][1] - c["agents_xy"][1][1]) == 2
    assert kinds_of({**c, "r": 2}, 1)[(0, 1)] == CUT_OFF, "one column more of radius and it counts"
    c = by["inactive agent"]
    assert c["is_active"] == [False, True] and not kinds_of(c, 1)
    assert kinds_of(c, 1, is_active=[True, True])[(0, 1)] == CUT_OFF, "were it active, it would block"
    assert max(by["one blocks two"]["expect"][(10, "all")][0]) == 2
    assert max(by["one blocked by two"]["expect"][(10, "all")][1]) == 2
    c = by["on_target leaves a blocker out"]
    assert c["expect"][(10, "all")] != c["expect"][(10, "on_target")]


def _random_state(rng, B, A, H, W, density):
    obst = (rng.random((B, H, W)) < density).astype(np.uint8)
    agents = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)    # agents may share a cell
    targets = np.stack([rng.integers(0, H, (B, A)), rng.integers(0, W, (B, A))], -1)   # obstacle targets included
    obst[np.arange(B)[:, None], agents[..., 0], agents[..., 1]] = 0                    # agents stand on free cells
    return obst, agents, targets, rng.random((B, A)) < 0.85


def test_sums_agree_and_modes_nest_on_random_instances():
    rng = np.random.default_rng(25)
    blocked_pairs = 0
    for r, inflation in ((1, 1), (2, 3), (3, 10), (2, 64)):
        obst, agents, targets, active = _random_state(rng, 3, 9, 9, 10, 0.3)
        count, blocked_by = blocking_reference(obst, agents, targets, active, r, inflation)
        assert (count.sum(1) == blocked_by.sum(1)).all()
        assert not count[~active].any() and not blocked_by[~active].any()
        blocked_pairs += int(count.sum())
        c2, b2 = blocking_reference(obst, agents, targets, active, r, inflation, "on_target")
        assert (c2 <= count).all() and (b2 <= blocked_by).all() and (c2.sum(1) == b2.sum(1)).all()
        on = (agents == targets).all(-1)
        assert not c2[~on].any()
        # a larger inflation never blocks more
        c3, _ = blocking_reference(obst, agents, targets, active, r, min(inflation + 2, 64))
        assert (c3 <= count).all()
        only = blocking_reference(obst, agents, targets, active, r, inflation, envs=[1])
        assert all(np.array_equal(o[1], g[1]) and not o[[0, 2]].any() for o, g in zip(only, (count, blocked_by)))
    assert blocked_pairs


def test_the_filter_only_dismisses_unblocked_pairs():
    """S25's shortcut against the naive reference on seeded random maps: a pair with F_j[c] undefined or
    F_j[c] + |c - s|_1 > F_j[s] is never blocked, at any inflation (1 is the strictest); the filter does dismiss pairs and
    does leave pairs, blocked and unblocked ones, to the search."""
    rng = np.random.default_rng(250)
    dismissed = left_blocked = left_free = 0
    for density in (0.15, 0.3, 0.4):
        obst, agents, targets, active = _random_state(rng, 4, 8, 8, 9, density)
        kinds = {}
        blocking_reference(obst, agents, targets, active, 3, 1, kinds=kinds)
        out, left = searched_pairs(obst, agents, targets, kinds)
        for b, i, j in out:
            assert kinds[(b, i, j)] == FREE, (b, i, j)
            assert filter_dismisses(obst[b], agents[b, i], agents[b, j], targets[b, j])   # (the same without the shared field)
        assert len(out) + len(left) == sum(k not in (NO_PATH, SAME_CELL) for k in kinds.values())
        dismissed += len(out)
        left_blocked += sum(kinds[p] in (DETOUR, CUT_OFF) for p in left)
        left_free += sum(kinds[p] == FREE for p in left)
        # the field the filter reads is the one the reference's first search walks
        b, i, j = next(iter(kinds))
        F = bfs_from(obst[b] != 0, *targets[b, j])
        assert F[tuple(agents[b, j])] == path_length(obst[b] != 0, agents[b, j], targets[b, j])
    assert dismissed and left_blocked and left_free


def _tally(obst, agents, targets, r, inflation):
    kinds = {}
    blocking_reference(obst, agents, targets, np.ones(agents.shape[:2], bool), r, inflation, kinds=kinds)
    _, left = searched_pairs(obst, agents, targets, kinds)
    return np.array([sum(v == CUT_OFF for v in kinds.values()), sum(v == DETOUR for v in kinds.values()),
                     sum(kinds[p] == FREE for p in left)])


@pytest.mark.parametrize("size", sorted(SQUARE_GROUPS))
def test_gpu_square_groups_are_not_vacuous(size):
    """Over the reset states of each map side's group the reference alone finds a pair blocked by cut-off, one blocked
    by a detour and one that passes the filter and is still not blocked.  Side 2 is exempt by arithmetic: one agent has
    no pair and four cells hold no detour."""
    total = np.zeros(3, dtype=np.int64)
    for k in range(3):
        obst, agents, targets, inflation = square_instance(size, k)
        assert obst.shape == (3, size, size) and agents.shape[1] == (1 if size == 2 else (1, 6, 13)[k]) and 2 <= inflation <= 4
        assert not obst[np.arange(3)[:, None], agents[..., 0], agents[..., 1]].any()
        assert not obst[np.arange(3)[:, None], targets[..., 0], targets[..., 1]].any()
        total += _tally(obst, agents, targets, RADIUS, inflation)
    assert (total > 0).all() if size > 2 else not total.any(), total


def test_gpu_wide_map_is_not_vacuous():
    obst, agents, targets = wide_instance()
    assert obst.shape[1] * obst.shape[2] > 65536
    assert (_tally(obst, agents, targets, WIDE["r"], WIDE["inflation"]) > 0).all()


def test_instances_are_a_function_of_their_arguments():
    a = instances(2, 9, 11, 5, 0.3, 7, cluster=2, reach=3)
    b = instances(2, 9, 11, 5, 0.3, 7, cluster=2, reach=3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    obst, starts, targets = a
    assert np.abs(targets - starts).max() <= 3
    assert len({tuple(c) for c in starts[0].tolist()}) == 5
    for row in MANY:
        assert row[0] > 256


def test_header_declares_and_library_exports(engine_lib):
    src = open(os.path.join(ROOT, "include", "pogema_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+pgx_blocking\s*\(\s*pgx_env\s*\*\s*env\s*,\s*int32_t\s+inflation\s*,\s*int32_t\s+flags\s*,"
                     r"\s*int32_t\s*\*\s*count\s*,\s*int32_t\s*\*\s*blocked_by\s*,\s*void\s*\*\s*stream\s*\)", text)
    on_target = int(re.search(r"#define\s+PGX_BLOCKING_ON_TARGET\s+(\d+)\b", text).group(1))
    most = int(re.search(r"#define\s+PGX_MAX_BLOCKING_INFLATION\s+(\d+)\b", text).group(1))
    assert _lib.BLOCKING_ON_TARGET == on_target == 1 and _lib.MAX_BLOCKING_INFLATION == most == 64
    assert _lib.BLOCKING_BLOCKERS == {"all": 0, "on_target": on_target}
    assert re.search(r"#define\s+PGX_ABI_VERSION\s+6\b", text), "the entry point is additive"
    assert "pgx_blocking" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_blocking")


def test_signatures_and_defaults():
    from pogema_amd import VecPogema
    from pogema_amd.envs import Pogema
    sig = inspect.signature(VecPogema.blocking)
    assert list(sig.parameters) == ["self", "inflation", "blockers", "out"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [10, "all", None]
    sig = inspect.signature(Pogema.blocking)
    assert list(sig.parameters) == ["self", "inflation", "blockers"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [10, "all"]


def test_invalid_arguments_need_no_device(engine_lib):
    """PGX_E_INVALID when both outputs are NULL, for an inflation outside 1..64, an unknown flag bit and a misaligned
    output: checked before the handle, so a NULL handle is never reached (a well-formed call on a NULL handle is refused
    too)."""
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf)
    base += -base % 16
    call = engine_lib.pgx_blocking   # (env, inflation, flags, count, blocked_by, stream)

    def refused(needle, *args):
        assert call(*args) == -1
        assert needle in engine_lib.pgx_last_error().decode()

    refused("both null", None, 10, 0, None, None, None)
    for inflation in (0, -1, 65, 1000):
        refused("outside 1..64", None, inflation, 0, base, base, None)
    for flags in (2, 3, 4, -1):
        refused("flags", None, 10, flags, base, base, None)
    for off in (1, 2, 3):
        refused("count is not 4-byte aligned", None, 10, 0, base + off, base, None)
        refused("blocked_by is not 4-byte aligned", None, 10, 1, base, base + off, None)
    # either output may be NULL, 1 and 64 are inflations, the flag is known: the refusal that remains is the NULL handle's
    refused("null handle", None, 1, 0, base, None, None)
    refused("null handle", None, 64, 1, None, base + 4, None)
    refused("null handle", None, 10, 1, base, base, None)


def test_parsers_need_no_gpu():
    from pogema_amd.queries import parse_blockers, parse_blocking_inflation
    for ok in (1, 10, 64, np.int64(2), np.int16(64)):
        got = parse_blocking_inflation(ok)
        assert got == int(ok) and type(got) is int
    assert parse_blocking_inflation() == 10
    for bad in (0, -1, 65, 960):
        with pytest.raises(ValueError, match=r"1\.\.64"):
            parse_blocking_inflation(bad)
    for bad in (2.0, True, False, "3", None, (3,)):
        with pytest.raises(TypeError, match=r"1\.\.64"):
            parse_blocking_inflation(bad)
    assert parse_blockers() == 0 and parse_blockers("all") == 0 and parse_blockers("on_target") == _lib.BLOCKING_ON_TARGET
    for bad in ("none", "", None, 0, True, ("all",)):
        with pytest.raises(ValueError, match=r"\['all', 'on_target'\]"):
            parse_blockers(bad)
