"""CPU: the reference of plan repair (tests/repair_plan_reference.py, docs/SPEC.md S29) does what the specification
says -- on the hand-built cases of tests/repair_plan_cases.py, whose outputs were worked out on paper, and on random
instances, where the properties S29 lists hold: everybody replanned is whca_plan, a plan repaired for the tail of its own
service order is that plan again, nobody asked for leaves a valid plan alone, kept agents keep their cells, and the result
is free of conflicts where the kept agents were and nobody failed.  The package's argument checks that need no engine are
checked here too."""
import numpy as np
import pytest

from repair_plan_cases import CASES, NAMES, active, expected, given, grid
from repair_plan_reference import repair_env, repair_reference, walk_scan
from test_whca import RANDOM
from util import generate_instances
from whca_reference import conflicts, whca_reference


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_cases(case):
    got = repair_env(grid(case["map"]), case["agents"], case["targets"], active(case), given(case), case["replan"],
                     case["priority"], case["on_target"])
    for name, g, w in zip(NAMES, got, expected(case)):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{case['name']}: {name}\n{g}\nexpected\n{w}"


def test_walk_scan():
    blocked = grid(["...", ".#.", "..."]) != 0
    assert walk_scan(blocked, (0, 0), (0, 2), [(0, 1), (0, 2), (9, 9)], "finish") == (True, 2)
    assert walk_scan(blocked, (0, 0), (0, 2), [(0, 1), (0, 2), (9, 9)], "nothing") == (False, 3)
    assert walk_scan(blocked, (0, 0), (0, 2), [(0, 0), (0, 0), (0, 0)], "finish") == (True, 3)        # stays are moves
    assert walk_scan(blocked, (0, 2), (0, 2), [(0, 2), (1, 1)], "finish") == (True, 1)                 # h >= 1, not h = 0
    assert walk_scan(blocked, (0, 0), (0, 2), [(1, 0), (1, 1)], "finish") == (False, 2)
    # the target itself is checked like any cell before the scan stops on it
    assert walk_scan(blocked, (0, 0), (0, 2), [(0, 2)], "finish") == (False, 1)


@pytest.fixture(scope="module")
def plans():
    """Per shape of test_whca.RANDOM and on_target mode: the instance, priorities and whca's own plan for them."""
    out = {}
    for name, size, A, density, B, seed, K in RANDOM:
        obstacles, agents, targets = generate_instances(B, size, size, A, density, seed)
        rng = np.random.default_rng(seed)
        prio = rng.integers(-3, 4, size=(B, A))
        act = rng.random((B, A)) < 0.9
        for on_target in ("finish", "nothing"):
            out[name, on_target] = (obstacles, agents, targets, act, K, prio,
                                    whca_reference(obstacles, agents, targets, act, K, prio, on_target))
    return out


KEYS = [(row[0], on_target) for row in RANDOM for on_target in ("finish", "nothing")]


@pytest.mark.parametrize("name,on_target", KEYS)
def test_everybody_replanned_is_whca_plan(plans, name, on_target):
    """Property 1, from given paths that are garbage."""
    obstacles, agents, targets, act, K, prio, want = plans[name, on_target]
    B, A = act.shape
    rng = np.random.default_rng(5)
    junk = rng.integers(-2 ** 31, 2 ** 31, size=(K, B, A, 2)).astype(np.int32)
    got = repair_reference(obstacles, agents, targets, act, junk, np.ones((B, A), dtype=bool), prio, on_target)
    for k in (0, 1, 2, 3):
        assert np.array_equal(got[k], want[k]), NAMES[k]
    assert np.array_equal(got[5], want[4]) and np.array_equal(got[4], act.astype(np.int32))
    # the same without a mask: no walk anywhere, so everybody is replanned all the same
    got = repair_reference(obstacles, agents, targets, act, np.full((K, B, A, 2), -1, dtype=np.int32), None, prio, on_target)
    for k in (0, 1, 2, 3):
        assert np.array_equal(got[k], want[k]), NAMES[k]


def tail_mask(act, prio, m):
    """The last min(m, planned) agents of every env's service order."""
    mask = np.zeros(act.shape, dtype=bool)
    for b in range(act.shape[0]):
        order = sorted((i for i in range(act.shape[1]) if act[b, i]), key=lambda i: (-int(prio[b, i]), i))
        mask[b, order[max(0, len(order) - m):]] = m > 0
    return mask


@pytest.mark.parametrize("name,on_target", KEYS)
def test_repairing_the_tail_of_the_service_order_is_the_plan_again(plans, name, on_target):
    """Properties 2 and 3: actions, cells and arrivals bit for bit, `failed` for the agents served again (a kept agent
    never counts as failed: it is held to its given cells, which for an agent that failed are its own cell)."""
    obstacles, agents, targets, act, K, prio, (actions, path, arrival, failed, last) = plans[name, on_target]
    B, A = act.shape
    for m in (0, 1, A // 2, A, None):
        mask = None if m is None else tail_mask(act, prio, m)
        got = repair_reference(obstacles, agents, targets, act, path, mask, prio, on_target)
        asked = np.zeros((B, A), dtype=bool) if mask is None else mask
        assert np.array_equal(got[0], actions) and np.array_equal(got[1], path) and np.array_equal(got[2], arrival), m
        assert np.array_equal(got[3], failed * asked) and np.array_equal(got[4], asked.astype(np.int32)), m
        assert np.array_equal(got[5], last), m


def corrupt(paths, rng, share=0.1):
    """About `share` of the agents get random cells, jumps or int32 extremes somewhere in their path."""
    paths = paths.copy()
    K, B, A = paths.shape[:3]
    hit = rng.random((B, A)) < share
    for b, i in np.argwhere(hit):
        h = rng.integers(K)
        kind = rng.integers(3)
        if kind == 0:
            paths[h:, b, i] = rng.integers(-3, 20, size=(K - h, 2))
        elif kind == 1:
            paths[h, b, i] += rng.integers(2, 5, size=2)
        else:
            paths[h, b, i] = rng.choice([-2 ** 31, 2 ** 31 - 1], size=2)
    return paths, hit


@pytest.mark.parametrize("name,on_target", KEYS)
def test_kept_agents_keep_their_cells_and_the_result_is_conflict_free(plans, name, on_target):
    """Properties 4 and 5, from whca's plan with a tenth of the agents corrupted, a random half asked for and other
    priorities."""
    obstacles, agents, targets, act, K, _, (_, path, _, given_failed, _) = plans[name, on_target]
    B, A = act.shape
    rng = np.random.default_rng(17)
    paths, hit = corrupt(path, rng)
    mask = rng.random((B, A)) < 0.5
    prio = rng.integers(-3, 4, size=(B, A))
    actions, out, arrival, failed, replanned, last = repair_reference(obstacles, agents, targets, act, paths, mask, prio,
                                                                      on_target)
    assert np.array_equal(replanned.astype(bool) & ~mask, replanned.astype(bool) & ~mask & hit), "a valid path was replanned"
    assert (replanned[mask & act] == 1).all() and (replanned[~act] == 0).all() and (failed[replanned == 0] == 0).all()
    checked = 0
    for b in range(B):
        kept = [i for i in range(A) if act[b, i] and not replanned[b, i]]
        for i in kept:
            n = last[b, i]
            assert np.array_equal(out[:n, b, i], paths[:n, b, i]) and (out[n:, b, i] == paths[n - 1, b, i]).all()
            assert (actions[n:, b, i] == 0).all()
        for i in range(A):
            if not act[b, i]:
                assert (out[:, b, i] == agents[b, i]).all() and (actions[:, b, i] == 0).all() and last[b, i] == -1
        kept_last = np.where(replanned[b] == 0, last[b], -1)
        if conflicts(agents[b], out[:, b], kept_last, np.zeros(A, dtype=np.int32)) or failed[b].any():
            continue
        checked += 1
        assert conflicts(agents[b], out[:, b], last[b], failed[b]) == [], f"{name}/{on_target} env {b}"
    assert checked >= 1, "the guarantee was checked in no env"


def test_arguments_are_checked_without_an_engine():
    """VecPogema.repair_plan refuses bad `paths`, `replan` and `out` before it touches the engine, and hands the
    engine the caller's pointers -- `paths` itself as out[path_xy] included."""
    import torch
    from pogema_amd import _lib
    from pogema_amd.queries import QueryMixin
    assert "pgx_repair_plan" in _lib.EXPORTED_SYMBOLS
    calls = []

    class Recorder:
        @staticmethod
        def pgx_repair_plan(*args):
            calls.append(args)
            return 0

    class NoEngine(QueryMixin):
        batch, num_agents, device = 2, 3, torch.device("cpu")
        _ACTION_CODE = {torch.int8: 0, torch.int32: 1, torch.int64: 2}
        _handle, _lib = None, Recorder
        _stream = staticmethod(lambda: None)

    env, K = NoEngine(), 4
    paths = torch.zeros((K, 2, 3, 2), dtype=torch.int32)
    for bad in (paths.to(torch.int64), paths.to(torch.float32), paths.numpy(), paths.tolist(), None):
        with pytest.raises(TypeError, match="paths must be an int32"):
            env.repair_plan(bad)
    for bad in (paths[0], paths[:, :1], paths[..., :1], torch.zeros((0, 2, 3, 2), dtype=torch.int32),
                torch.zeros((32, 2, 3, 2), dtype=torch.int32), torch.zeros((K, 2, 3, 4), dtype=torch.int32)[..., ::2],
                torch.zeros((K, 3, 2, 2), dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"paths must be .*shape \(K, 2, 3, 2\).*got shape") as ei:
            env.repair_plan(bad)
        assert str(tuple(bad.shape)) in str(ei.value)
    for bad in (torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.float32), [[0] * 3] * 2):
        with pytest.raises(TypeError, match="replan must be a bool or uint8"):
            env.repair_plan(paths, replan=bad)
    for bad in (torch.zeros((2, 4), dtype=torch.bool), torch.zeros((3, 2), dtype=torch.uint8),
                torch.zeros((2, 6), dtype=torch.uint8)[:, ::2], torch.zeros((3, 2), dtype=torch.bool).t()):
        with pytest.raises(ValueError, match="replan must be a contiguous"):
            env.repair_plan(paths, replan=bad)
    with pytest.raises(TypeError, match="priority"):
        env.repair_plan(paths, priority=torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="dtype must be"):
        env.repair_plan(paths, dtype=torch.float32)

    make = lambda: [torch.zeros((K, 2, 3), dtype=torch.int32), torch.zeros((K, 2, 3, 2), dtype=torch.int32),
                    torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int32),
                    torch.zeros((2, 3), dtype=torch.int32)]
    with pytest.raises(ValueError, match="out must be"):
        env.repair_plan(paths, out=tuple(make()[:4]))
    for k, t in ((0, torch.zeros((K, 2, 3))), (1, torch.zeros((K, 2, 3), dtype=torch.int32)),
                 (2, torch.zeros((2, 3), dtype=torch.int64)), (3, None), (4, torch.zeros((3, 2), dtype=torch.int32))):
        o = make()
        o[k] = t
        with pytest.raises(ValueError, match="out"):
            env.repair_plan(paths, out=tuple(o))
    # overlaps: a longer buffer that holds `paths` and an output side by side, one cell apart
    flat = torch.zeros(2 * paths.numel(), dtype=torch.int32)
    inside = flat[:paths.numel()].view(K, 2, 3, 2)
    o = make()
    o[1] = flat[2:2 + paths.numel()].view(K, 2, 3, 2)
    with pytest.raises(ValueError, match=r"out\[path_xy\] overlaps paths"):
        env.repair_plan(inside, out=tuple(o))
    o = make()
    o[0] = flat[:K * 6].view(K, 2, 3)
    with pytest.raises(ValueError, match=r"out\[actions\] overlaps paths"):
        env.repair_plan(inside, out=tuple(o))
    o = make()
    o[4] = flat[paths.numel() - 6:paths.numel()].view(2, 3)
    with pytest.raises(ValueError, match=r"out\[replanned\] overlaps paths"):
        env.repair_plan(inside, out=tuple(o))
    assert calls == []
    o = make()
    o[4] = flat[paths.numel():paths.numel() + 6].view(2, 3)        # right behind `paths`: no overlap
    o[1] = inside                                                   # in place
    mask = torch.ones((2, 3), dtype=torch.bool)
    got = env.repair_plan(inside, replan=mask, out=tuple(o))
    assert all(g is t for g, t in zip(got, o)) and len(calls) == 1
    handle, flags, horizon, p_paths, p_replan, p_prio, p_actions, code, p_path, p_arr, p_failed, p_repl, stream = calls[0]
    assert (flags, horizon, code, p_prio) == (0, K, 1, None)
    assert p_paths == p_path == inside.data_ptr() and p_replan == mask.data_ptr() and p_repl == o[4].data_ptr()
    assert (p_actions, p_arr, p_failed) == (o[0].data_ptr(), o[2].data_ptr(), o[3].data_ptr())
    fresh = env.repair_plan(paths, dtype=torch.int8)
    assert fresh[0].dtype == torch.int8 and tuple(fresh[0].shape) == (K, 2, 3) and tuple(fresh[1].shape) == (K, 2, 3, 2)
    assert all(t.dtype == torch.int32 and tuple(t.shape) == (2, 3) for t in fresh[2:]) and calls[1][4] is None
