"""GPU: blocking counts (VecPogema.blocking / pgx_blocking, docs/SPEC.md S25) equal the naive CPU reference
(tests/blocking_reference.py) bit for bit on get_state() and the installed maps -- the hand-built cases, both search
layouts, one and two row words, 2- and 4-byte fields, every collision system and on_target mode, agent counts up to
1024, inflation 1, 10 and 64, both `blockers` modes; `out=` tensors and offset views change nothing; the shared field
cache follows S11's contract; the engine state is left alone; a graph replay equals the eager run.  The random inputs are
tests/blocking_cases.py's, which tests/test_blocking.py proves not to be vacuous."""
import numpy as np
import pytest

from agent_counts import LAYOUT_ROWS, radii_accepted
from blocking_cases import (CASES, MANY, MODES, RADIUS, SQUARE_BATCH, SQUARE_GROUPS, WIDE, instances, many_instance,
                            square_instance, wide_instance)
from blocking_reference import blocking_reference
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu


def _reference(env, inflation, blockers, envs=None):
    st = env.get_state()
    return blocking_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                              st["is_active"].cpu().numpy(), env.obs_radius, inflation, blockers, envs=envs)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} mismatches, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _check(env, what="", settings=((10, "all"),), envs=None):
    """blocking() == the reference, bit for bit, for every (inflation, blockers) of `settings`; `envs`: only those rows.
    Returns the last reference."""
    torch = lazy_torch()
    rows = slice(None) if envs is None else list(envs)
    for inflation, blockers in settings:
        want = _reference(env, inflation, blockers, envs=envs)
        got = env.blocking(inflation=inflation, blockers=blockers)
        tag = f"{what} [inflation {inflation}, {blockers}]"
        for g, w, name in zip(got, want, ("count", "blocked_by")):
            assert g.dtype == torch.int32 and tuple(g.shape) == (env.batch, env.num_agents)
            _same(g[rows], w[rows], f"{tag} {name}")
        assert torch.equal(got[0].sum(1), got[1].sum(1)), f"{tag}: the sums differ"
    return want


def _install(obstacles, agents, targets, r, collision="soft", on_target="nothing", **kw):
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(map=obstacles[0].tolist(), num_agents=agents.shape[1], obs_radius=r, collision_system=collision,
                    on_target=on_target, max_episode_steps=256, seed=1)
    env = VecPogema(gc, batch=len(obstacles), **kw)
    env.reset_from_state(obstacles, agents, targets)
    return env


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_shared_cases(case):
    """The hand-built cases, installed through GridConfig(map, agents_xy, targets_xy) at batch 2, against the arrays the
    case writes out and against the reference."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(map="\n".join(case["map"]), agents_xy=case.get("start_xy", case["agents_xy"]),
                    targets_xy=case["targets_xy"], obs_radius=case["r"],
                    on_target="finish" if "actions" in case else "nothing", max_episode_steps=64)
    env = VecPogema(gc, batch=2)
    env.reset(seed=0)
    if "actions" in case:
        env.step(torch.as_tensor([case["actions"]] * 2, device=env.device))
    assert env.get_state()["is_active"][0].cpu().numpy().astype(bool).tolist() == case["is_active"]
    _check(env, what=case["name"], settings=tuple(case["expect"]))
    for (inflation, blockers), (want_count, want_by) in case["expect"].items():
        count, blocked_by = env.blocking(inflation=inflation, blockers=blockers)
        for b in range(2):
            assert count[b].tolist() == want_count and blocked_by[b].tolist() == want_by, (case["name"], inflation, blockers)
    env.close()


# sides up to 32 take one 32-bit word of the padded bitmap per row, 33 and 64 two; 64 and 65 switch between the two
# search layouts
@pytest.mark.parametrize("size", sorted(SQUARE_GROUPS))
def test_square_maps_match_reference(size):
    found = 0
    for k in range(3):
        obstacles, agents, targets, inflation = square_instance(size, k)
        collision, on_target = MODES[(k + size) % 3]
        env = _install(obstacles, agents, targets, RADIUS, collision, on_target)
        assert env.batch == SQUARE_BATCH
        what = f"size {size} A={agents.shape[1]} {collision}/{on_target}"
        found += int(_check(env, what=f"{what} reset", settings=((inflation, "on_target"), (inflation, "all")))[0].sum())
        rng = np.random.default_rng(size + k)
        for _ in range(4):
            env.step(mixed_actions(env, rng, p_expert=0.7))
        _check(env, what=f"{what} after 4 steps", settings=((inflation, "all"),))
        env.close()
    assert found or size == 2


def test_wide_cell_map():
    """257 x 256 has more than 65536 cells: 4-byte fields."""
    obstacles, agents, targets = wide_instance()
    env = _install(obstacles, agents, targets, WIDE["r"], "block_both", "restart")
    want = _check(env, what="257 x 256 reset", settings=((WIDE["inflation"], "all"),))
    assert want[0].any()
    rng = np.random.default_rng(257)
    for _ in range(4):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, what="257 x 256 after 4 steps", settings=((WIDE["inflation"], "all"), (1, "all")))
    env.close()


@pytest.mark.parametrize("row", sorted(MANY))
def test_many_agents(row):
    """257 and 1024 agents on tests/agent_counts.py's maps: a wave's lanes stride over an env's blockers 5 and 16 times.
    The naive reference runs on the last env only."""
    agents, size, batch = row
    assert row in (LAYOUT_ROWS[0], (1024, 64, 2)) and MANY[row]["r"] in radii_accepted(agents, size, batch)
    obstacles, starts, targets = many_instance(row)
    env = _install(obstacles, starts, targets, MANY[row]["r"], "soft", "finish")
    rng = np.random.default_rng(agents)
    env.step(mixed_actions(env, rng, p_expert=0.8))
    want = _check(env, what=f"A={agents}", settings=((MANY[row]["inflation"], "all"),), envs=[batch - 1])
    assert want[0][batch - 1].sum() > 0
    env.close()


@pytest.mark.parametrize("size", [16, 70])
def test_inflations_and_modes(size):
    """Inflation 1, the default and 64, under both `blockers` modes, on both layouts; agents that wait on their targets
    make "on_target" differ from "all"."""
    obstacles, agents, targets = instances(3, size, size, 10, 0.35, size, cluster=3)
    targets[:, ::3] = agents[:, ::3]
    env = _install(obstacles, agents, targets, 3)
    settings = tuple((k, mode) for k in (1, 10, 64) for mode in ("all", "on_target"))
    _check(env, what=f"size {size}", settings=settings)
    c1, _ = env.blocking(inflation=1)
    c64, _ = env.blocking(inflation=64)
    con, _ = env.blocking(inflation=1, blockers="on_target")
    d = env.blocking()
    assert all(lazy_torch().equal(a, b) for a, b in zip(d, env.blocking(inflation=10, blockers="all")))
    assert bool((c64 <= c1).all()) and bool((con <= c1).all()) and int(c1.sum()) > int(c64.sum()) > 0
    assert 0 < int(con.sum()) < int(c1.sum())
    env.close()


def test_out_tensors_offset_views_and_errors():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    obstacles, agents, targets = instances(3, 12, 12, 7, 0.3, 12, cluster=2)
    gc = GridConfig(map=obstacles[0].tolist(), num_agents=7, obs_radius=2, on_target="nothing", max_episode_steps=64)
    env = VecPogema(gc, batch=3)
    with pytest.raises(PgxError) as ei:
        env.blocking()
    assert ei.value.code == -4  # before a reset, like step()
    env.reset_from_state(obstacles, agents, targets)
    want = env.blocking(inflation=2)
    assert bool(want[0].any())
    outs = tuple(torch.full((3, 7), 9, dtype=torch.int32, device=env.device) for _ in range(2))
    got = env.blocking(inflation=2, out=outs)
    assert got[0] is outs[0] and got[1] is outs[1] and all(torch.equal(g, w) for g, w in zip(got, want))
    # views one int32 past a 16-byte boundary: the same result, nothing written around them
    bufs = [torch.full((21 + 8,), 7, dtype=torch.int32, device=env.device) for _ in range(2)]
    views = tuple(b[1:22].view(3, 7) for b in bufs)
    assert views[0].data_ptr() % 16 == 4
    got = env.blocking(inflation=2, out=views)
    for g, v, w, b in zip(got, views, want, bufs):
        assert g is v and torch.equal(v, w) and bool((b[:1] == 7).all()) and bool((b[22:] == 7).all())
    for bad in (outs[0].to(torch.int64), outs[0][:, :6], torch.empty((3, 14), dtype=torch.int32, device=env.device)[:, ::2],
                torch.empty((3, 7), dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"out\[count\]"):
            env.blocking(out=(bad, outs[1]))
        with pytest.raises(ValueError, match=r"out\[blocked_by\]"):
            env.blocking(out=(outs[0], bad))
    with pytest.raises(ValueError, match="out must be"):
        env.blocking(out=(outs[0],))
    with pytest.raises(ValueError, match=r"out\[count\] is None"):
        env.blocking(out=(None, outs[1]))
    for bad in (0, -1, 65):
        with pytest.raises(ValueError, match=r"1\.\.64"):
            env.blocking(inflation=bad)
    for bad in (2.0, True, "3", None):
        with pytest.raises(TypeError, match="inflation"):
            env.blocking(inflation=bad)
    with pytest.raises(ValueError, match=r"\['all', 'on_target'\]"):
        env.blocking(blockers="goal")
    # through the C entry either output may be NULL
    only = torch.full((3, 7), 9, dtype=torch.int32, device=env.device)
    from pogema_amd import _lib
    _lib.check(env._lib.pgx_blocking(env._handle, 2, 0, only.data_ptr(), None, env._stream()))
    assert torch.equal(only, want[0])
    _lib.check(env._lib.pgx_blocking(env._handle, 2, 0, None, only.data_ptr(), env._stream()))
    assert torch.equal(only, want[1])
    env.close()

    one = pogema_v0(GridConfig(map=obstacles[0].tolist(), agents_xy=agents[0].tolist(), targets_xy=targets[0].tolist(),
                               obs_radius=2, on_target="nothing", max_episode_steps=64))
    one.reset(seed=0)
    count, blocked_by = one.blocking(inflation=2)
    assert isinstance(count, list) and isinstance(blocked_by, list) and all(type(v) is int for v in count + blocked_by)
    assert count == want[0][0].tolist() and blocked_by == want[1][0].tolist()
    assert one.blocking(inflation=2, blockers="on_target") == tuple(
        t[0].tolist() for t in one._vec.blocking(inflation=2, blockers="on_target"))
    one.close()


def test_cache_contract():
    torch = lazy_torch()
    for size in (16, 80):
        B, A = 4, 6
        obstacles, agents, targets = instances(B, size, size, A, 0.3, size + 1, cluster=3)
        # a first call on a fresh env allocates the cache and builds every field; a second one builds nothing
        env = _install(obstacles, agents, targets, 3)
        assert env.cost_to_go_builds == 0
        env.blocking(inflation=3)
        assert env.cost_to_go_builds == B * A
        _check(env, what=f"size {size} second call", settings=((3, "all"),))
        assert env.cost_to_go_builds == B * A
        env.close()
        # the cache is cost_to_go()'s: after it nothing is left to build; set_targets makes the moved agents' fields stale
        env = _install(obstacles, agents, targets, 3)
        env.cost_to_go()
        assert env.cost_to_go_builds == B * A
        env.blocking()
        assert env.cost_to_go_builds == B * A
        tgt = targets.copy()
        rng = np.random.default_rng(size)
        moved = [(0, 1), (2, 5), (3, 0)]
        for b, i in moved:
            free = np.argwhere(obstacles[b] == 0)
            free = free[(free != tgt[b, i]).any(1)]
            tgt[b, i] = free[rng.integers(len(free))]
        env.set_targets(torch.as_tensor(tgt))
        env.blocking(inflation=3)
        assert env.cost_to_go_builds == B * A + len(moved)
        _check(env, what=f"size {size} after set_targets", settings=((3, "all"),))
        env.cost_to_go()
        assert env.cost_to_go_builds == B * A + len(moved)
        env.close()


def test_first_call_inside_capture_is_refused():
    torch = lazy_torch()
    from pogema_amd._lib import PgxError
    obstacles, agents, targets = instances(2, 12, 12, 4, 0.3, 5, cluster=2)
    env = _install(obstacles, agents, targets, 2)
    out = tuple(torch.zeros((2, 4), dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError, match="bytes") as ei:
        with torch.cuda.graph(g):
            env.blocking(out=out)
    assert ei.value.code == -4
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == 0
    _check(env, what="after the refused capture", settings=((2, "all"),))
    env.close()


def test_state_untouched():
    """get_state() and the next step()'s outputs are identical with and without a preceding blocking()."""
    torch = lazy_torch()
    for size, coll, on_target in ((20, "soft", "restart"), (70, "block_both", "finish")):
        obstacles, agents, targets = instances(3, size, size, 9, 0.3, size, cluster=3)
        a = _install(obstacles, agents, targets, 3, coll, on_target, auto_reset=True, reuse_buffers=False)
        b = _install(obstacles, agents, targets, 3, coll, on_target, auto_reset=True, reuse_buffers=False)
        rng = np.random.default_rng(31)
        for t in range(4):
            acts = torch.as_tensor(rng.integers(0, 5, size=(3, 9)), device=a.device)
            before = a.get_state(occupancy=True)
            a.blocking(inflation=(1, 10, 64, 3)[t], blockers=("all", "on_target")[t % 2])
            sa, sb = a.get_state(occupancy=True), b.get_state(occupancy=True)
            for k in sa:
                assert torch.equal(sa[k], before[k]) and torch.equal(sa[k], sb[k]), f"size {size} step {t}: {k}"
            assert np.array_equal(installed_maps(a), installed_maps(b))
            ra, rb = a.step(acts), b.step(acts)
            for x, y in zip(ra[:4], rb[:4]):
                assert torch.equal(x, y), f"size {size} step {t}"
        a.close()
        b.close()


@pytest.mark.parametrize("size", [16, 72])
def test_graph_replay_equals_eager(size):
    """blocking() captured once after an eager call, on one stream; replays after further steps (and after new targets,
    which make fields stale) equal the eager result on the same state."""
    torch = lazy_torch()
    B, A = 4, 8
    obstacles, agents, targets = instances(B, size, size, A, 0.35, size + 2, cluster=3)
    env = _install(obstacles, agents, targets, 3)
    outs = tuple(torch.zeros_like(t) for t in env.blocking(inflation=3))  # eager: allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.blocking(inflation=3, out=outs)
    built = env.cost_to_go_builds
    for t in range(5):
        a, _ = env.expert_actions()
        env.step(a)
        if t == 2:                           # every agent gets the first or the last free cell, whichever is new to it
            old = env.get_state()["targets_xy"].cpu().numpy()
            free = [np.argwhere(m == 0) for m in obstacles]
            new = np.stack([np.where((old[b] == free[b][0]).all(-1, keepdims=True), free[b][-1], free[b][0])
                            for b in range(B)])
            env.set_targets(torch.as_tensor(new))
        for o in outs:
            o.fill_(-1)
        g.replay()
        if t == 2:
            torch.cuda.synchronize()
            assert env.cost_to_go_builds == built + B * A, "the replay did not rebuild the stale fields"
        for o, e in zip(outs, env.blocking(inflation=3)):
            assert torch.equal(o, e), f"step {t}"
    _check(env, what="after replays", settings=((3, "all"),))
    env.close()
