"""GPU: windowed cooperative A* (VecPogema.whca_plan / pgx_whca_plan, docs/SPEC.md S28) equals the CPU reference
(tests/whca_reference.py) applied to get_state() and the installed maps, bit for bit on all four outputs: every lane
layout, both ends of the horizon's range, boxes larger than the map and boxes clipped by its edges, non-square and large
maps, every collision system, on_target mode and action dtype, the hand-built cases.  The call keeps pibt_plan()'s
contract -- state untouched, one cache refresh per call, capturable after one eager call -- and its plan passes
path_conflicts() and is what rollout(actions) does."""
import numpy as np
import pytest

from test_visible_agents_gpu import LAYOUTS
from util import generate_instances, installed_maps, lazy_torch, mixed_actions
from whca_cases import CASES, expected, grid
from whca_reference import conflicts, whca_reference

pytestmark = pytest.mark.gpu

NAMES = ("actions", "path_xy", "arrival", "failed")


def _check(env, K, on_target, priority=None, what="", dtype=None, out=None):
    """whca_plan(K) == the reference on get_state() + the installed maps; returns (the four output tensors, the
    reference's arrays)."""
    torch = lazy_torch()
    kw = {} if dtype is None else {"dtype": dtype}
    got = env.whca_plan(K, priority=priority, out=out, **kw)
    B, A = env.batch, env.num_agents
    if out is None:
        assert got[0].dtype == (torch.int64 if dtype is None else dtype)
    assert tuple(got[0].shape) == (K, B, A)
    assert got[1].dtype == torch.int32 and tuple(got[1].shape) == (K, B, A, 2)
    for t in got[2:]:
        assert t.dtype == torch.int32 and tuple(t.shape) == (B, A)
    st = env.get_state()
    want = whca_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                          st["is_active"].cpu().numpy(), K, None if priority is None else priority.cpu().numpy(),
                          on_target=on_target)
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy().astype(w.dtype)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: "
                               f"{g[tuple(bad[0])]} vs {w[tuple(bad[0])]}")
    return got, want


def _random_priority(env, rng, low=-3, high=4):
    torch = lazy_torch()
    return torch.as_tensor(rng.integers(low, high, size=(env.batch, env.num_agents)), dtype=torch.int32, device=env.device)


@pytest.mark.parametrize("agents,size,batch", LAYOUTS)
def test_every_lane_layout_matches_reference(agents, size, batch):
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(agents)
    batch = min(batch, 24)   # the reference is a Python search per agent
    K = 6 if agents < 1024 else 3
    gc = GridConfig(size=size, num_agents=agents, obs_radius=1 + agents % 5, density=0.1, seed=agents,
                    collision_system="soft", on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=batch)
    env.reset(seed=agents)
    full = np.iinfo(np.int32)
    _check(env, K, "finish", _random_priority(env, rng, full.min, full.max + 1), what=f"A={agents} random")
    _check(env, K, "finish", None, what=f"A={agents} None")
    env.close()


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_both_ends_of_the_horizon(on_target):
    """K = 1, and K = 31 on a 12 x 12 map: the 63 x 63 box is larger than the map on every side."""
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=12, num_agents=8, obs_radius=2, density=0.3, seed=6, collision_system="soft",
                               on_target=on_target), batch=6)
    env.reset(seed=6)
    rng = np.random.default_rng(6)
    prio = _random_priority(env, rng)
    _check(env, 1, on_target, prio, what="K=1")
    (_, _, arrival, _), _ = _check(env, 31, on_target, prio, what="K=31")
    assert int((arrival > 0).sum()) > 0
    _check(env, 31, on_target, None, what="K=31 None")
    env.close()


def test_longest_horizon_inside_a_large_map():
    """K = 31 on 80 x 80: the boxes lie inside the map or are clipped by one or two of its edges (agents are put into
    the corners and on the borders too)."""
    from pogema_amd import GridConfig, VecPogema
    B, A, size = 2, 8, 80
    obstacles, agents, targets = generate_instances(B, size, size, A, 0.3, 8)
    free = [np.argwhere(obstacles[b] == 0) for b in range(B)]
    for b in range(B):       # the free cells nearest to the four corners, and two on the borders
        for i, corner in enumerate([(0, 0), (0, size - 1), (size - 1, 0), (size - 1, size - 1), (0, size // 2), (size // 2, 0)]):
            taken = {tuple(c) for k, c in enumerate(agents[b]) if k != i}
            cells = sorted((tuple(c) for c in free[b] if tuple(c) not in taken),
                           key=lambda c: abs(c[0] - corner[0]) + abs(c[1] - corner[1]))
            agents[b, i] = cells[0]
    env = VecPogema(GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=3, seed=8, collision_system="soft",
                               on_target="nothing"), batch=B)
    env.reset_from_state(obstacles, agents, targets, validate=False)
    _check(env, 31, "nothing", None, what="80x80 K=31")
    env.close()


@pytest.mark.parametrize("name,rows,cols,agents,batch", [("wide", 5, 40, 12, 11), ("tall", 37, 6, 12, 11),
                                                         ("large", 300, 300, 12, 2)])
def test_other_map_shapes(name, rows, cols, agents, batch):
    """Non-square maps; 300 x 300: more than 65536 cells, the cache's 32-bit fields."""
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(rows)
    if name == "large":
        gc = GridConfig(size=rows, num_agents=agents, obs_radius=4, density=0.2, seed=5, collision_system="soft",
                        on_target="nothing", max_episode_steps=64)
    else:
        grid_rows = "\n".join("".join("#" if (x * 7 + y * 3) % 11 == 0 else "." for y in range(cols)) for x in range(rows))
        gc = GridConfig(map=grid_rows, num_agents=agents, obs_radius=3, seed=3, collision_system="soft", on_target="nothing",
                        max_episode_steps=64)
    env = VecPogema(gc, batch=batch)
    env.reset(seed=3)
    _check(env, 9, "nothing", _random_priority(env, rng), what=name)
    env.step(mixed_actions(env, rng, p_expert=0.8))
    _check(env, 9, "nothing", None, what=name + " after a step")
    env.close()


def _shared_cells(st):
    """Active agents beyond the first on their cell, summed over the envs."""
    xy, act = st["agents_xy"].cpu().numpy(), st["is_active"].cpu().numpy()
    cells = [[tuple(p) for p, a in zip(xy[b], act[b]) if a] for b in range(len(xy))]
    return sum(len(c) - len(set(c)) for c in cells)


@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    """Finished (hidden) agents and lifelong retargets precede the plan.  Under `soft` the envs start with agents that
    share a cell; that state is planned as well, before the steps: only the bit-exactness is asserted there, S28's
    guarantee needs distinct cells."""
    from pogema_amd import GridConfig, VecPogema
    B, A, size = 12, 10, 10
    obstacles, agents, targets = generate_instances(B, size, size, A, 0.2, 7)
    if collision == "soft":
        agents[:, 1] = agents[:, 0]
        agents[:, 7] = agents[:, 5] = agents[:, 4]
    gc = GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=3, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=40)
    env = VecPogema(gc, batch=B, auto_reset=True)
    env.reset_from_state(obstacles, agents, targets, validate=collision != "soft")
    rng = np.random.default_rng(11)
    prio = _random_priority(env, rng)
    if collision == "soft":
        assert _shared_cells(env.get_state()) == 3 * B
        _check(env, 7, on_target, prio, what=f"soft/{on_target} shared cells")
        _check(env, 7, on_target, None, what=f"soft/{on_target} shared cells, no priorities")
    for t in range(30):      # a few mixed steps; under finish until an agent is hidden
        env.step(mixed_actions(env, rng, p_expert=0.6))
        if t >= 3 and (on_target != "finish" or not bool(env.get_state()["is_active"].all())):
            break
    st = env.get_state()
    if on_target == "finish":
        assert not bool(st["is_active"].all()), "no finished (hidden) agent"
    _, (_, path, _, failed, last) = _check(env, 7, on_target, prio, what=f"{collision}/{on_target}")
    if _shared_cells(st) == 0:
        xy = st["agents_xy"].cpu().numpy()
        for b in range(B):
            assert conflicts(xy[b], path[:, b], last[b], failed[b]) == []
    env.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_cases(case):
    from pogema_amd import GridConfig, VecPogema
    torch = lazy_torch()
    A, B = len(case["agents"]), 3
    env = VecPogema(GridConfig(map="\n".join(case["map"]), num_agents=A, obs_radius=2, seed=1, collision_system="soft",
                               on_target=case["on_target"]), batch=B)
    env.reset_from_state(grid(case["map"]), np.array(case["agents"], dtype=np.int32), np.array(case["targets"], dtype=np.int32),
                         validate=False)
    prio = None
    if case["priority"] is not None:
        prio = torch.as_tensor(np.array([case["priority"]] * B), dtype=torch.int32, device=env.device)
    got = env.whca_plan(case["horizon"], priority=prio)
    for name, g, w in zip(NAMES, got, expected(case)):
        w = np.repeat(w[:, None], B, 1) if name in ("actions", "path_xy") else np.repeat(w[None], B, 0)
        assert np.array_equal(g.cpu().numpy().astype(w.dtype), w), f"{case['name']}: {name}"
    env.close()


def test_unreachable_target_action_dtypes_and_out():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A, K = 9, 14, 8
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.3, seed=9, collision_system="soft",
                               on_target="nothing"), batch=B)
    env.reset(seed=9)
    rng = np.random.default_rng(9)
    # targets moved to free cells of other components where the map has one: set_targets checks only that they are free
    maps = installed_maps(env)
    st = env.get_state()
    targets = st["targets_xy"].cpu().numpy().copy()
    from expert_reference import bfs_from
    moved = 0
    for b in range(B):
        for i in range(0, A, 3):
            D = bfs_from(maps[b] != 0, *st["agents_xy"][b, i].tolist())
            far = np.argwhere((D < 0) & (maps[b] == 0))
            if len(far):
                targets[b, i] = far[rng.integers(len(far))]
                moved += 1
    assert moved > 0, "no map with two components"
    env.set_targets(targets)
    prio = _random_priority(env, rng)
    base, (_, path, _, _, _) = _check(env, K, "nothing", prio, what="unreachable targets")
    for dtype in (torch.int8, torch.int32, torch.int64):
        got, _ = _check(env, K, "nothing", prio, what=str(dtype), dtype=dtype)
        assert torch.equal(got[0].to(torch.int64), base[0]) and all(torch.equal(g, b) for g, b in zip(got[1:], base[1:]))
        assert torch.equal(env.whca_plan(K, priority=prio.to(torch.int64), dtype=dtype)[0], got[0])
    dev = env.device
    make = lambda: [torch.full((K, B, A), 99, dtype=torch.int32, device=dev), torch.full((K, B, A, 2), 99, dtype=torch.int32, device=dev),
                    torch.full((B, A), 99, dtype=torch.int32, device=dev), torch.full((B, A), 99, dtype=torch.int32, device=dev)]
    out = make()
    got, _ = _check(env, K, "nothing", prio, what="out=", out=tuple(out))
    assert all(g is o for g, o in zip(got, out))
    bad = {0: [torch.empty((K, B, A), dtype=torch.float32, device=dev), torch.empty((K + 1, B, A), dtype=torch.int32, device=dev),
               torch.empty((K, B, A), dtype=torch.int32)],
           1: [torch.empty((K, B, A, 2), dtype=torch.int64, device=dev), torch.empty((B, A, 2), dtype=torch.int32, device=dev)],
           2: [torch.empty((B, A), dtype=torch.int64, device=dev), torch.empty((B, A + 1), dtype=torch.int32, device=dev)],
           3: [torch.empty((B, 2 * A), dtype=torch.int32, device=dev)[:, ::2], None]}
    for k, tensors in bad.items():
        for t in tensors:
            o = make()
            o[k] = t
            with pytest.raises(ValueError, match="out"):
                env.whca_plan(K, out=tuple(o))
    with pytest.raises(ValueError, match="out must be"):
        env.whca_plan(K, out=tuple(make()[:3]))
    # through the C-ABI: PGX_E_INVALID, nothing is launched; the three optional outputs may be NULL
    call = env._lib.pgx_whca_plan
    assert call(env._handle, 0, 0, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 0, 32, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 1, K, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 0, K, None, None, 1, None, None, None, env._stream()) == -1
    guard = torch.full((K * B * A + 64,), 77, dtype=torch.int32, device=dev)
    assert call(env._handle, 0, K, prio.data_ptr(), guard[32:].data_ptr(), 1, None, None, None, env._stream()) == 0
    assert torch.equal(guard[32:32 + K * B * A].view(K, B, A).to(torch.int64), base[0])
    assert bool((guard[:32] == 77).all()) and bool((guard[32 + K * B * A:] == 77).all())
    env.close()


# ---- contract ---------------------------------------------------------------------------------------------------------
def test_state_untouched_and_one_refresh_per_call():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=14, num_agents=12, obs_radius=3, density=0.2, seed=31, collision_system="soft",
                    on_target="restart", max_episode_steps=32)
    env = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
    env.reset(seed=31)
    assert env.cost_to_go_builds == 0
    before = env.save_state()["engine"].clone()
    st0 = {k: v.clone() for k, v in env.get_state().items()}
    first = env.whca_plan(7)                                  # allocates the cache: one field per active agent
    n = env.cost_to_go_builds
    assert n == 8 * 12, n
    again = env.whca_plan(7, priority=torch.zeros((8, 12), dtype=torch.int64, device=env.device))
    env.whca_plan(31)
    env.pibt_plan(5)
    assert env.cost_to_go_builds == n, "a call on an unchanged state built fields"
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    assert torch.equal(env.save_state()["engine"], before)
    assert all(torch.equal(v, st0[k]) for k, v in env.get_state().items())
    env.close()


def test_first_call_inside_a_capture_is_refused_and_a_later_capture_replays():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    B, A, K = 16, 10, 6
    gc = GridConfig(size=12, num_agents=A, obs_radius=3, density=0.2, seed=4, collision_system="soft",
                    on_target="restart", max_episode_steps=24)
    env = VecPogema(gc, batch=B, auto_reset=True)
    env.reset(seed=4)
    prio = torch.zeros((B, A), dtype=torch.int32, device=env.device)
    out = (torch.zeros((K, B, A), dtype=torch.int64, device=env.device), torch.zeros((K, B, A, 2), dtype=torch.int32, device=env.device),
           torch.zeros((B, A), dtype=torch.int32, device=env.device), torch.zeros((B, A), dtype=torch.int32, device=env.device))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step(torch.zeros((B, A), dtype=torch.int64, device=env.device))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError) as ei:
        with torch.cuda.graph(g):
            env.whca_plan(K, priority=prio, out=out)
    assert ei.value.code == -4 and "capture" in str(ei.value) and "pgx_whca_plan" in str(ei.value)
    torch.cuda.synchronize()
    env.whca_plan(K, priority=prio, out=out)              # the eager call that allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.whca_plan(K, priority=prio, out=out)
    rng = np.random.default_rng(4)
    for t in range(3):
        env.step(out[0][0].clone() if t % 2 else mixed_actions(env, rng, p_expert=0.8))   # the state changes
        prio.copy_(torch.as_tensor(rng.integers(-2, 3, size=(B, A)), dtype=torch.int32))
        g.replay()
        got = [o.clone() for o in out]
        want, _ = _check(env, K, "restart", prio, what=f"replay {t}")
        assert all(torch.equal(x, y) for x, y in zip(got, want)), f"replay {t}"
    env.close()


def test_refused_horizons_and_list_view():
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=10, num_agents=9, obs_radius=3, density=0.1, seed=21, collision_system="soft"), batch=6)
    with pytest.raises(PgxError) as ei:
        env.whca_plan(3)
    assert ei.value.code == -4                           # PGX_E_STATE before a reset
    env.reset(seed=21)
    for horizon in (0, 32, 2.5, True, -3, "3", None):
        with pytest.raises(ValueError, match=r"horizon must be an integer in 1\.\.31"):
            env.whca_plan(horizon)
    env.close()

    one = pogema_v0(GridConfig(size=8, num_agents=10, obs_radius=3, density=0.0, seed=21, collision_system="soft"))
    one.reset(seed=21)
    plan = one.whca_plan(4)
    assert isinstance(plan, list) and len(plan) == 4 and all(len(row) == 10 and all(isinstance(a, int) for a in row) for row in plan)
    assert plan == one._vec.whca_plan(4)[0][:, 0].cpu().numpy().tolist()
    assert isinstance(one.whca_plan(2, priority=list(range(10))), list)
    for row in plan:
        one.step(row)
    one.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------
E2E = dict(size=16, agents=16, batch=48, K=16, seed=4)


def test_plan_passes_path_conflicts_and_is_what_rollout_does():
    """soft / finish: in the envs without a failed agent the plan has no vertex and no edge conflict by path_conflicts()'
    own count, and rollout(actions) walks it: every agent still active afterwards stands on path_xy[K - 1], every agent
    with arrival >= 1 has finished."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    c = E2E
    K, B, A = c["K"], c["batch"], c["agents"]
    obstacles, agents, targets = generate_instances(B, c["size"], c["size"], A, 0.3, c["seed"])
    # the seed was chosen with the reference alone: at most a quarter of the envs hold a failed agent
    ref = whca_reference(obstacles, agents, targets, np.ones((B, A), dtype=bool), K, None, "finish")
    ref_left_out = int((ref[3].sum(axis=1) > 0).sum())
    assert 4 * ref_left_out <= B, ref_left_out

    gc = GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=3, seed=c["seed"], collision_system="soft",
                    on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=B, auto_reset=False)
    env.reset_from_state(obstacles, agents, targets)
    actions, path_xy, arrival, failed = env.whca_plan(K)
    for name, g, w in zip(NAMES, (actions, path_xy, arrival, failed), ref):
        assert np.array_equal(g.cpu().numpy().astype(w.dtype), w), name
    clean = failed.sum(dim=1) == 0
    left_out = B - int(clean.sum())
    print(f"whca end to end: {left_out} of {B} envs left out for holding a failed agent")
    assert 4 * left_out <= B, left_out
    count = env.path_conflicts(path_xy, kinds=("vertex", "edge"))[3]
    assert int(count[clean].sum()) == 0
    assert int((arrival >= 1).sum()) * 2 >= B * A, "fewer than half of the agents arrive inside the window"

    env.rollout(actions, obs_slots=0)
    st = env.get_state()
    on = st["is_active"] & clean.view(-1, 1)
    assert bool(on.any())
    assert torch.equal(st["agents_xy"][on], path_xy[K - 1][on])
    assert not bool((st["is_active"] & (arrival >= 1) & clean.view(-1, 1)).any())
    env.close()
