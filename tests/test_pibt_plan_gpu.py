"""GPU: the multi-step planner (VecPogema.pibt_plan / pgx_pibt_plan, docs/SPEC.md S16) equals the CPU reference
(tests/pibt_plan_reference.py) applied to get_state() and the installed maps, bit for bit on all four outputs: every lane
layout, non-square and large maps, every collision system, on_target mode and action dtype, fixed priorities, both ends
of the horizon's range.  The plan agrees with the existing path -- PibtPolicy.act() / step() / update() step by step,
and rollout(actions) -- and keeps pibt_actions()' contract: state untouched, one cache refresh per call, capturable
after one eager call."""
import numpy as np
import pytest

from pibt_plan_reference import pibt_plan_reference
from test_visible_agents_gpu import LAYOUTS
from util import generate_instances, installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

NAMES = ("actions", "path_xy", "arrival", "priority")


def _check(env, K, on_target, priority=None, what="", dtype=None, growing=True):
    """pibt_plan(K) == the reference on get_state() + the installed maps; returns the four output tensors."""
    torch = lazy_torch()
    kw = {} if dtype is None else {"dtype": dtype}
    got = env.pibt_plan(K, priority=priority, growing=growing, **kw)
    B, A = env.batch, env.num_agents
    assert got[0].dtype == (torch.int64 if dtype is None else dtype) and tuple(got[0].shape) == (K, B, A)
    assert got[1].dtype == torch.int32 and tuple(got[1].shape) == (K, B, A, 2)
    for t in got[2:]:
        assert t.dtype == torch.int32 and tuple(t.shape) == (B, A)
    st = env.get_state()
    want = pibt_plan_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                               st["is_active"].cpu().numpy(), K, None if priority is None else priority.cpu().numpy(),
                               on_target=on_target, growing=growing)
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy().astype(w.dtype)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: "
                               f"{g[tuple(bad[0])]} vs {w[tuple(bad[0])]}")
    return got


def _random_priority(env, rng, low=-3, high=4):
    torch = lazy_torch()
    return torch.as_tensor(rng.integers(low, high, size=(env.batch, env.num_agents)), dtype=torch.int32, device=env.device)


@pytest.mark.parametrize("agents,size,batch", LAYOUTS)
def test_every_lane_layout_matches_reference(agents, size, batch):
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(agents)
    batch = min(batch, 24)   # the reference is a Python recursion per env and step; the last workgroup stays partly filled
    K = 6 if agents < 1024 else 3
    gc = GridConfig(size=size, num_agents=agents, obs_radius=1 + agents % 5, density=0.1, seed=agents,
                    collision_system="soft", on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=batch)
    env.reset(seed=agents)
    full = np.iinfo(np.int32)
    _, _, arrival, _ = _check(env, K, "finish", _random_priority(env, rng, full.min, full.max + 1), what=f"A={agents} random")
    _check(env, K, "finish", None, what=f"A={agents} None")
    if agents <= 16:         # (on the larger maps of the larger layouts six steps are too few)
        assert int((arrival > 0).sum()) > 0, "no agent arrived inside the horizon"
    env.close()


@pytest.mark.parametrize("name,rows,cols,agents,batch", [("wide", 5, 40, 12, 11), ("tall", 37, 6, 12, 11),
                                                         ("large", 300, 300, 12, 2)])
def test_other_map_shapes(name, rows, cols, agents, batch):
    """Non-square maps; 300 x 300: more than 65536 cells, the cache's 32-bit fields."""
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(rows)
    if name == "large":
        gc = GridConfig(size=rows, num_agents=agents, obs_radius=4, density=0.2, seed=5, collision_system="soft",
                        on_target="finish", max_episode_steps=64)
    else:
        grid = "\n".join("".join("#" if (x * 7 + y * 3) % 11 == 0 else "." for y in range(cols)) for x in range(rows))
        gc = GridConfig(map=grid, num_agents=agents, obs_radius=3, seed=3, collision_system="soft", on_target="finish",
                        max_episode_steps=64)
    env = VecPogema(gc, batch=batch)
    env.reset(seed=3)
    _check(env, 4, "finish", _random_priority(env, rng), what=name)
    env.step(mixed_actions(env, rng, p_expert=0.8))
    _check(env, 4, "finish", None, what=name + " after a step")
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
    share a cell (two on one cell, three on another: S13's `now` is the lowest of them), which the engine's own steps
    produce too rarely to wait for; that state is planned as well, before the steps."""
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
        _check(env, 5, on_target, prio, what=f"soft/{on_target} shared cells")
        _check(env, 5, on_target, None, what=f"soft/{on_target} shared cells, no priorities")
    for t in range(30):      # a few mixed steps; under finish until an agent is hidden
        env.step(mixed_actions(env, rng, p_expert=0.6))
        if t >= 3 and (on_target != "finish" or not bool(env.get_state()["is_active"].all())):
            break
    if on_target == "finish":
        assert not bool(env.get_state()["is_active"].all()), "no finished (hidden) agent"
    _check(env, 5, on_target, prio, what=f"{collision}/{on_target}")
    _check(env, 5, on_target, prio, what=f"{collision}/{on_target} fixed", growing=False)
    env.close()


def test_every_action_dtype_and_horizon_one():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=10, num_agents=14, obs_radius=3, density=0.2, seed=9, collision_system="soft",
                               on_target="finish"), batch=9)
    env.reset(seed=9)
    rng = np.random.default_rng(9)
    prio = _random_priority(env, rng)
    base = _check(env, 5, "finish", prio, what="int64")
    for dtype in (torch.int8, torch.int32, torch.int64):
        got = _check(env, 5, "finish", prio, what=str(dtype), dtype=dtype)
        assert torch.equal(got[0].to(torch.int64), base[0]) and all(torch.equal(g, b) for g, b in zip(got[1:], base[1:]))
        # any integer dtype of `priority` is converted
        assert torch.equal(env.pibt_plan(5, priority=prio.to(torch.int64), dtype=dtype)[0], got[0])
    # horizon = 1 is pibt_actions() on the same state
    for p in (prio, None):
        for dtype in (torch.int8, torch.int64):
            one_a, one_n = env.pibt_actions(priority=p, dtype=dtype)
            a, path, _, _ = env.pibt_plan(1, priority=p, dtype=dtype)
            assert torch.equal(a[0], one_a) and torch.equal(path[0], one_n)
    env.close()


def test_longest_horizon():
    from pogema_amd import GridConfig, VecPogema
    for on_target in ("finish", "nothing"):
        env = VecPogema(GridConfig(size=6, num_agents=3, obs_radius=2, density=0.2, seed=2, collision_system="soft",
                                   on_target=on_target), batch=2)
        env.reset(seed=2)
        _, _, arrival, _ = _check(env, 256, on_target, None, what=f"K=256 {on_target}")
        assert int((arrival > 0).sum()) > 0
        env.close()


# ---- agreement with the existing path -------------------------------------------------------------------------------
AGREE = dict(size=16, agents=12, batch=64, K=8, seed=3)


def _agreement_case(on_target):
    """The seeded instances and what the reference alone says about them: the envs whose episode outlasts the plan (under
    `finish` an episode ends when every agent has arrived, under `nothing` when all stand on their targets at once) and
    the arrivals inside it."""
    c = AGREE
    obstacles, agents, targets = generate_instances(c["batch"], c["size"], c["size"], c["agents"], 0.3, c["seed"])
    active = np.ones(agents.shape[:2], dtype=bool)
    _, path, arrival, _, planned = pibt_plan_reference(obstacles, agents, targets, active, c["K"], on_target=on_target)
    if on_target == "finish":
        ended = ~planned[1:].any(axis=2)                              # [K, B]: nobody is left after step h
    else:
        ended = (path == targets[None]).all(axis=3).all(axis=2)
    return obstacles, agents, targets, ended.any(axis=0), arrival


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_plan_agrees_with_policy_steps_and_with_rollout(on_target):
    torch = lazy_torch()
    from pogema_amd import GridConfig, PibtPolicy, VecPogema
    c = AGREE
    K, B, A = c["K"], c["batch"], c["agents"]
    obstacles, agents, targets, ref_ended, ref_arrival = _agreement_case(on_target)
    # the seed was picked so that the reference alone meets both conditions
    assert int((~ref_ended).sum()) * 2 >= B
    assert bool(((ref_arrival > 0) & (ref_arrival <= K))[~ref_ended].any())

    gc = GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=3, seed=c["seed"], collision_system="soft",
                    on_target=on_target, max_episode_steps=64)
    envs = [VecPogema(gc, batch=B, auto_reset=False) for _ in range(3)]
    for env in envs:
        env.reset_from_state(obstacles, agents, targets)
    planner, stepper, roller = envs

    actions, path_xy, arrival, priority = planner.pibt_plan(K)

    policy = PibtPolicy(stepper)
    alive = torch.ones(B, dtype=torch.bool, device=stepper.device)      # envs whose episode has not ended so far
    full = torch.zeros(B, dtype=torch.bool, device=stepper.device)
    for h in range(K):
        a, next_xy = policy.act()
        assert torch.equal(a[alive], actions[h][alive]), f"step {h}: actions"
        assert torch.equal(next_xy[alive], path_xy[h][alive]), f"step {h}: next_xy"
        out = stepper.step(a)
        policy.update(out[1], out[4]["episode_done"])
        assert torch.equal(stepper.get_state()["agents_xy"][alive], path_xy[h][alive]), f"step {h}: agents_xy"
        alive = alive & ~out[4]["episode_done"].to(torch.bool)
        if h == K - 2:
            full = alive.clone()        # compared through all eight steps: no episode_done before the last one
    assert int(full.sum()) * 2 >= B, int(full.sum())
    assert bool(((arrival > 0) & (arrival <= K))[full].any())
    assert torch.equal(policy.priority[alive], priority[alive])

    roller.rollout(actions, obs_slots=0)
    st = roller.get_state()
    on = st["is_active"] & alive.view(-1, 1)
    assert bool(on.any())
    assert torch.equal(st["agents_xy"][on], path_xy[K - 1][on])
    for env in envs:
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
    first = env.pibt_plan(7)                                  # allocates the cache: one field per active agent
    n = env.cost_to_go_builds
    assert n == 8 * 12, n
    again = env.pibt_plan(7, priority=torch.zeros((8, 12), dtype=torch.int64, device=env.device))
    env.pibt_plan(32, growing=False)
    env.pibt_actions()
    assert env.cost_to_go_builds == n, "a call on an unchanged state built fields"
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    assert torch.equal(env.save_state()["engine"], before)
    env.close()


def test_first_call_inside_a_capture_is_refused_and_a_later_capture_replays():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    B, A, K = 16, 10, 4
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
            env.pibt_plan(K, priority=prio, out=out)
    assert ei.value.code == -4 and "capture" in str(ei.value) and "pgx_pibt_plan" in str(ei.value)
    torch.cuda.synchronize()
    env.pibt_plan(K, priority=prio, out=out)              # the eager call that allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.pibt_plan(K, priority=prio, out=out)
    rng = np.random.default_rng(4)
    for t in range(3):
        env.step(out[0][0].clone() if t % 2 else mixed_actions(env, rng, p_expert=0.8))   # the state changes
        prio.copy_(torch.as_tensor(rng.integers(-2, 3, size=(B, A)), dtype=torch.int32))
        g.replay()
        got = [o.clone() for o in out]
        want = _check(env, K, "restart", prio, what=f"replay {t}")
        assert all(torch.equal(x, y) for x, y in zip(got, want)), f"replay {t}"
    env.close()


def test_out_tensors_refused_arguments_and_list_view():
    torch = lazy_torch()
    from pogema_amd import GridConfig, PibtPolicy, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    B, A, K = 6, 9, 3
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.1, seed=21, collision_system="soft"), batch=B)
    with pytest.raises(PgxError) as ei:
        env.pibt_plan(K)
    assert ei.value.code == -4                           # PGX_E_STATE before a reset
    env.reset(seed=21)
    want = env.pibt_plan(K)
    dev = env.device
    make = lambda: [torch.full((K, B, A), 99, dtype=torch.int32, device=dev), torch.full((K, B, A, 2), 99, dtype=torch.int32, device=dev),
                    torch.full((B, A), 99, dtype=torch.int32, device=dev), torch.full((B, A), 99, dtype=torch.int32, device=dev)]
    out = make()
    got = env.pibt_plan(K, out=tuple(out))
    assert all(g is o for g, o in zip(got, out))
    assert torch.equal(out[0].to(torch.int64), want[0]) and all(torch.equal(o, w) for o, w in zip(out[1:], want[1:]))
    bad = {0: [torch.empty((K, B, A), dtype=torch.float32, device=dev), torch.empty((K + 1, B, A), dtype=torch.int32, device=dev),
               torch.empty((B, A), dtype=torch.int32, device=dev), torch.empty((K, B, A), dtype=torch.int32)],
           1: [torch.empty((K, B, A, 2), dtype=torch.int64, device=dev), torch.empty((B, A, 2), dtype=torch.int32, device=dev)],
           2: [torch.empty((B, A), dtype=torch.int64, device=dev), torch.empty((B, A + 1), dtype=torch.int32, device=dev)],
           3: [torch.empty((B, 2 * A), dtype=torch.int32, device=dev)[:, ::2], None]}
    for k, tensors in bad.items():
        for t in tensors:
            o = make()
            o[k] = t
            with pytest.raises(ValueError, match="out"):
                env.pibt_plan(K, out=tuple(o))
    with pytest.raises(ValueError, match="out must be"):
        env.pibt_plan(K, out=tuple(make()[:3]))
    for horizon in (0, 257, -3, 2.5, "3", None):
        with pytest.raises(ValueError, match="horizon"):
            env.pibt_plan(horizon)
    # through the C-ABI with a handle: PGX_E_INVALID, nothing is launched; the three optional outputs may be NULL
    call = env._lib.pgx_pibt_plan
    assert call(env._handle, 0, 0, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 0, 257, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 4, K, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 0, K, None, None, 1, None, None, None, env._stream()) == -1
    guard = torch.full((K * B * A + 64,), 77, dtype=torch.int32, device=dev)
    assert call(env._handle, 0, K, None, guard[32:].data_ptr(), 1, None, None, None, env._stream()) == 0
    assert torch.equal(guard[32:32 + K * B * A].view(K, B, A).to(torch.int64), want[0])
    assert bool((guard[:32] == 77).all()) and bool((guard[32 + K * B * A:] == 77).all())

    # PibtPolicy.plan: the priorities go in and the final ones are kept
    policy = PibtPolicy(env)
    policy.priority += 3
    a, path, arrival = policy.plan(K)
    ref = env.pibt_plan(K, priority=torch.full((B, A), 3, dtype=torch.int32, device=dev))
    assert torch.equal(a, ref[0]) and torch.equal(path, ref[1]) and torch.equal(arrival, ref[2])
    assert torch.equal(policy.priority, ref[3])
    env.close()

    one = pogema_v0(GridConfig(size=8, num_agents=10, obs_radius=3, density=0.0, seed=21, collision_system="soft"))
    one.reset(seed=21)
    plan = one.pibt_plan(4)
    assert isinstance(plan, list) and len(plan) == 4 and all(len(row) == 10 and all(isinstance(a, int) for a in row) for row in plan)
    assert plan == one._vec.pibt_plan(4)[0][:, 0].cpu().numpy().tolist()
    assert plan[0] == one.pibt_actions()
    assert isinstance(one.pibt_plan(2, priority=list(range(10))), list)
    for row in plan:
        one.step(row)
    one.close()
