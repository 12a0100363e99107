"""GPU: the multi-step planner with the swap operation (VecPogema.pibt_plan(swap=True) / pgx_pibt_swap_plan, docs/SPEC.md
S27) equals the CPU reference (tests/pibt_swap_plan_reference.py) applied to get_state() and the installed maps, bit for
bit on all four outputs: every lane layout on states in which lists are reversed at steps after the first, the dead end
the plain plan never leaves, every collision system and on_target mode, both ends of the horizon's range, non-square
maps, 32-bit fields, a map pool, new targets, the walk cap on either side.  The plan agrees with the step-by-step policy
with swap and with rollout(actions), leaves the plain plan as it was, and keeps pibt_plan()'s contract: state untouched,
one cache refresh per call, capturable after one eager call."""
import numpy as np
import pytest

from pibt_plan_reference import pibt_plan_reference
from pibt_swap_cases import CAP_LENGTHS, DEAD_END, grid, head_on_instances, serpentine
from pibt_swap_plan_cases import AGREE, LATE_MIN, add_counts, agreement_case, meets, plan_case
from pibt_swap_plan_reference import late, pibt_swap_plan_reference
from pibt_swap_reference import MAX_WALK
from test_visible_agents_gpu import LAYOUTS
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

NAMES = ("actions", "path_xy", "arrival", "priority")


def _state(env):
    st = env.get_state()
    return (installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(), st["is_active"].cpu().numpy())


def _compare(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy().astype(w.dtype)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: "
                               f"{g[tuple(bad[0])]} vs {w[tuple(bad[0])]}")


def _check(env, K, on_target, priority=None, what="", dtype=None, growing=True, total=None):
    """pibt_plan(K, swap=True) == the reference on get_state() + the installed maps; returns the four output tensors
    and the reference's counters [K, B], which it also adds to `total` (pibt_swap_plan_cases.add_counts)."""
    torch = lazy_torch()
    kw = {} if dtype is None else {"dtype": dtype}
    got = env.pibt_plan(K, priority=priority, growing=growing, swap=True, **kw)
    B, A = env.batch, env.num_agents
    assert got[0].dtype == (torch.int64 if dtype is None else dtype) and tuple(got[0].shape) == (K, B, A)
    assert got[1].dtype == torch.int32 and tuple(got[1].shape) == (K, B, A, 2)
    for t in got[2:]:
        assert t.dtype == torch.int32 and tuple(t.shape) == (B, A)
    want = pibt_swap_plan_reference(*_state(env), K, None if priority is None else priority.cpu().numpy(),
                                    on_target=on_target, growing=growing)
    _compare(got, want, what)
    if total is not None:
        add_counts(total, want[5])
    return got, want[5]


def _dev(env, a, dtype=None):
    torch = lazy_torch()
    return None if a is None else torch.as_tensor(a, dtype=dtype or torch.int32, device=env.device)


def _random_priority(env, rng, low=-3, high=4):
    return _dev(env, rng.integers(low, high, size=(env.batch, env.num_agents)))


def _install(obstacles, agents, targets, **kw):
    """Installs states [B, ...] on their own maps (one hand-built state: pass it with a leading axis of 1)."""
    from pogema_amd import GridConfig, VecPogema
    obstacles = np.asarray(obstacles, dtype=np.uint8)
    agents, targets = np.asarray(agents, dtype=np.int32), np.asarray(targets, dtype=np.int32)
    text = "\n".join("".join("#" if v else "." for v in row) for row in obstacles[0])
    cfg = dict(map=text, num_agents=agents.shape[1], obs_radius=2, seed=1, collision_system="soft", on_target="finish",
               max_episode_steps=64)
    cfg.update(kw)
    env = VecPogema(GridConfig(**cfg), batch=len(agents), auto_reset=False)
    env.reset_from_state(obstacles, agents, targets)
    return env


@pytest.mark.parametrize("agents,size,batch", LAYOUTS)
def test_every_lane_layout_matches_reference(agents, size, batch):
    """pibt_swap_plan_cases.plan_case's states under a random priority over the whole int32 range and under None.  The
    reference's late counts on the installed states are at least LATE_MIN[agents]: a change of a generator cannot hollow
    the case out (tests/test_pibt_swap_plan.py recounts the layouts up to 200 agents without a device)."""
    from pogema_amd import GridConfig, VecPogema
    total = {}
    for obstacles, pos, tgt, prio, side, r, K in plan_case(agents, size, batch):
        gc = GridConfig(size=side, num_agents=agents, obs_radius=r, density=0.3, seed=agents, collision_system="soft",
                        on_target="finish", max_episode_steps=64)
        env = VecPogema(gc, batch=len(pos))
        env.reset_from_state(obstacles, pos, tgt)
        _check(env, K, "finish", _dev(env, prio), what=f"A={agents} random", total=total)
        _check(env, K, "finish", None, what=f"A={agents} None", total=total)
        env.close()
    print(agents, total)
    assert meets(total, agents) == [], (total, LATE_MIN[agents])


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_dead_end_plan_arrives_and_the_rollout_follows_it(on_target):
    torch = lazy_torch()
    rows, agents, targets = DEAD_END
    env = _install(grid(rows)[None], [agents], [targets], on_target=on_target)
    (actions, path_xy, arrival, priority), count = _check(env, 9, on_target, None, what="dead end")
    assert arrival[0].tolist() == [9, 8] and priority[0].tolist() == [0, 0]
    assert count["reversed"][:, 0].tolist() == count["pulled"][:, 0].tolist() == [0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert env.pibt_plan(9)[2][0].tolist() == [-1, -1], "the plain plan was expected to stay in the dead end"
    assert path_xy[-1, 0].tolist() == [list(t) for t in targets]
    env.rollout(actions, obs_slots=0)
    st = env.get_state()
    if on_target == "nothing":
        assert torch.equal(st["agents_xy"], st["targets_xy"])
    else:
        assert not bool(st["is_active"].any()), "an agent did not finish"
    env.close()


def _shared_cells(st):
    """Active agents beyond the first on their cell, summed over the envs."""
    xy, act = st["agents_xy"].cpu().numpy(), st["is_active"].cpu().numpy()
    cells = [[tuple(p) for p, a in zip(xy[b], act[b]) if a] for b in range(len(xy))]
    return sum(len(c) - len(set(c)) for c in cells)


@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    """Head-on states; finished (hidden) agents and lifelong retargets precede the plan.  Under `soft` the envs start
    with agents that share a cell (two on one cell, three on another: `now` is the lowest of them, in the table the
    walks use as in the candidate lists); that state is planned as well, before the steps."""
    from pogema_amd import GridConfig, VecPogema
    B, A, size = 12, 10, 10
    obstacles, agents, targets, _ = head_on_instances(B, size, A, seed=7)
    if collision == "soft":
        agents = agents.copy()
        agents[:, 1] = agents[:, 0]
        agents[:, 7] = agents[:, 5] = agents[:, 4]
    gc = GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=3, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=40)
    env = VecPogema(gc, batch=B, auto_reset=True)
    env.reset_from_state(obstacles, agents, targets, validate=collision != "soft")
    rng = np.random.default_rng(11)
    prio = _random_priority(env, rng)
    total = {}
    if collision == "soft":
        assert _shared_cells(env.get_state()) == 3 * B
        _check(env, 5, on_target, prio, what=f"soft/{on_target} shared cells", total=total)
        _check(env, 5, on_target, None, what=f"soft/{on_target} shared cells, no priorities", total=total)
    for t in range(30):      # a few mixed steps; under finish until an agent is hidden
        env.step(mixed_actions(env, rng, p_expert=0.6))
        if t >= 3 and (on_target != "finish" or not bool(env.get_state()["is_active"].all())):
            break
    if on_target == "finish":
        assert not bool(env.get_state()["is_active"].all()), "no finished (hidden) agent"
    _check(env, 5, on_target, prio, what=f"{collision}/{on_target}", total=total)
    _check(env, 5, on_target, prio, what=f"{collision}/{on_target} fixed", growing=False, total=total)
    print(collision, on_target, total)
    env.close()


def _head_on_env(batch=9, size=10, agents=14, seed=9, **kw):
    from pogema_amd import GridConfig, VecPogema
    obstacles, pos, tgt, _ = head_on_instances(batch, size, agents, seed=seed)
    cfg = dict(size=size, num_agents=agents, obs_radius=3, density=0.3, seed=seed, collision_system="soft")
    cfg.update(kw)
    env = VecPogema(GridConfig(**cfg), batch=batch)
    env.reset_from_state(obstacles, pos, tgt)
    return env


def test_every_action_dtype_and_horizon_one():
    torch = lazy_torch()
    env = _head_on_env()
    prio = _random_priority(env, np.random.default_rng(9))
    base, _ = _check(env, 5, "finish", prio, what="int64")
    for dtype in (torch.int8, torch.int32, torch.int64):
        got, _ = _check(env, 5, "finish", prio, what=str(dtype), dtype=dtype)
        assert torch.equal(got[0].to(torch.int64), base[0]) and all(torch.equal(g, b) for g, b in zip(got[1:], base[1:]))
        # any integer dtype of `priority` is converted
        assert torch.equal(env.pibt_plan(5, priority=prio.to(torch.int64), dtype=dtype, swap=True)[0], got[0])
    # horizon = 1 is pibt_actions(swap=True) on the same state, which differs from the plain planner's here
    for p in (prio, None):
        for dtype in (torch.int8, torch.int32, torch.int64):
            one_a, one_n = env.pibt_actions(priority=p, dtype=dtype, swap=True)
            a, path, _, _ = env.pibt_plan(1, priority=p, dtype=dtype, swap=True)
            assert torch.equal(a[0], one_a) and torch.equal(path[0], one_n)
        assert not torch.equal(env.pibt_actions(priority=p)[0], env.pibt_plan(1, priority=p, swap=True)[0][0])
    env.close()


def test_longest_horizon():
    for on_target in ("finish", "nothing"):
        obstacles, pos, tgt, _ = head_on_instances(4, 10, 8, seed=2)
        env = _install(obstacles, pos, tgt, on_target=on_target, max_episode_steps=512)
        (_, _, arrival, _), count = _check(env, 256, on_target, None, what=f"K=256 {on_target}")
        assert int((arrival > 0).sum()) > 0 and int(count["reversed"].sum()) > 0
        env.close()


def test_plain_plan_is_unchanged():
    """pibt_plan(K) before and after a swap plan on the same state: identical, equal to its own reference, and not what
    the swap plan answers."""
    torch = lazy_torch()
    env = _head_on_env()
    prio = _random_priority(env, np.random.default_rng(9))
    for p in (None, prio):
        before = env.pibt_plan(6, priority=p)
        swapped = env.pibt_plan(6, priority=p, swap=True)
        after = env.pibt_plan(6, priority=p)
        explicit = env.pibt_plan(6, priority=p, swap=False)
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(before, after, explicit))
        want = pibt_plan_reference(*_state(env), 6, None if p is None else p.cpu().numpy(), on_target="finish")
        _compare(before, want, "plain plan")
        assert not torch.equal(swapped[0], before[0])
    env.close()


# ---- agreement with the existing path -------------------------------------------------------------------------------
@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_plan_agrees_with_policy_steps_and_with_rollout(on_target):
    """Corridor states on which lists are reversed at steps h >= 1: K iterations of PibtPolicy(env, swap=True).act() /
    step() / update() visit path_xy's cells and end with priority_out, until an env's episode ends; rollout(actions)
    ends on the same cells."""
    torch = lazy_torch()
    from pogema_amd import PibtPolicy
    K = AGREE["K"]
    obstacles, agents, targets = agreement_case()
    B = len(agents)
    planner, stepper, roller = (_install(obstacles, agents, targets, on_target=on_target, obs_radius=3) for _ in range(3))
    (actions, path_xy, arrival, priority), count = _check(planner, K, on_target, None, what=f"agreement {on_target}")
    assert late(count, "reversed") >= 5 and late(count, "pulled") >= 5, "no late reversals on the agreement states"

    policy = PibtPolicy(stepper, swap=True)
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
            full = alive.clone()        # compared through all K steps: no episode_done before the last one
    assert int(full.sum()) * 2 >= B, int(full.sum())
    late_rows = torch.as_tensor(count["reversed"][1:].sum(axis=0) > 0, device=full.device)
    assert bool((full & late_rows).any()), "no env with a late reversal was compared through all steps"
    assert torch.equal(policy.priority[alive], priority[alive])
    # PibtPolicy.plan(swap=True) is the same plan and keeps the final priorities
    planned = PibtPolicy(planner, swap=True)
    a2, path2, arrival2 = planned.plan(K, swap=True)
    assert torch.equal(a2, actions) and torch.equal(path2, path_xy) and torch.equal(arrival2, arrival)
    assert torch.equal(planned.priority, priority)

    roller.rollout(actions, obs_slots=0)
    st = roller.get_state()
    on = st["is_active"] & alive.view(-1, 1)
    assert bool(on.any())
    assert torch.equal(st["agents_xy"][on], path_xy[K - 1][on])
    for env in (planner, stepper, roller):
        env.close()


# ---- maps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows,cols", [("wide", 5, 40), ("tall", 37, 6)])
def test_non_square_maps(name, rows, cols):
    from pogema_amd import GridConfig, VecPogema
    text = "\n".join("".join("#" if (x * 7 + y * 3) % 11 == 0 or (x % 2 and y % 5) else "." for y in range(cols))
                     for x in range(rows))
    rng = np.random.default_rng(rows)
    env = VecPogema(GridConfig(map=text, num_agents=12, obs_radius=3, seed=3, collision_system="soft", on_target="finish",
                               max_episode_steps=64), batch=11)
    env.reset(seed=3)
    total = {}
    _check(env, 6, "finish", _random_priority(env, rng), what=name, total=total)
    env.step(mixed_actions(env, rng, p_expert=0.8))
    _check(env, 6, "finish", None, what=name + " after a step", total=total)
    print(name, total)
    env.close()


def test_head_on_pairs_on_a_large_map_with_32_bit_fields():
    """300 x 300 at density 0.3 with 12 agents, most of them in head-on pairs: more than 65536 cells, walks over the
    cache's 32-bit fields at every step."""
    from pogema_amd import GridConfig, VecPogema
    obstacles, pos, tgt, _ = head_on_instances(2, 300, 12, seed=300)
    env = VecPogema(GridConfig(size=300, num_agents=12, obs_radius=4, density=0.3, seed=5, collision_system="soft",
                               on_target="nothing", max_episode_steps=64), batch=2)
    env.reset_from_state(obstacles, pos, tgt)
    total = {}
    _check(env, 4, "nothing", None, what="300 head on", total=total)
    _check(env, 4, "nothing", _random_priority(env, np.random.default_rng(3)), what="300 head on, priorities", total=total)
    print("300 x 300:", total)
    assert total["first"]["reversed"] + total["reversed"] >= 1, total
    env.close()


def test_map_pool_and_set_targets():
    """A map pool, then new targets for some agents: the targets change, the next plan refreshes the cache once, and only
    the fields of the moved targets are rebuilt."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(77)
    H = W = 14
    B, A = 10, 6
    pool = (rng.random((5, H, W)) < 0.3).astype(np.uint8)
    env = VecPogema(GridConfig(size=H, num_agents=A, obs_radius=3, seed=2, collision_system="soft", on_target="nothing",
                               max_episode_steps=32), batch=B, map_pool=torch.as_tensor(pool))
    env.reset(seed=2)
    assert len(set(env.map_index.cpu().numpy().tolist())) > 1
    prio = _random_priority(env, rng)
    _check(env, 5, "nothing", prio, what="pool reset")
    built = env.cost_to_go_builds
    assert built == B * A
    # new targets for the first two agents of every env: each other's cells, head on wherever they stand
    maps, pos, tgt, _ = _state(env)
    new = tgt.copy()
    new[:, 0], new[:, 1] = pos[:, 1], pos[:, 0]
    moved = int((new != tgt).any(axis=2).sum())
    assert moved >= B
    env.set_targets(new)
    assert np.array_equal(env.get_state()["targets_xy"].cpu().numpy(), new)
    _check(env, 5, "nothing", prio, what="after set_targets")
    assert env.cost_to_go_builds == built + moved
    _check(env, 9, "nothing", None, what="after set_targets, again")
    assert env.cost_to_go_builds == built + moved
    env.close()


@pytest.mark.parametrize("name", list(CAP_LENGTHS))
def test_walk_cap(name):
    """K = 2 only: every lane may walk the whole cap in every step.  Below the cap the pair swaps in at both steps; above
    it both steps are the plain plan's."""
    torch = lazy_torch()
    obstacles, agents, targets = serpentine(CAP_LENGTHS[name])
    env = _install(obstacles[None], [agents], [targets])
    (actions, _, _, _), count = _check(env, 2, "finish", None, what=name)
    if name == "below the cap":
        assert count["reversed"][:, 0].tolist() == [1, 1] and count["pulled"][:, 0].tolist() == [1, 1]
        assert int(count["longest_walk"].max()) == MAX_WALK - 1
        assert actions[0, 0].tolist() != [0, 0]
    else:
        assert int(count["reversed"].sum()) == 0 and int(count["longest_walk"].max()) == MAX_WALK
        plain = env.pibt_plan(2)
        assert all(torch.equal(x, y) for x, y in zip(env.pibt_plan(2, swap=True), plain))
        assert actions[:, 0].tolist() == [[0, 0], [0, 0]]
    env.close()


# ---- contract ---------------------------------------------------------------------------------------------------------
def test_state_untouched_and_one_refresh_per_call():
    torch = lazy_torch()
    env = _head_on_env(batch=8, size=14, agents=12, seed=31, on_target="restart", max_episode_steps=32)
    assert env.cost_to_go_builds == 0
    before = env.save_state()["engine"].clone()
    first = env.pibt_plan(7, swap=True)                       # allocates the cache: one field per active agent
    n = env.cost_to_go_builds
    assert n == 8 * 12, n
    again = env.pibt_plan(7, priority=torch.zeros((8, 12), dtype=torch.int64, device=env.device), swap=True)
    env.pibt_plan(32, growing=False, swap=True)
    env.pibt_plan(1, swap=True)
    env.pibt_actions(swap=True)
    assert env.cost_to_go_builds == n, "a call on an unchanged state built fields"
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    assert torch.equal(env.save_state()["engine"], before)
    env.close()


def test_cache_is_shared_with_the_plain_plan():
    for first in ("swap", "plain"):
        env = _head_on_env(batch=20, size=16, agents=8, seed=5, max_episode_steps=64)
        assert env.cost_to_go_builds == 0
        calls = {"swap": lambda: env.pibt_plan(4, swap=True), "plain": lambda: env.pibt_plan(4)}
        second = "plain" if first == "swap" else "swap"
        calls[first]()
        n = env.cost_to_go_builds
        assert n == int(env.get_state()["is_active"].sum()), (first, n)   # one field per active agent, whoever asked first
        calls[second]()
        assert env.cost_to_go_builds == n, f"{second} after {first} rebuilt fields of an unchanged state"
        calls[first]()
        env.cost_to_go()
        assert env.cost_to_go_builds == n
        env.close()


def test_first_call_inside_a_capture_is_refused_and_a_later_capture_replays():
    torch = lazy_torch()
    from pogema_amd._lib import PgxError
    B, A, K = 16, 10, 4
    env = _head_on_env(batch=B, size=12, agents=A, seed=4, on_target="restart", max_episode_steps=24)
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
            env.pibt_plan(K, priority=prio, out=out, swap=True)
    assert ei.value.code == -4 and "capture" in str(ei.value) and "pgx_pibt_swap_plan" in str(ei.value)
    torch.cuda.synchronize()
    env.pibt_plan(K, priority=prio, out=out, swap=True)      # the eager call that allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.pibt_plan(K, priority=prio, out=out, swap=True)
    rng = np.random.default_rng(4)
    for t in range(3):
        env.step(out[0][0].clone() if t % 2 else mixed_actions(env, rng, p_expert=0.8))   # the state changes
        prio.copy_(torch.as_tensor(rng.integers(-2, 3, size=(B, A)), dtype=torch.int32))
        g.replay()
        got = [o.clone() for o in out]
        want, _ = _check(env, K, "restart", prio, what=f"replay {t}")
        assert all(torch.equal(x, y) for x, y in zip(got, want)), f"replay {t}"
    env.close()


def test_out_tensors_refused_arguments_and_list_view():
    torch = lazy_torch()
    from pogema_amd import GridConfig, PibtPolicy, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    B, A, K = 6, 9, 3
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.3, seed=21, collision_system="soft"), batch=B)
    with pytest.raises(PgxError) as ei:
        env.pibt_plan(K, swap=True)
    assert ei.value.code == -4 and "pgx_pibt_swap_plan" in str(ei.value)   # PGX_E_STATE before a reset
    obstacles, pos, tgt, _ = head_on_instances(B, 10, A, seed=21)
    env.reset_from_state(obstacles, pos, tgt)
    want = env.pibt_plan(K, swap=True)
    assert not torch.equal(want[0], env.pibt_plan(K)[0])
    dev = env.device
    for dtype in (torch.int8, torch.int32, torch.int64):
        out = [torch.full((K, B, A), 99, dtype=dtype, device=dev), torch.full((K, B, A, 2), 99, dtype=torch.int32, device=dev),
               torch.full((B, A), 99, dtype=torch.int32, device=dev), torch.full((B, A), 99, dtype=torch.int32, device=dev)]
        got = env.pibt_plan(K, out=tuple(out), swap=True)
        assert all(g is o for g, o in zip(got, out))
        assert torch.equal(out[0].to(torch.int64), want[0]) and all(torch.equal(o, w) for o, w in zip(out[1:], want[1:]))
    make = lambda: [torch.full((K, B, A), 99, dtype=torch.int32, device=dev), torch.full((K, B, A, 2), 99, dtype=torch.int32, device=dev),
                    torch.full((B, A), 99, dtype=torch.int32, device=dev), torch.full((B, A), 99, dtype=torch.int32, device=dev)]
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
                env.pibt_plan(K, out=tuple(o), swap=True)
    with pytest.raises(ValueError, match="out must be"):
        env.pibt_plan(K, out=tuple(make()[:3]), swap=True)
    for horizon in (0, 257, -3, 2.5, "3", None):
        with pytest.raises(ValueError, match="horizon"):
            env.pibt_plan(horizon, swap=True)
    with pytest.raises(TypeError, match="swap"):
        env.pibt_plan(K, swap="yes")
    with pytest.raises(TypeError):
        env.pibt_plan(K, None, True, torch.int64, None, True)        # keyword-only
    # through the C-ABI with a handle: PGX_E_INVALID, nothing is launched; the three optional outputs may be NULL
    out = make()
    call = env._lib.pgx_pibt_swap_plan
    assert call(env._handle, 0, 0, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 0, 257, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 4, K, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 2, K, None, out[0].data_ptr(), 1, None, None, None, env._stream()) == -1
    assert call(env._handle, 0, K, None, None, 1, None, None, None, env._stream()) == -1
    guard = torch.full((K * B * A + 64,), 77, dtype=torch.int32, device=dev)
    assert call(env._handle, 0, K, None, guard[32:].data_ptr(), 1, None, None, None, env._stream()) == 0
    assert torch.equal(guard[32:32 + K * B * A].view(K, B, A).to(torch.int64), want[0])
    assert bool((guard[:32] == 77).all()) and bool((guard[32 + K * B * A:] == 77).all())

    # PibtPolicy.plan(swap=True): the priorities go in and the final ones are kept, whatever the policy was built with
    for built_with in (False, True):
        policy = PibtPolicy(env, swap=built_with)
        policy.priority += 3
        a, path, arrival = policy.plan(K, swap=True)
        ref = env.pibt_plan(K, priority=torch.full((B, A), 3, dtype=torch.int32, device=dev), swap=True)
        assert torch.equal(a, ref[0]) and torch.equal(path, ref[1]) and torch.equal(arrival, ref[2])
        assert torch.equal(policy.priority, ref[3])
    env.close()

    rows, agents, targets = DEAD_END
    one = pogema_v0(GridConfig(map="\n".join(rows), num_agents=2, obs_radius=2, seed=21, collision_system="soft"))
    one._vec.reset_from_state(grid(rows)[None], np.array([agents], dtype=np.int32), np.array([targets], dtype=np.int32))
    plan = one.pibt_plan(9, swap=True)
    assert isinstance(plan, list) and len(plan) == 9 and all(len(row) == 2 and all(isinstance(a, int) for a in row) for row in plan)
    assert plan == [[4, 0], [3, 3], [3, 3], [3, 3], [4, 1], [4, 2], [4, 3], [4, 3], [4, 0]]
    assert plan[0] == one.pibt_actions(swap=True) and one.pibt_plan(9) == one.pibt_plan(9, swap=False) != plan
    assert isinstance(one.pibt_plan(2, priority=[0, 1], swap=True), list)
    one.close()
