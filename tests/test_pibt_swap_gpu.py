"""GPU: the cooperative planner with the swap operation (VecPogema.pibt_actions(swap=True) / pgx_pibt_swap_actions,
docs/SPEC.md S23) equals the CPU reference (tests/pibt_swap_reference.py) applied to get_state() and the installed maps,
bit for bit on actions and next_xy: every lane layout on states full of head-on pairs, non-square and large maps, the
hand-built instances with the walk cap on either side, every priority form and action dtype, after resets and steps of
every collision system and on_target mode, with a map pool and after set_targets.  Under `soft` every planned agent,
pulled ones included, arrives on its next cell; the dead end plain PIBT livelocks in is solved.  The call shares
cost_to_go()'s cache with the plain planner, leaves the engine state alone, can be captured in a HIP graph after one
eager call, and leaves the plain planner as it was."""
import contextlib

import numpy as np
import pytest

from agent_counts import shared_fields
from pibt_reference import check_invariants, pibt_reference
from pibt_swap_cases import (CAP_LENGTHS, DEAD_END, LAYOUT_MIN, PINNED, grid, head_on_instances, layout_case,
                             layout_priorities, layout_radii, serpentine)
from pibt_swap_reference import COUNTERS, MAX_WALK, pibt_swap_reference
from test_visible_agents_gpu import LAYOUTS
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu


def _state(env):
    st = env.get_state()
    return (installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(), st["is_active"].cpu().numpy())


def _check(env, priority=None, what="", dtype=None, invariants=False, total=None):
    """pibt_actions(priority, swap=True) == the reference on get_state() + the installed maps; returns (actions,
    next_xy) tensors and adds the reference's counters to `total`."""
    torch = lazy_torch()
    kw = {} if dtype is None else {"dtype": dtype}
    actions, next_xy = env.pibt_actions(priority=priority, swap=True, **kw)
    assert actions.dtype == (torch.int64 if dtype is None else dtype) and tuple(actions.shape) == (env.batch, env.num_agents)
    assert next_xy.dtype == torch.int32 and tuple(next_xy.shape) == (env.batch, env.num_agents, 2)
    maps, pos, tgt, active = _state(env)
    # (hundreds of distinct targets per env: the reference's one search per target and call comes from a shared memo)
    with shared_fields(maps, tgt) if env.num_agents > 256 else contextlib.nullcontext():
        ref_a, ref_n, count = pibt_swap_reference(maps, pos, tgt, active, None if priority is None else priority.cpu().numpy())
    for name, g, w in (("actions", actions.cpu().numpy().astype(np.int64), ref_a), ("next_xy", next_xy.cpu().numpy(), ref_n)):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: "
                               f"{g[tuple(bad[0])]} vs {w[tuple(bad[0])]}")
    if invariants:
        for b in range(env.batch):
            assert check_invariants(maps[b], pos[b], active[b], ref_n[b]) == [], (what, b)
    if total is not None:
        for name in COUNTERS:
            total[name] = max(total.get(name, 0), int(count[name].max())) if name == "longest_walk" else \
                total.get(name, 0) + int(count[name].sum())
    return actions, next_xy


def _dev(env, a, dtype=None):
    torch = lazy_torch()
    return None if a is None else torch.as_tensor(a, dtype=dtype or torch.int32, device=env.device)


def _priorities(env, rng):
    torch = lazy_torch()
    shape = (env.batch, env.num_agents)
    return (None, _dev(env, rng.integers(-3, 4, size=shape)), torch.full(shape, 7, dtype=torch.int32, device=env.device))


@pytest.mark.parametrize("agents,size,batch", LAYOUTS)
def test_every_lane_layout_matches_reference(agents, size, batch):
    """States in which about half of the agents stand head on in pairs (pibt_swap_cases.head_on_instances, density 0.3):
    summed over the case the reference must have reversed at least one list (one agent has no partner: nothing to
    reverse), and at least LAYOUT_MIN[agents] of each kind -- bounds the reference meets on the installed states alone
    (tests/test_pibt_swap.py checks that without a device)."""
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(agents)
    total = {}
    for r in layout_radii(agents):
        obstacles, pos, tgt, prios = layout_case(agents, size, batch, r)
        gc = GridConfig(size=size, num_agents=agents, obs_radius=r, density=0.3, seed=agents + r,
                        collision_system="soft", on_target="finish", max_episode_steps=64)
        env = VecPogema(gc, batch=len(pos))
        env.reset_from_state(obstacles, pos, tgt)
        for k, prio in enumerate(layout_priorities(agents, prios)):
            _check(env, _dev(env, prio), what=f"A={agents} r={r} installed prio#{k}", invariants=True, total=total)
        for _ in range(4):
            env.step(mixed_actions(env, rng, p_expert=0.8))
        for k, prio in enumerate(prios[:2] if agents <= 256 else prios[:1]):
            _check(env, _dev(env, prio), what=f"A={agents} r={r} after 4 steps prio#{k}", total=total)
        env.close()
    print(agents, total)
    unpulled = total["reversed"] - total["pulled"]
    if agents > 1:
        assert total["reversed"] >= 1, total
    want = LAYOUT_MIN.get(agents, {})
    assert total["clear"] >= want.get("clear", 0) and total["pulled"] >= want.get("pulled", 0) \
        and unpulled >= want.get("unpulled", 0), (total, want)


@pytest.mark.parametrize("name,rows,cols", [("wide", 5, 40), ("tall", 37, 6), ("odd", 13, 21), ("wide_large", 7, 90),
                                            ("tall_large", 70, 9)])
def test_non_square_maps(name, rows, cols):
    from pogema_amd import GridConfig, VecPogema
    text = "\n".join("".join("#" if (x * 7 + y * 3) % 11 == 0 or (x % 2 and y % 5) else "." for y in range(cols))
                     for x in range(rows))
    rng = np.random.default_rng(rows)
    env = VecPogema(GridConfig(map=text, num_agents=12, obs_radius=3, seed=3, collision_system="soft",
                               max_episode_steps=64), batch=11)
    env.reset(seed=3)
    prios = _priorities(env, rng)
    for t in range(5):
        a, _ = _check(env, prios[t % 3], what=f"{name} step {t}", invariants=t == 0)
        env.step(a)
    env.close()


@pytest.mark.parametrize("size,agents,batch", [(80, 40, 3), (300, 12, 2), (1024, 3, 1)])
def test_large_maps(size, agents, batch):
    """Sides above 64: the cache's large layout; above 65536 cells its 32-bit fields; coordinates above 1000."""
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(size)
    env = VecPogema(GridConfig(size=size, num_agents=agents, obs_radius=4, density=0.2, seed=5, collision_system="soft",
                               max_episode_steps=64), batch=batch)
    env.reset(seed=5)
    prios = _priorities(env, rng)
    _check(env, prios[1], what=f"{size} reset", invariants=True)
    for _ in range(3):
        env.step(env.pibt_actions(swap=True)[0])
    _check(env, None, what=f"{size} after 3 steps")
    env.close()


def test_head_on_pairs_on_a_large_map_with_32_bit_fields():
    """300 x 300 at density 0.3 with 40 agents, most of them in head-on pairs: walks over 32-bit fields."""
    from pogema_amd import GridConfig, VecPogema
    obstacles, pos, tgt, _ = head_on_instances(2, 300, 40, seed=300)
    env = VecPogema(GridConfig(size=300, num_agents=40, obs_radius=4, density=0.3, seed=5, collision_system="soft",
                               max_episode_steps=64), batch=2)
    env.reset_from_state(obstacles, pos, tgt)
    total = {}
    a, _ = _check(env, None, what="300 head on", invariants=True, total=total)
    env.step(a)
    _check(env, _priorities(env, np.random.default_rng(3))[1], what="300 head on, step 1", total=total)
    assert total["reversed"] >= 1 and total["pulled"] >= 1, total
    env.close()


def test_crowded_agents_side_by_side_on_a_large_map():
    """Agents packed into the far corner of a 200 x 200 map: pushes, chains and failed branches at large coordinates."""
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(200)
    obst = np.zeros((2, 200, 200), dtype=np.uint8)
    obst[:, 190, 150:199] = 1
    cells = np.array([(199 - i // 6, 199 - i % 6) for i in range(30)], dtype=np.int32)
    agents = np.stack([cells, cells[::-1]])
    targets = np.stack([cells[rng.permutation(30)], np.array([(i // 6, i % 6) for i in range(30)], dtype=np.int32)])
    env = VecPogema(GridConfig(size=200, num_agents=30, obs_radius=4, density=0.0, seed=5, collision_system="soft",
                               max_episode_steps=64), batch=2)
    env.reset_from_state(obst, agents, targets)
    prios = _priorities(env, rng)
    for t in range(6):
        a, _ = _check(env, prios[t % 3], what=f"corner step {t}", invariants=True)
        env.step(a)
    env.close()


# ---- hand-built instances ------------------------------------------------------------------------------------------
def _install(obstacles, agents, targets, **kw):
    from pogema_amd import GridConfig, VecPogema
    obstacles = np.asarray(obstacles, dtype=np.uint8)
    text = "\n".join("".join("#" if v else "." for v in row) for row in obstacles)
    cfg = dict(map=text, num_agents=len(agents), obs_radius=2, seed=1, collision_system="soft", on_target="finish",
               max_episode_steps=64)
    cfg.update(kw)
    env = VecPogema(GridConfig(**cfg), batch=1, auto_reset=False)
    env.reset_from_state(obstacles[None], np.array([agents], dtype=np.int32), np.array([targets], dtype=np.int32))
    return env


@pytest.mark.parametrize("name,instance,priority,actions,cells,counted", PINNED, ids=[p[0] for p in PINNED])
def test_pinned_outputs(name, instance, priority, actions, cells, counted):
    rows, agents, targets = instance
    env = _install(grid(rows), agents, targets)
    total = {}
    a, n = _check(env, _dev(env, None if priority is None else [priority]), what=name, invariants=True, total=total)
    assert a[0].tolist() == actions and [tuple(v) for v in n[0].tolist()] == cells
    assert {k: v for k, v in total.items() if v and k != "longest_walk"} == counted
    env.close()


def test_dead_end_is_solved_where_plain_pibt_livelocks():
    from pogema_amd import PibtPolicy
    rows, agents, targets = DEAD_END

    def run(swap, limit):
        env = _install(grid(rows), agents, targets)
        policy = PibtPolicy(env, swap=swap)
        for t in range(limit):
            a, _ = policy.act()
            out = env.step(a)
            policy.update(out[1], out[4]["episode_done"])
            if not bool(env.get_state()["is_active"].any()):
                env.close()
                return t + 1
        env.close()
        return None

    assert run(False, 36) is None, "plain PIBT was expected to livelock in the dead end"
    steps = run(True, 36)
    print("dead end solved in", steps, "steps")
    assert steps is not None and steps <= 9


@pytest.mark.parametrize("name", list(CAP_LENGTHS))
def test_walk_cap(name):
    """The junction is met in walk step MAX_WALK - 1 (swapped) or MAX_WALK (the cap: no swap, plain PIBT's answer)."""
    obstacles, agents, targets = serpentine(CAP_LENGTHS[name])
    env = _install(obstacles, agents, targets)
    total = {}
    a, _ = _check(env, None, what=name, invariants=True, total=total)
    if name == "below the cap":
        assert total["reversed"] == 1 and total["pulled"] == 1 and total["longest_walk"] == MAX_WALK - 1
        assert a[0].tolist() != [0, 0]
    else:
        assert total["reversed"] == 0 and total["longest_walk"] == MAX_WALK and a[0].tolist() == [0, 0]
    env.close()


# ---- modes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    """Finished (hidden) agents, lifelong retargets and auto-resets occur between the checks (`soft` steps leave no two
    agents on one cell, whatever the actions: test_shared_cells installs such states)."""
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=12, num_agents=10, obs_radius=3, density=0.3, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=40)
    env = VecPogema(gc, batch=12, auto_reset=True)
    env.reset(seed=7)
    rng = np.random.default_rng(11)
    prios = _priorities(env, rng)
    inactive_seen = retargeted = False
    last_targets = None
    total = {}
    for t in range(45):
        st = env.get_state()
        if last_targets is not None and int(st["elapsed"].min()) > 0:
            retargeted |= bool((st["targets_xy"] != last_targets)[st["elapsed"] > 0].any())
        last_targets = st["targets_xy"].clone()
        if t % 3 == 0:
            _check(env, prios[(t // 3) % 3], what=f"{collision}/{on_target} step {t}", total=total)
            inactive_seen |= bool((~st["is_active"]).any())
        # mostly the planner itself, some noise
        a = env.pibt_actions(priority=prios[1], swap=True)[0] if t % 2 else mixed_actions(env, rng, p_expert=0.85)
        env.step(a)
    print(collision, on_target, total)
    if on_target == "finish":
        assert inactive_seen, "no finished (hidden) agent was ever checked"
    if on_target == "restart":
        assert retargeted, "no lifelong retarget happened"
    env.close()


def test_shared_cells():
    """Planned agents that stand on one cell (states S13 calls outside its guarantees): `now` of the cell is the lowest
    index, in the table the walks use as in the candidate lists, and the output is still exactly the pseudo-code's."""
    from pogema_amd import GridConfig, VecPogema
    obstacles, pos, tgt, _ = head_on_instances(8, 8, 6, seed=8)
    pos = pos.copy()
    pos[:, 5] = pos[:, 0]                    # agent 5 stands where agent 0 stands,
    pos[::2, 4] = pos[::2, 1]                # and in every other env agent 4 where agent 1 stands
    env = VecPogema(GridConfig(size=8, num_agents=6, obs_radius=2, density=0.3, seed=1, collision_system="soft",
                               on_target="nothing", max_episode_steps=64), batch=8)
    env.reset_from_state(obstacles, pos, tgt, validate=False)
    xy = env.get_state()["agents_xy"].cpu().numpy()
    assert np.array_equal(xy, pos), "the engine did not install the shared cells"
    rng = np.random.default_rng(8)
    total = {}
    for k, prio in enumerate(_priorities(env, rng)):
        _check(env, prio, what=f"shared prio#{k}", total=total)
    print("shared cells:", total)
    env.close()


def test_soft_step_puts_every_planned_agent_on_its_next_cell():
    """Pulled agents among them: the reference's pull count over the run is above zero."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, PibtPolicy, VecPogema
    obstacles, pos, tgt, _ = head_on_instances(32, 10, 24, seed=17)
    gc = GridConfig(size=10, num_agents=24, obs_radius=3, density=0.3, seed=17, collision_system="soft",
                    on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=32, auto_reset=False)
    env.reset_from_state(obstacles, pos, tgt)
    policy = PibtPolicy(env, swap=True)
    moved = pulled = 0
    for t in range(20):
        before = env.get_state()
        actions, next_xy = policy.act()
        if t % 4 == 0:
            maps, p, g, act = _state(env)
            ref_a, ref_n, count = pibt_swap_reference(maps, p, g, act, policy.priority.cpu().numpy())
            assert np.array_equal(ref_a, actions.cpu().numpy()) and np.array_equal(ref_n, next_xy.cpu().numpy()), f"step {t}"
            pulled += int(count["pulled"].sum())
        out = env.step(actions)
        after = env.get_state()
        was = before["is_active"]
        assert torch.equal(after["agents_xy"][was], next_xy[was]), f"step {t}"
        moved += int((actions[was] != 0).sum())
        policy.update(out[1], out[4]["episode_done"])
    assert moved > 500 and pulled > 0, (moved, pulled)
    env.close()


# ---- infrastructure ----------------------------------------------------------------------------------------------------
def _head_on_env(batch=9, size=10, agents=14, seed=9, **kw):
    from pogema_amd import GridConfig, VecPogema
    obstacles, pos, tgt, _ = head_on_instances(batch, size, agents, seed=seed)
    cfg = dict(size=size, num_agents=agents, obs_radius=3, density=0.3, seed=seed, collision_system="soft")
    cfg.update(kw)
    env = VecPogema(GridConfig(**cfg), batch=batch)
    env.reset_from_state(obstacles, pos, tgt)
    return env


def test_every_action_dtype():
    torch = lazy_torch()
    env = _head_on_env()
    prio = _priorities(env, np.random.default_rng(9))[1]
    base, base_next = _check(env, prio, what="int64")
    for dtype in (torch.int8, torch.int32, torch.int64):
        a, n = _check(env, prio, what=str(dtype), dtype=dtype)
        assert torch.equal(a.to(torch.int64), base) and torch.equal(n, base_next)
        a2, _ = env.pibt_actions(priority=prio.to(torch.int64), dtype=dtype, swap=True)
        assert torch.equal(a2, a)
    env.close()


def test_plain_planner_is_unchanged():
    """pibt_actions() and pibt_actions(swap=False) are identical to each other and to pibt_reference on a state on which
    the swap planner answers differently."""
    torch = lazy_torch()
    env = _head_on_env()
    prio = _priorities(env, np.random.default_rng(9))[1]
    maps, pos, tgt, active = _state(env)
    for p in (None, prio):
        a0, n0 = env.pibt_actions(priority=p)
        a1, n1 = env.pibt_actions(priority=p, swap=False)
        ref_a, ref_n = pibt_reference(maps, pos, tgt, active, None if p is None else p.cpu().numpy())
        assert torch.equal(a0, a1) and torch.equal(n0, n1)
        assert np.array_equal(a0.cpu().numpy(), ref_a) and np.array_equal(n0.cpu().numpy(), ref_n)
        assert not torch.equal(env.pibt_actions(priority=p, swap=True)[0], a0)
    env.close()


def test_map_pool_and_set_targets():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(77)
    H = W = 14
    pool = (rng.random((5, H, W)) < 0.3).astype(np.uint8)
    env = VecPogema(GridConfig(size=H, num_agents=6, obs_radius=3, seed=2, collision_system="soft", max_episode_steps=32),
                    batch=10, map_pool=torch.as_tensor(pool))
    env.reset(seed=2)
    assert len(set(env.map_index.cpu().numpy().tolist())) > 1
    prios = _priorities(env, rng)
    _check(env, prios[1], what="pool reset", invariants=True)
    for _ in range(3):
        env.step(env.pibt_actions(swap=True)[0])
    _check(env, None, what="pool after steps")
    env.reset(seed=3)                      # other maps under the same cache
    _check(env, prios[1], what="pool second reset")
    # new targets: a neighbour's cell where an agent has a free neighbour cell (head on with whoever stands there),
    # else a free cell of the env's own map
    maps = installed_maps(env)
    pos = env.get_state()["agents_xy"].cpu().numpy()
    t = np.stack([np.argwhere(m == 0)[rng.permutation(int((m == 0).sum()))[:6]] for m in maps]).astype(np.int32)
    for b in range(10):
        for i in range(0, 6, 2):
            t[b, i], t[b, i + 1] = pos[b, i + 1], pos[b, i]
    env.set_targets(t)
    assert np.array_equal(env.get_state()["targets_xy"].cpu().numpy(), t)
    _check(env, prios[1], what="after set_targets")
    env.close()


def test_cache_is_shared_with_the_plain_planner():
    env = None
    for first in ("swap", "plain"):
        env = _head_on_env(batch=20, size=16, agents=8, seed=5, max_episode_steps=64)
        assert env.cost_to_go_builds == 0
        calls = {"swap": lambda: env.pibt_actions(swap=True), "plain": env.pibt_actions}
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


def test_state_untouched():
    """save_state() blobs before and after the call are equal, and the next step() equals that of a twin env that never
    planned."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=14, num_agents=12, obs_radius=3, density=0.3, seed=31, collision_system="soft",
                    on_target="restart", max_episode_steps=32)
    a = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
    b = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
    a.reset(seed=31)
    b.reset(seed=31)
    rng = np.random.default_rng(31)
    for t in range(6):
        acts = torch.as_tensor(rng.integers(0, 5, size=(8, 12)), device=a.device)
        before = a.save_state()["engine"].clone()
        a.pibt_actions(swap=True)
        a.pibt_actions(priority=torch.as_tensor(rng.integers(0, 9, size=(8, 12)), device=a.device), swap=True)
        assert torch.equal(a.save_state()["engine"], before), f"step {t}"
        ra, rb = a.step(acts), b.step(acts)
        for x, y in zip(ra[:4], rb[:4]):
            assert torch.equal(x, y), f"step {t}"
        assert torch.equal(ra[4]["is_active"], rb[4]["is_active"])
    a.close()
    b.close()


def test_first_call_inside_a_capture_is_refused_and_a_later_capture_replays():
    torch = lazy_torch()
    from pogema_amd._lib import PgxError
    B, A = 16, 10
    env = _head_on_env(batch=B, size=12, agents=A, seed=4, on_target="restart", max_episode_steps=24)
    prio = torch.zeros((B, A), dtype=torch.int32, device=env.device)
    out = (torch.zeros((B, A), dtype=torch.int64, device=env.device), torch.zeros((B, A, 2), dtype=torch.int32, device=env.device))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step(torch.zeros((B, A), dtype=torch.int64, device=env.device))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError) as ei:
        with torch.cuda.graph(g):
            env.pibt_actions(priority=prio, out=out, swap=True)
    assert ei.value.code == -4 and "capture" in str(ei.value) and "pgx_pibt_swap_actions" in str(ei.value)
    torch.cuda.synchronize()
    env.pibt_actions(priority=prio, out=out, swap=True)           # the eager call that allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.pibt_actions(priority=prio, out=out, swap=True)
    rng = np.random.default_rng(4)
    total = {}
    for t in range(12):
        env.step(out[0].clone() if t % 2 else mixed_actions(env, rng, p_expert=0.8))   # the state changes, targets are redrawn
        prio.copy_(torch.as_tensor(rng.integers(-2, 3, size=(B, A)), dtype=torch.int32))
        g.replay()
        got_a, got_n = out[0].clone(), out[1].clone()
        want_a, want_n = _check(env, prio, what=f"replay {t}", total=total)
        assert torch.equal(got_a, want_a) and torch.equal(got_n, want_n), f"replay {t}"
    print("replays:", total)
    env.close()


def test_out_tensors_refused_arguments_and_list_view():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    B, A = 6, 9
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.3, seed=21), batch=B)
    with pytest.raises(PgxError) as ei:
        env.pibt_actions(swap=True)
    assert ei.value.code == -4 and "pgx_pibt_swap_actions" in str(ei.value)   # PGX_E_STATE before a reset
    obstacles, pos, tgt, _ = head_on_instances(B, 10, A, seed=21)
    env.reset_from_state(obstacles, pos, tgt)
    actions, next_xy = env.pibt_actions(swap=True)
    oa = torch.full((B, A), 99, dtype=torch.int32, device=env.device)
    on = torch.full((B, A, 2), 99, dtype=torch.int32, device=env.device)
    ra, rn = env.pibt_actions(out=(oa, on), swap=True)
    assert ra is oa and rn is on and torch.equal(oa.to(torch.int64), actions) and torch.equal(on, next_xy)
    bad_out = [
        (torch.empty((B, A), dtype=torch.float32, device=env.device), on),
        (oa, torch.empty((B, A, 2), dtype=torch.int64, device=env.device)),
        (torch.empty((B, A + 1), dtype=torch.int32, device=env.device), on),
        (oa, torch.empty((B, A), dtype=torch.int32, device=env.device)),
        (torch.empty((B, 2 * A), dtype=torch.int32, device=env.device)[:, ::2], on),
        (torch.empty((B, A), dtype=torch.int32), on),
        (oa,),
        (oa, None),
    ]
    for out in bad_out:
        with pytest.raises(ValueError, match="out"):
            env.pibt_actions(out=out, swap=True)
    with pytest.raises(ValueError, match="dtype"):
        env.pibt_actions(dtype=torch.float32, swap=True)
    with pytest.raises(ValueError, match="priority"):
        env.pibt_actions(priority=torch.zeros((B, A + 1), dtype=torch.int32, device=env.device), swap=True)
    with pytest.raises(ValueError, match="priority"):
        env.pibt_actions(priority=torch.zeros((B, A), dtype=torch.int32), swap=True)
    with pytest.raises(TypeError, match="priority"):
        env.pibt_actions(priority=torch.zeros((B, A), dtype=torch.float32, device=env.device), swap=True)
    with pytest.raises(TypeError, match="priority"):
        env.pibt_actions(priority=[[0] * A] * B, swap=True)
    with pytest.raises(TypeError, match="swap"):
        env.pibt_actions(swap="yes")
    with pytest.raises(TypeError):
        env.pibt_actions(None, torch.int64, None, True)       # keyword-only
    # through the C-ABI with a handle: PGX_E_INVALID, nothing is launched; next_xy = NULL is allowed
    call = env._lib.pgx_pibt_swap_actions
    assert call(env._handle, 0, None, None, 1, None, env._stream()) == -1
    assert call(env._handle, 2, None, oa.data_ptr(), 1, None, env._stream()) == -1
    assert call(env._handle, 0, None, oa.data_ptr(), 5, None, env._stream()) == -1
    guard = torch.full((B * A + 64,), 77, dtype=torch.int32, device=env.device)
    nguard = torch.full((2 * B * A + 64,), 77, dtype=torch.int32, device=env.device)
    assert call(env._handle, 0, None, guard[32:].data_ptr(), 1, None, env._stream()) == 0
    assert call(env._handle, 0, None, oa.data_ptr(), 1, nguard[32:].data_ptr(), env._stream()) == 0
    assert torch.equal(guard[32:32 + B * A].view(B, A).to(torch.int64), actions)
    assert bool((guard[:32] == 77).all()) and bool((guard[32 + B * A:] == 77).all())
    assert torch.equal(nguard[32:32 + 2 * B * A].view(B, A, 2), next_xy)
    assert bool((nguard[:32] == 77).all()) and bool((nguard[32 + 2 * B * A:] == 77).all())
    env.close()

    rows, agents, targets = PINNED[1][1]
    one = pogema_v0(GridConfig(map="\n".join(rows), num_agents=2, obs_radius=2, seed=21, collision_system="soft"))
    one._vec.reset_from_state(grid(rows)[None], np.array([agents], dtype=np.int32), np.array([targets], dtype=np.int32))
    acts = one.pibt_actions(swap=True)
    assert isinstance(acts, list) and all(isinstance(a, int) for a in acts) and acts == PINNED[1][3]
    assert one.pibt_actions() == one.pibt_actions(swap=False) == [0, 0]
    assert isinstance(one.pibt_actions(priority=[0, 1], swap=True), list)
    one.close()
