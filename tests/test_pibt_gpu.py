"""GPU: the cooperative planner (VecPogema.pibt_actions / pgx_pibt_actions, docs/SPEC.md S13) equals the CPU reference
(tests/pibt_reference.py) applied to get_state() and the installed maps, bit for bit on actions and next_xy: every lane
layout, small and large cache layouts, every priority form and action dtype, after resets and steps of every collision
system and on_target mode, with a map pool and after set_targets.  Under `soft` every planned agent arrives on its
next cell; a head-on corridor the shortest-path expert never solves is solved.  The call shares cost_to_go()'s cache,
leaves the engine state alone and can be captured in a HIP graph after one eager call."""
import contextlib

import numpy as np
import pytest

from agent_counts import shared_fields
from pibt_reference import check_invariants, pibt_reference
from test_visible_agents_gpu import LAYOUTS
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu


def _check(env, priority=None, what="", dtype=None, invariants=False):
    """pibt_actions(priority) == the reference on get_state() + the installed maps; returns (actions, next_xy) tensors."""
    torch = lazy_torch()
    kw = {} if dtype is None else {"dtype": dtype}
    actions, next_xy = env.pibt_actions(priority=priority, **kw)
    assert actions.dtype == (torch.int64 if dtype is None else dtype) and tuple(actions.shape) == (env.batch, env.num_agents)
    assert next_xy.dtype == torch.int32 and tuple(next_xy.shape) == (env.batch, env.num_agents, 2)
    st = env.get_state()
    maps = installed_maps(env)
    pos, active, tgt = st["agents_xy"].cpu().numpy(), st["is_active"].cpu().numpy(), st["targets_xy"].cpu().numpy()
    # (hundreds of distinct targets per env: the reference's one search per target and call comes from a shared memo)
    with shared_fields(maps, tgt) if env.num_agents > 256 else contextlib.nullcontext():
        ref_a, ref_n = pibt_reference(maps, pos, tgt, active, None if priority is None else priority.cpu().numpy())
    for name, g, w in (("actions", actions.cpu().numpy().astype(np.int64), ref_a), ("next_xy", next_xy.cpu().numpy(), ref_n)):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: "
                               f"{g[tuple(bad[0])]} vs {w[tuple(bad[0])]}")
    if invariants:
        for b in range(env.batch):
            assert check_invariants(maps[b], pos[b], active[b], ref_n[b]) == [], (what, b)
    return actions, next_xy


def _priorities(env, rng):
    torch = lazy_torch()
    shape = (env.batch, env.num_agents)
    return (None, torch.as_tensor(rng.integers(-3, 4, size=shape), dtype=torch.int32, device=env.device),
            torch.full(shape, 7, dtype=torch.int32, device=env.device))


@pytest.mark.parametrize("agents,size,batch", LAYOUTS)
def test_every_lane_layout_matches_reference(agents, size, batch):
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(agents)
    batch = min(batch, 40)   # the reference is a Python recursion per env; the last workgroup stays partly filled
    for r in ((1, 5) if agents < 1024 else (2,)):
        gc = GridConfig(size=size, num_agents=agents, obs_radius=r, density=0.1, seed=agents + r,
                        collision_system="soft", on_target="finish", max_episode_steps=64)
        env = VecPogema(gc, batch=batch)
        env.reset(seed=agents + r)
        prios = _priorities(env, rng)
        for k, prio in enumerate(prios if agents < 1024 else prios[1:2]):
            _check(env, prio, what=f"A={agents} r={r} reset prio#{k}", invariants=True)
        for _ in range(4):
            env.step(mixed_actions(env, rng, p_expert=0.8))
        for k, prio in enumerate(prios[:2] if agents < 1024 else prios[:1]):
            _check(env, prio, what=f"A={agents} r={r} after 4 steps prio#{k}")
        env.close()


@pytest.mark.parametrize("name,rows,cols", [("wide", 5, 40), ("tall", 37, 6), ("odd", 13, 21), ("wide_large", 7, 90),
                                            ("tall_large", 70, 9)])
def test_non_square_maps(name, rows, cols):
    from pogema_amd import GridConfig, VecPogema
    grid = "\n".join("".join("#" if (x * 7 + y * 3) % 11 == 0 else "." for y in range(cols)) for x in range(rows))
    rng = np.random.default_rng(rows)
    env = VecPogema(GridConfig(map=grid, num_agents=12, obs_radius=3, seed=3, collision_system="soft",
                               max_episode_steps=64), batch=11)
    env.reset(seed=3)
    prios = _priorities(env, rng)
    for t in range(5):
        _check(env, prios[t % 3], what=f"{name} step {t}", invariants=t == 0)
        env.step(mixed_actions(env, rng, p_expert=0.8))
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
        env.step(env.pibt_actions()[0])
    _check(env, None, what=f"{size} after 3 steps")
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


def test_every_action_dtype():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=10, num_agents=14, obs_radius=3, density=0.2, seed=9, collision_system="soft"), batch=9)
    env.reset(seed=9)
    rng = np.random.default_rng(9)
    prio = _priorities(env, rng)[1]
    base, base_next = _check(env, prio, what="int64")
    for dtype in (torch.int8, torch.int32, torch.int64):
        a, n = _check(env, prio, what=str(dtype), dtype=dtype)
        assert torch.equal(a.to(torch.int64), base) and torch.equal(n, base_next)
        # any integer dtype of `priority` is converted
        a2, _ = env.pibt_actions(priority=prio.to(torch.int64), dtype=dtype)
        assert torch.equal(a2, a)
    env.close()


@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    """Finished (hidden) agents, lifelong retargets and auto-resets all occur between the checks."""
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=12, num_agents=10, obs_radius=3, density=0.25, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=40)
    env = VecPogema(gc, batch=12, auto_reset=True)
    env.reset(seed=7)
    rng = np.random.default_rng(11)
    prios = _priorities(env, rng)
    inactive_seen = retargeted = False
    last_targets = None
    for t in range(45):
        st = env.get_state()
        if last_targets is not None and int(st["elapsed"].min()) > 0:
            retargeted |= bool((st["targets_xy"] != last_targets)[st["elapsed"] > 0].any())
        last_targets = st["targets_xy"].clone()
        if t % 3 == 0:
            _check(env, prios[(t // 3) % 3], what=f"{collision}/{on_target} step {t}")
            inactive_seen |= bool((~st["is_active"]).any())
        # mostly the planner itself, some noise so that agents also stand on one cell under `soft`
        a = env.pibt_actions(priority=prios[1])[0] if t % 2 else mixed_actions(env, rng, p_expert=0.85)
        env.step(a)
    if on_target == "finish":
        assert inactive_seen, "no finished (hidden) agent was ever checked"
    if on_target == "restart":
        assert retargeted, "no lifelong retarget happened"
    env.close()


def test_map_pool_and_set_targets():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(77)
    H = W = 14
    pool = (rng.random((5, H, W)) < 0.15).astype(np.uint8)
    env = VecPogema(GridConfig(size=H, num_agents=6, obs_radius=3, seed=2, collision_system="soft", max_episode_steps=32),
                    batch=10, map_pool=torch.as_tensor(pool))
    env.reset(seed=2)
    assert len(set(env.map_index.cpu().numpy().tolist())) > 1
    prios = _priorities(env, rng)
    _check(env, prios[1], what="pool reset", invariants=True)
    for _ in range(3):
        env.step(env.pibt_actions()[0])
    _check(env, None, what="pool after steps")
    env.reset(seed=3)                      # other maps under the same cache
    _check(env, prios[1], what="pool second reset")
    # new targets: free cells of each env's own map (its first free cells, one per agent)
    maps = installed_maps(env)
    t = np.stack([np.argwhere(m == 0)[rng.permutation(int((m == 0).sum()))[:6]] for m in maps]).astype(np.int32)
    env.set_targets(t)
    assert np.array_equal(env.get_state()["targets_xy"].cpu().numpy(), t)
    _check(env, prios[1], what="after set_targets")
    env.close()


def test_soft_step_puts_every_planned_agent_on_its_next_cell():
    torch = lazy_torch()
    from pogema_amd import GridConfig, PibtPolicy, VecPogema
    gc = GridConfig(size=10, num_agents=24, obs_radius=3, density=0.2, seed=17, collision_system="soft",
                    on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=32, auto_reset=False)
    env.reset(seed=17)
    policy = PibtPolicy(env)
    assert policy.priority.dtype == torch.int32 and tuple(policy.priority.shape) == (32, 24)
    moved = 0
    for t in range(20):
        before = env.get_state()
        actions, next_xy = policy.act()
        want_prio = policy.priority.clone()
        out = env.step(actions)
        after = env.get_state()
        was = before["is_active"]
        assert was.any()
        assert torch.equal(after["agents_xy"][was], next_xy[was]), f"step {t}"
        moved += int((actions[was] != 0).sum())
        policy.update(out[1], out[4]["episode_done"])
        # the textbook rule, restated
        zero = ((out[1] > 0) | (after["agents_xy"] == after["targets_xy"]).all(-1) | ~after["is_active"]
                | out[4]["episode_done"].to(torch.bool).view(-1, 1))
        assert torch.equal(policy.priority, torch.where(zero, torch.zeros_like(want_prio), want_prio + 1))
    assert moved > 1000
    assert int(policy.priority.max()) > 0
    env.close()


def test_head_on_corridor_is_solved_where_the_expert_deadlocks():
    """A corridor of L = 9 cells (row 2) with one bay above its cell c = 6:

          #########            0 starts at the left end (2, 0) and wants the right end (2, 8),
          ######.##            1 starts at the right end (2, 8) and wants the left end (2, 0).
          .........

    The expert walks them towards each other until they stand side by side in the middle; from then on every step is
    the same swap, which `soft` reverts, for ever.

    PIBT with PibtPolicy's priorities, a bound by hand.  Both priorities start at 0 and grow by one per step until an
    agent stands on its target, so they stay equal and agent 0 (the lower index) plans first in every step until it
    has finished.  Agent 0 therefore moves right in EVERY step: the cell it wants is free, or agent 1 stands there, in
    which case 1 inherits the turn and has a cell to go to -- right along the corridor, or up into the bay once it
    stands below it (both are one step farther from its target; `up` is the lower action).  The agents meet around the
    middle, cell 4, left of the bay, so 1 reaches the bay before the corridor's end and never fails.  Agent 0 stands on
    its target after exactly L - 1 steps and is hidden (on_target = "finish").  At that moment agent 1 is somewhere in
    the corridor or in the bay, at most L steps from its target (the corridor's far end is L - 1 away, the bay
    c + 1 <= L - 1).  From then on it is alone and every step brings it one cell closer: at most L more steps.
    Bound: (L - 1) + L = 2 L - 1 = 17 steps.  (The reference takes 13 on this instance.)"""
    torch = lazy_torch()
    from pogema_amd import GridConfig, PibtPolicy, VecPogema
    L = 9
    grid = "#" * L + "\n" + "######.##" + "\n" + "." * L
    obst = np.array([[[c == "#" for c in row] for row in grid.split("\n")]], dtype=np.uint8)
    agents = np.array([[(2, 0), (2, L - 1)]], dtype=np.int32)
    targets = np.array([[(2, L - 1), (2, 0)]], dtype=np.int32)

    def run(policy_name):
        env = VecPogema(GridConfig(map=grid, num_agents=2, obs_radius=2, seed=1, collision_system="soft", on_target="finish",
                                   max_episode_steps=4 * L), batch=1, auto_reset=False)
        env.reset_from_state(obst, agents, targets)
        policy = PibtPolicy(env)
        for t in range(4 * L):
            if policy_name == "pibt":
                a, _ = policy.act()
            else:
                a, _ = env.expert_actions()
            out = env.step(a)
            policy.update(out[1], out[4]["episode_done"])
            if not bool(env.get_state()["is_active"].any()):
                env.close()
                return t + 1
        env.close()
        return None

    assert run("expert") is None, "the expert was expected to deadlock in the corridor"
    steps = run("pibt")
    print("corridor solved in", steps, "steps")
    assert steps is not None and steps <= 2 * L - 1


def test_cache_is_shared_with_cost_to_go():
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=16, num_agents=8, obs_radius=3, density=0.2, seed=5, collision_system="soft", max_episode_steps=64)
    for first in ("pibt", "cost_to_go"):
        env = VecPogema(gc, batch=20)
        env.reset(seed=5)
        assert env.cost_to_go_builds == 0
        calls = {"pibt": env.pibt_actions, "cost_to_go": env.cost_to_go}
        second = "cost_to_go" if first == "pibt" else "pibt"
        calls[first]()
        n = env.cost_to_go_builds
        assert n == 20 * 8, (first, n)                 # one field per active agent, whoever asked first
        calls[second]()
        assert env.cost_to_go_builds == n, f"{second} after {first} rebuilt fields of an unchanged state"
        calls[first]()
        assert env.cost_to_go_builds == n
        env.step(env.pibt_actions()[0])                  # targets did not move: still nothing to build
        calls[second]()
        assert env.cost_to_go_builds == n
        env.close()


def test_state_untouched():
    """save_state() blobs before and after the call are equal, and the next step() equals that of a twin env that never
    planned."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=14, num_agents=12, obs_radius=3, density=0.2, seed=31, collision_system="soft",
                    on_target="restart", max_episode_steps=32)
    a = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
    b = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
    a.reset(seed=31)
    b.reset(seed=31)
    rng = np.random.default_rng(31)
    for t in range(6):
        acts = torch.as_tensor(rng.integers(0, 5, size=(8, 12)), device=a.device)
        before = a.save_state()["engine"].clone()
        a.pibt_actions()
        a.pibt_actions(priority=torch.as_tensor(rng.integers(0, 9, size=(8, 12)), device=a.device))
        assert torch.equal(a.save_state()["engine"], before), f"step {t}"
        ra, rb = a.step(acts), b.step(acts)
        for x, y in zip(ra[:4], rb[:4]):
            assert torch.equal(x, y), f"step {t}"
        assert torch.equal(ra[4]["is_active"], rb[4]["is_active"])
    a.close()
    b.close()


def test_first_call_inside_a_capture_is_refused_and_a_later_capture_replays():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    B, A = 16, 10
    gc = GridConfig(size=12, num_agents=A, obs_radius=3, density=0.2, seed=4, collision_system="soft",
                    on_target="restart", max_episode_steps=24)
    env = VecPogema(gc, batch=B, auto_reset=True)
    env.reset(seed=4)
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
            env.pibt_actions(priority=prio, out=out)
    assert ei.value.code == -4 and "capture" in str(ei.value) and "pgx_pibt_actions" in str(ei.value)
    torch.cuda.synchronize()
    env.pibt_actions(priority=prio, out=out)           # the eager call that allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.pibt_actions(priority=prio, out=out)
    rng = np.random.default_rng(4)
    for t in range(12):
        env.step(out[0].clone() if t % 2 else mixed_actions(env, rng, p_expert=0.8))   # the state changes, targets are redrawn
        prio.copy_(torch.as_tensor(rng.integers(-2, 3, size=(B, A)), dtype=torch.int32))
        g.replay()
        got_a, got_n = out[0].clone(), out[1].clone()
        want_a, want_n = _check(env, prio, what=f"replay {t}")
        assert torch.equal(got_a, want_a) and torch.equal(got_n, want_n), f"replay {t}"
    env.close()


def test_out_tensors_refused_arguments_and_list_view():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    B, A = 6, 9
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.1, seed=21), batch=B)
    with pytest.raises(PgxError) as ei:
        env.pibt_actions()
    assert ei.value.code == -4                           # PGX_E_STATE before a reset
    env.reset(seed=21)
    actions, next_xy = env.pibt_actions()
    oa = torch.full((B, A), 99, dtype=torch.int32, device=env.device)
    on = torch.full((B, A, 2), 99, dtype=torch.int32, device=env.device)
    ra, rn = env.pibt_actions(out=(oa, on))
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
            env.pibt_actions(out=out)
    with pytest.raises(ValueError, match="dtype"):
        env.pibt_actions(dtype=torch.float32)
    with pytest.raises(ValueError, match="priority"):
        env.pibt_actions(priority=torch.zeros((B, A + 1), dtype=torch.int32, device=env.device))
    with pytest.raises(ValueError, match="priority"):
        env.pibt_actions(priority=torch.zeros((B, A), dtype=torch.int32))
    with pytest.raises(TypeError, match="priority"):
        env.pibt_actions(priority=torch.zeros((B, A), dtype=torch.float32, device=env.device))
    with pytest.raises(TypeError, match="priority"):
        env.pibt_actions(priority=[[0] * A] * B)
    # through the C-ABI with a handle: PGX_E_INVALID, nothing is launched; next_xy = NULL is allowed
    call = env._lib.pgx_pibt_actions
    assert call(env._handle, 0, None, None, 1, None, env._stream()) == -1
    assert call(env._handle, 2, None, oa.data_ptr(), 1, None, env._stream()) == -1
    assert call(env._handle, 0, None, oa.data_ptr(), 5, None, env._stream()) == -1
    guard = torch.full((B * A + 64,), 77, dtype=torch.int32, device=env.device)
    assert call(env._handle, 0, None, guard[32:].data_ptr(), 1, None, env._stream()) == 0
    assert torch.equal(guard[32:32 + B * A].view(B, A).to(torch.int64), actions)
    assert bool((guard[:32] == 77).all()) and bool((guard[32 + B * A:] == 77).all())
    env.close()

    one = pogema_v0(GridConfig(size=8, num_agents=10, obs_radius=3, density=0.0, seed=21, collision_system="soft"))
    one.reset(seed=21)
    acts = one.pibt_actions()
    assert isinstance(acts, list) and len(acts) == 10 and all(isinstance(a, int) for a in acts)
    assert acts == [int(a) for a in one._vec.pibt_actions()[0][0].cpu().numpy()]
    assert isinstance(one.pibt_actions(priority=list(range(10))), list)
    one.step(one.pibt_actions())
    one.close()
