"""GPU: move outcomes (VecPogema.move_outcomes / pgx_move_outcomes, docs/SPEC.md S17) equal the CPU reference
(tests/move_outcomes_reference.py) applied to get_state() and the installed maps, bit for bit on all four outputs: every
lane layout under every collision system, non-square, large and pooled maps, after set_targets and load_state.  The
step itself agrees: after step(actions) the agents stand on the next_xy the query gave before it.  Every code occurs;
the planner's and the shield's actions get no failure code under `soft`; the very first call of an engine is captured in
a graph; the state, the cache counter and the bad-action counter are untouched."""
import ctypes as C

import numpy as np
import pytest

from move_outcomes_reference import FOLLOW, MOVED, NUM_OUTCOMES, OBSTACLE, OCCUPIED, STAY, move_outcomes_reference
from test_visible_agents_gpu import LAYOUTS
from util import installed_maps, lazy_torch, mixed_actions, random_actions

pytestmark = pytest.mark.gpu

SYSTEMS = [("priority", "lowest_index"), ("block_both", "lowest_index"), ("soft", "lowest_index"), ("soft", "all_stay")]


def _env(collision="soft", soft_vertex="lowest_index", batch=8, on_target="finish", **kw):
    from pogema_amd import GridConfig, Semantics, VecPogema
    args = dict(size=10, num_agents=12, obs_radius=3, density=0.2, seed=5, max_episode_steps=64)
    args.update(kw)
    if "map" in args:
        del args["size"], args["density"]
    env = VecPogema(GridConfig(collision_system=collision, on_target=on_target, **args), batch=batch, auto_reset=False,
                    semantics=Semantics(soft_vertex=soft_vertex))
    return env


def _actions(env, rng, seed):
    """random_actions with p_noop = 0.2 plus a few out-of-range values."""
    a = random_actions(1, env.batch, env.num_agents, seed, p_noop=0.2)[0]
    bad = rng.random(a.shape) < 0.05
    a[bad] = rng.choice([-1, 5, 7, 100, -128], size=int(bad.sum()))
    return lazy_torch().as_tensor(a, device=env.device)


def _check(env, actions, what="", got=None):
    """move_outcomes(actions) == the reference on get_state() + the installed maps.  Returns the four tensors."""
    torch = lazy_torch()
    got = got if got is not None else env.move_outcomes(actions)
    B, A = env.batch, env.num_agents
    for t, dtype, shape in zip(got, (torch.int32, torch.uint8, torch.int32, torch.int32),
                               ((B, A, 2), (B, A), (B, A), (B, NUM_OUTCOMES))):
        assert t.dtype == dtype and tuple(t.shape) == shape
    st = env.get_state()
    active = st["is_active"].cpu().numpy()
    ref = move_outcomes_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), active, actions.cpu().numpy(),
                                  env.grid_config.collision_system, env.semantics.soft_vertex)
    for name, g, w in zip(("next_xy", "outcome", "blocker", "counts"), got, ref):
        g = g.cpu().numpy()
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"
    assert np.array_equal(ref[3].sum(axis=1), active.sum(axis=1))
    return got


@pytest.mark.parametrize("collision,soft_vertex", SYSTEMS)
@pytest.mark.parametrize("agents,size,batch", LAYOUTS)
def test_every_lane_layout_matches_reference(agents, size, batch, collision, soft_vertex):
    rng = np.random.default_rng(agents)
    env = _env(collision, soft_vertex, batch=min(batch, 40), size=size, num_agents=agents, obs_radius=2 if agents == 1024 else 3,
               density=0.1, seed=agents)
    env.reset(seed=agents)
    _check(env, _actions(env, rng, 1), f"A={agents} {collision}/{soft_vertex} reset")
    for _ in range(4):
        env.step(mixed_actions(env, rng, p_expert=0.8))
    _check(env, _actions(env, rng, 2), f"A={agents} {collision}/{soft_vertex} after 4 steps")
    env.close()


@pytest.mark.parametrize("on_target", ["finish", "nothing", "restart"])
@pytest.mark.parametrize("collision,soft_vertex", SYSTEMS)
def test_the_step_agrees(collision, soft_vertex, on_target):
    """The check that does not go through the reference: hidden agents keep their stored cell, so all agents compare."""
    torch = lazy_torch()
    rng = np.random.default_rng(3)
    env = _env(collision, soft_vertex, batch=24, on_target=on_target, num_agents=20, size=8, seed=8)
    env.reset(seed=8)
    moved = stayed = 0
    for t in range(8):
        actions = _actions(env, rng, 10 + t)
        before = env.get_state()
        next_xy, outcome, _, _ = env.move_outcomes(actions)
        env.step(actions)
        after = env.get_state()["agents_xy"]
        assert torch.equal(after, next_xy), f"{collision}/{soft_vertex}/{on_target} step {t}"
        arrived = (after != before["agents_xy"]).any(-1)
        assert torch.equal(arrived, outcome == MOVED)
        moved += int(arrived.sum())
        stayed += int((outcome >= 2).sum())
    assert moved > 100 and stayed > 100
    env.close()


@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_every_code_occurs(collision):
    rng = np.random.default_rng(1)
    env = _env(collision, batch=64, num_agents=40, size=10, density=0.2, seed=2)
    env.reset(seed=2)
    seen, total = set(), np.zeros(NUM_OUTCOMES, dtype=np.int64)
    for t in range(8):
        actions = _actions(env, rng, 20 + t)
        _, outcome, _, counts = _check(env, actions, f"{collision} step {t}") if t in (0, 7) else env.move_outcomes(actions)
        seen |= set(np.unique(outcome.cpu().numpy()).tolist())
        total += counts.cpu().numpy().sum(axis=0)
        env.step(actions)
    assert seen == set(range(NUM_OUTCOMES)) - ({FOLLOW} if collision == "soft" else set()), (collision, total.tolist())
    env.close()


def test_planner_and_shield_actions_get_no_failure_code_under_soft():
    torch = lazy_torch()
    rng = np.random.default_rng(4)
    env = _env("soft", batch=16, num_agents=24, size=10, seed=17)
    env.reset(seed=17)
    for t in range(6):
        for actions, want in (env.pibt_actions()[:2],
                              env.shield_actions(torch.as_tensor(rng.standard_normal((16, 24, 5)).astype(np.float32),
                                                                 device=env.device))[:2]):
            next_xy, outcome, blocker, _ = _check(env, actions, f"step {t}")
            assert torch.equal(next_xy, want) and int(outcome.max()) <= MOVED and int(blocker.max()) == -1
        env.step(actions)
    env.close()


def test_planner_moves_reverted_under_priority_are_follow_or_occupied():
    env = _env("priority", batch=16, num_agents=30, size=8, density=0.1, seed=23)
    env.reset(seed=23)
    codes = set()
    for t in range(8):
        actions, _ = env.pibt_actions()
        _, outcome, _, _ = _check(env, actions, f"step {t}")
        codes |= set(np.unique(outcome.cpu().numpy()).tolist())
        env.step(actions)
    assert codes <= {STAY, MOVED, OCCUPIED, FOLLOW} and FOLLOW in codes, codes
    env.close()


@pytest.mark.parametrize("name,rows,cols", [("wide", 5, 40), ("tall", 37, 6)])
def test_non_square_maps(name, rows, cols):
    grid = "\n".join("".join("#" if (x * 7 + y * 3) % 11 == 0 else "." for y in range(cols)) for x in range(rows))
    rng = np.random.default_rng(rows)
    for collision, soft_vertex in SYSTEMS:
        env = _env(collision, soft_vertex, batch=11, map=grid)
        env.reset(seed=3)
        for t in range(3):
            actions = _actions(env, rng, t)
            _check(env, actions, f"{name} {collision} step {t}")
            env.step(actions)
        env.close()


@pytest.mark.parametrize("size,agents,batch", [(300, 12, 2), (1024, 5, 1)])
def test_large_maps(size, agents, batch):
    """Coordinates above 1000; the engine's large-map layout."""
    rng = np.random.default_rng(size)
    for collision in ("priority", "soft"):
        env = _env(collision, batch=batch, size=size, num_agents=agents, obs_radius=4, density=0.2)
        env.reset(seed=5)
        if size == 1024:      # a crowd in the far corner: a chain, a contest and the ring, at coordinates above 1000
            maps = installed_maps(env).copy()
            maps[:, 1016:, 1016:] = 0
            xy = np.array([[(1023, 1023), (1023, 1022), (1023, 1021), (1022, 1023), (1021, 1022)]], dtype=np.int32)
            env.reset_from_state(maps, xy, xy[:, ::-1].copy())
            codes = set()
            for acts in ([4, 4, 4, 2, 2], [1, 4, 0, 3, 2], [3, 3, 3, 3, 3]):
                a = lazy_torch().as_tensor([acts], device=env.device)
                codes |= set(_check(env, a, f"1024 corner {acts}")[1].cpu().numpy().ravel().tolist())
            assert OBSTACLE in codes and OCCUPIED in codes, codes     # the ring at 1024, and the agent behind it
        for t in range(3):
            actions = _actions(env, rng, t)
            _check(env, actions, f"{size} {collision} step {t}")
            env.step(actions)
        env.close()


def test_map_pool_set_targets_and_load_state():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(77)
    H = W = 14
    pool = (rng.random((5, H, W)) < 0.15).astype(np.uint8)
    env = VecPogema(GridConfig(size=H, num_agents=6, obs_radius=3, seed=2, collision_system="priority", max_episode_steps=32),
                    batch=10, map_pool=torch.as_tensor(pool), auto_reset=False)
    env.reset(seed=2)
    assert len(set(env.map_index.cpu().numpy().tolist())) > 1
    _check(env, _actions(env, rng, 1), "pool reset")
    saved = env.save_state()
    maps = installed_maps(env)
    targets = np.stack([np.argwhere(m == 0)[rng.permutation(int((m == 0).sum()))[:6]] for m in maps]).astype(np.int32)
    env.set_targets(targets)
    actions = _actions(env, rng, 2)
    first = [t.clone() for t in _check(env, actions, "after set_targets")]
    for t in range(3):
        env.step(_actions(env, rng, 3 + t))
    _check(env, actions, "after steps")
    env.load_state(saved)
    for g, w in zip(_check(env, actions, "after load_state"), first):
        assert torch.equal(g, w)             # the same cells as before the steps: targets do not matter
    env.close()


def test_outputs_action_types_and_refused_arguments():
    torch = lazy_torch()
    from pogema_amd import GridConfig, pogema_v0
    from pogema_amd._lib import OUTCOMES, PgxError
    rng = np.random.default_rng(21)
    env = _env("priority", batch=6, num_agents=9)
    B, A = 6, 9
    with pytest.raises(PgxError) as ei:
        env.move_outcomes(torch.zeros((B, A), dtype=torch.int64, device=env.device))
    assert ei.value.code == -4                           # PGX_E_STATE before a reset
    env.reset(seed=21)
    actions = _actions(env, rng, 1).clamp(-100, 100)
    want = _check(env, actions, "fresh outputs")
    out = (torch.full((B, A, 2), 99, dtype=torch.int32, device=env.device), torch.full((B, A), 99, dtype=torch.uint8, device=env.device),
           torch.full((B, A), 99, dtype=torch.int32, device=env.device), torch.full((B, NUM_OUTCOMES), 99, dtype=torch.int32, device=env.device))
    got = env.move_outcomes(actions, out=out)
    assert all(g is o for g, o in zip(got, out)) and all(torch.equal(g, w) for g, w in zip(got, want))
    for dtype in (torch.int8, torch.int32, torch.int64):
        assert all(torch.equal(g, w) for g, w in zip(env.move_outcomes(actions.to(dtype)), want)), dtype
    assert all(torch.equal(g, w) for g, w in zip(env.move_outcomes(actions.cpu().numpy()), want))
    bad_out = [("next_xy", (torch.empty((B, A, 3), dtype=torch.int32, device=env.device),) + out[1:]),
               ("outcome", (out[0], torch.empty((B, A), dtype=torch.int8, device=env.device)) + out[2:]),
               ("blocker", out[:2] + (torch.empty((B, A + 1), dtype=torch.int32, device=env.device), out[3])),
               ("counts", out[:3] + (torch.empty((B, NUM_OUTCOMES + 1), dtype=torch.int32, device=env.device),)),
               ("counts", out[:3] + (None,)), ("out", out[:3])]
    for name, o in bad_out:
        with pytest.raises(ValueError, match=name):
            env.move_outcomes(actions, out=o)
    with pytest.raises(ValueError, match="actions"):
        env.move_outcomes(actions[:, :4])
    # through the C-ABI: any subset of the outputs; PGX_E_INVALID launches nothing
    call, h, ap, st = env._lib.pgx_move_outcomes, env._handle, actions.data_ptr(), env._stream()
    guard = torch.full((B * NUM_OUTCOMES + 64,), 77, dtype=torch.int32, device=env.device)
    assert call(h, ap, 2, 0, None, None, None, guard[32:].data_ptr(), st) == 0
    assert torch.equal(guard[32:32 + B * NUM_OUTCOMES].view(B, NUM_OUTCOMES), want[3])
    assert bool((guard[:32] == 77).all()) and bool((guard[32 + B * NUM_OUTCOMES:] == 77).all())
    only = torch.full((B, A), 99, dtype=torch.uint8, device=env.device)
    assert call(h, ap, 2, 0, None, only.data_ptr(), None, None, st) == 0 and torch.equal(only, want[1])
    only = torch.full((B, A, 2), 99, dtype=torch.int32, device=env.device)
    assert call(h, ap, 2, 0, only.data_ptr(), None, out[2].fill_(99).data_ptr(), None, st) == 0
    assert torch.equal(only, want[0]) and torch.equal(out[2], want[2])
    assert call(h, ap, 2, 0, None, None, None, None, st) == -1
    assert call(h, None, 2, 0, None, out[1].data_ptr(), None, None, st) == -1
    assert call(h, ap, 2, 1, None, out[1].data_ptr(), None, None, st) == -1
    assert call(h, ap, 5, 0, None, out[1].data_ptr(), None, None, st) == -1
    assert call(h, ap + 4, 2, 0, None, out[1].data_ptr(), None, None, st) == -1
    assert call(h, ap, 2, 0, out[0].data_ptr() + 2, None, None, None, st) == -1
    assert call(C.c_void_p(), ap, 2, 0, None, out[1].data_ptr(), None, None, st) == -1
    env.close()

    one = pogema_v0(GridConfig(size=8, num_agents=10, obs_radius=3, density=0.0, seed=21, collision_system="block_both"))
    one.reset(seed=21)
    acts = [int(a) for a in rng.integers(0, 5, size=10)]
    view = one.move_outcomes(acts)
    assert len(view) == 10 and all(v["outcome"] in OUTCOMES and isinstance(v["next_xy"], tuple) for v in view)
    assert all((v["blocker"] is None) == (v["outcome"] in ("STAY", "MOVED", "OBSTACLE")) for v in view)
    one.step(acts)
    assert one.get_agents_xy() == [v["next_xy"] for v in view]
    one.close()


def test_first_call_ever_is_captured_in_a_graph():
    torch = lazy_torch()
    B, A = 16, 10
    rng = np.random.default_rng(4)
    env = _env("block_both", batch=B, num_agents=A, size=12, seed=4)
    env.reset(seed=4)
    actions = torch.zeros((B, A), dtype=torch.int64, device=env.device)
    out = (torch.zeros((B, A, 2), dtype=torch.int32, device=env.device), torch.zeros((B, A), dtype=torch.uint8, device=env.device),
           torch.zeros((B, A), dtype=torch.int32, device=env.device), torch.zeros((B, NUM_OUTCOMES), dtype=torch.int32, device=env.device))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.move_outcomes(actions, out=out)
    for t in range(4):
        env.step(_actions(env, rng, 40 + t))
        actions.copy_(_actions(env, rng, 50 + t))
        g.replay()
        replayed = tuple(o.clone() for o in out)
        _check(env, actions, f"replay {t}", got=replayed)
        for r, e in zip(replayed, env.move_outcomes(actions)):
            assert torch.equal(r, e)
    assert env.cost_to_go_builds == 0
    env.close()


@pytest.mark.parametrize("bad_action", ["noop", "flag"])
def test_state_and_counters_untouched(bad_action):
    torch = lazy_torch()
    from pogema_amd import GridConfig, Semantics, VecPogema
    gc = GridConfig(size=14, num_agents=12, obs_radius=3, density=0.2, seed=31, collision_system="soft", on_target="restart",
                    max_episode_steps=32)
    envs = [VecPogema(gc, batch=8, auto_reset=False, reuse_buffers=False, semantics=Semantics(bad_action=bad_action))
            for _ in range(2)]
    for e in envs:
        e.reset(seed=31)
    env, twin = envs
    env.cost_to_go()                                     # the cache exists, so that its counter can be watched
    builds = env.cost_to_go_builds
    rng = np.random.default_rng(31)
    for t in range(4):
        before = env.save_state()["engine"].clone()
        bad = _actions(env, rng, 60 + t)
        bad[0, 0] = 9                                    # an out-of-range action of an active agent
        env.move_outcomes(bad)
        assert torch.equal(env.save_state()["engine"], before), f"step {t}"
        assert env.cost_to_go_builds == builds
        assert int(env._lib.pgx_bad_action_count(env._handle, env._stream())) == 0
        good = torch.as_tensor(rng.integers(0, 5, size=(8, 12)), device=env.device)
        for a, b in zip(env.step(good)[:4], twin.step(good)[:4]):
            assert torch.equal(a, b)
        assert torch.equal(env.get_state()["agents_xy"], twin.get_state()["agents_xy"])
        builds = env.cost_to_go_builds
    for e in envs:
        e.close()
