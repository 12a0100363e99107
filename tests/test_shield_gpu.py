"""GPU: collision shielding (VecPogema.shield_actions / pgx_shield_actions, docs/SPEC.md S15) equals the CPU reference
(tests/shield_reference.py) applied to get_state() and the installed maps, bit for bit on actions, next_xy and
overridden: every lane layout, both tie-break modes, every priority form, score type and special value, after resets and
steps of every collision system and on_target mode, in a crowd whose pushes fail, with a map pool and after
set_targets.  Under `soft` every planned agent arrives on its next cell whatever the scores.  The default mode allocates
nothing and is captured in a HIP graph as the first call ever made; tie_break="distance" shares cost_to_go()'s cache."""
import contextlib

import numpy as np
import pytest

from agent_counts import shared_fields
from pibt_reference import check_invariants
from shield_inputs import crowd_scores, crowd_state, random_scores, special_scores
from shield_reference import shield_reference
from test_pibt_gpu import _priorities
from test_visible_agents_gpu import LAYOUTS
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

MODES = (None, "distance")


def _check(env, scores, priority=None, tie_break=None, what="", invariants=False, got=None):
    """shield_actions(scores, priority, tie_break) == the reference on get_state() + the installed maps; `got`: the
    tensors to check instead of a fresh call.  Returns (actions, next_xy, overridden)."""
    torch = lazy_torch()
    actions, next_xy, overridden = got if got is not None else env.shield_actions(scores, priority=priority, tie_break=tie_break)
    B, A = env.batch, env.num_agents
    assert actions.dtype == torch.int64 and tuple(actions.shape) == (B, A)
    assert next_xy.dtype == torch.int32 and tuple(next_xy.shape) == (B, A, 2)
    assert overridden.dtype == torch.uint8 and tuple(overridden.shape) == (B, A)
    st = env.get_state()
    maps = installed_maps(env)
    pos, active, tgt = st["agents_xy"].cpu().numpy(), st["is_active"].cpu().numpy(), st["targets_xy"].cpu().numpy()
    # (above 256 agents the reference's one search per distinct target and call comes from a shared memo)
    with shared_fields(maps, tgt) if A > 256 and tie_break is not None else contextlib.nullcontext():
        ref = shield_reference(maps, pos, tgt, active, scores.float().cpu().numpy(),
                               None if priority is None else priority.cpu().numpy(), tie_break)
    for name, g, w in (("actions", actions.cpu().numpy(), ref[0]), ("next_xy", next_xy.cpu().numpy(), ref[1]),
                       ("overridden", overridden.cpu().numpy(), ref[2])):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what} tie_break={tie_break}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: "
                               f"{g[tuple(bad[0])]} vs {w[tuple(bad[0])]}")
    if invariants:
        for b in range(B):
            assert check_invariants(maps[b], pos[b], active[b], ref[1][b]) == [], (what, b)
    return actions, next_xy, overridden


def _scores(env, rng, make=random_scores):
    return lazy_torch().as_tensor(make(rng, env.batch, env.num_agents), device=env.device)


@pytest.mark.parametrize("agents,size,batch", LAYOUTS)
def test_every_lane_layout_matches_reference(agents, size, batch):
    """Both tie-break modes and the three priority forms, after a reset and after 4 mixed steps.  At A = 1024 one
    priority form per state (random after the reset, none after the steps): every check there is a Python recursion over
    2048 agents, and the forms differ in the serving order only, which the smaller layouts cover in full."""
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(agents)
    batch = min(batch, 40)   # the reference is a Python recursion per env; the last workgroup stays partly filled
    seen = []
    for r in ((1, 5) if agents < 1024 else (2,)):
        gc = GridConfig(size=size, num_agents=agents, obs_radius=r, density=0.1, seed=agents + r,
                        collision_system="soft", on_target="finish", max_episode_steps=64)
        env = VecPogema(gc, batch=batch)
        env.reset(seed=agents + r)
        if agents >= 200:    # the reference runs one BFS per distinct target of an env: eight targets, not hundreds
            env.set_targets(env.get_state()["targets_xy"].cpu().numpy()[:, np.arange(agents) % 8])
        prios = _priorities(env, rng)
        for k, prio in enumerate(prios if agents < 1024 else prios[1:2]):
            for mode in MODES:
                out = _check(env, _scores(env, rng), prio, mode, what=f"A={agents} r={r} reset prio#{k}", invariants=True)
                seen.append(out[2].float().mean().item())
        for _ in range(4):
            env.step(mixed_actions(env, rng, p_expert=0.8))
        for k, prio in enumerate(prios if agents < 1024 else prios[:1]):
            for mode in MODES:
                _check(env, _scores(env, rng), prio, mode, what=f"A={agents} r={r} after 4 steps prio#{k}")
        env.close()
    assert 0.0 < np.mean(seen) < 1.0, seen     # the policy's choice was sometimes kept and sometimes not


@pytest.mark.parametrize("name,rows,cols", [("wide", 5, 40), ("tall", 37, 6)])
def test_non_square_maps(name, rows, cols):
    from pogema_amd import GridConfig, VecPogema
    grid = "\n".join("".join("#" if (x * 7 + y * 3) % 11 == 0 else "." for y in range(cols)) for x in range(rows))
    rng = np.random.default_rng(rows)
    env = VecPogema(GridConfig(map=grid, num_agents=12, obs_radius=3, seed=3, collision_system="soft",
                               max_episode_steps=64), batch=11)
    env.reset(seed=3)
    prios = _priorities(env, rng)
    for t in range(4):
        for mode in MODES:
            a = _check(env, _scores(env, rng), prios[t % 3], mode, what=f"{name} step {t}", invariants=t == 0)[0]
        env.step(a)
    env.close()


@pytest.mark.parametrize("size,agents,batch", [(300, 12, 2), (1024, 3, 1)])
def test_large_maps(size, agents, batch):
    """Coordinates above 1000; above 65536 cells the 32-bit fields of the cache under tie_break="distance".  The agents
    share a few targets: the reference runs one BFS over the whole map per target and env."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(size)
    env = VecPogema(GridConfig(size=size, num_agents=agents, obs_radius=4, density=0.2, seed=5, collision_system="soft",
                               max_episode_steps=64), batch=batch)
    env.reset(seed=5)
    shared = 2 if size == 300 else 1
    env.set_targets(env.get_state()["targets_xy"].cpu().numpy()[:, np.arange(agents) % shared])
    prios = _priorities(env, rng)
    _check(env, _scores(env, rng), prios[1], None, what=f"{size} reset", invariants=True)
    flat = torch.zeros((batch, agents, 5), device=env.device)
    _check(env, flat, prios[1], "distance", what=f"{size} reset, equal scores", invariants=True)   # the fields decide
    for _ in range(2):
        env.step(env.shield_actions(flat, tie_break="distance")[0])
    _check(env, _scores(env, rng, special_scores), None, None, what=f"{size} after 2 steps")
    if size == 300:
        _check(env, _scores(env, rng, special_scores), None, "distance", what=f"{size} after 2 steps")
    env.close()


def test_crowd_pushing_into_a_wall():
    """tests/shield_inputs.py's crowd: everyone scores `left` highest; PIBT calls fail in every env (test_shield.py)."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(200)
    obst, agents, targets = crowd_state()
    env = VecPogema(GridConfig(size=200, num_agents=30, obs_radius=4, density=0.0, seed=5, collision_system="soft",
                               max_episode_steps=64), batch=2)
    env.reset_from_state(obst, agents, targets)
    scores = torch.as_tensor(crowd_scores(), device=env.device)
    prios = _priorities(env, rng)
    moved = 0
    for t in range(6):
        a, _, o = _check(env, scores, prios[t % 3], MODES[t % 2], what=f"crowd step {t}", invariants=True)
        assert bool(o.any()) and not bool(o.all())
        moved += int((a != 0).sum())
        env.step(a)
    assert moved > 50
    env.close()


def test_score_equivalences():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A = 9, 14
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.2, seed=9, collision_system="soft"), batch=B)
    env.reset(seed=9)
    rng = np.random.default_rng(9)
    prios = _priorities(env, rng)
    for step in range(3):
        # constant scores + the distance tie-break = the planner, whatever the constant and its type
        for prio in prios:
            want = env.pibt_actions(priority=prio)
            for value, dtype in ((0.0, torch.float32), (-3.25, torch.float16), (float("inf"), torch.bfloat16),
                                 (float("nan"), torch.float32)):
                flat = torch.full((B, A, 5), value, dtype=dtype, device=env.device)
                a, n, o = env.shield_actions(flat, priority=prio, tie_break="distance")
                assert torch.equal(a, want[0]) and torch.equal(n, want[1]), (step, value)
                assert torch.equal(o.bool(), (want[0] != 0) & env.get_state()["is_active"])
        # narrow types: the same result as the same values widened to float32 (rounding to them makes ties)
        base = _scores(env, rng)
        base[0, :, :] = torch.as_tensor([6e-8, -6e-8, 1e-7, 0.0, -0.0], device=env.device)     # float16 subnormals
        for dtype in (torch.float16, torch.bfloat16):
            narrow = base.to(dtype)
            for mode in MODES:
                got = env.shield_actions(narrow, priority=prios[1], tie_break=mode)
                want = env.shield_actions(narrow.to(torch.float32), priority=prios[1], tie_break=mode)
                for g, w in zip(got, want):
                    assert torch.equal(g, w), (step, dtype, mode)
                _check(env, narrow, prios[1], mode, what=f"{dtype} step {step}", got=got)
        # a non-contiguous view gives what its contiguous copy gives
        wide = _scores(env, rng).repeat(1, 1, 2)
        view = wide[:, :, ::2]
        assert not view.is_contiguous()
        for g, w in zip(env.shield_actions(view), env.shield_actions(view.contiguous())):
            assert torch.equal(g, w)
        tr = torch.as_tensor(random_scores(rng, A, B), device=env.device).transpose(0, 1)
        assert not tr.is_contiguous()
        _check(env, tr, None, None, what="transposed view")
        env.step(mixed_actions(env, rng, p_expert=0.7))
    env.close()


def test_special_values():
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(1234)
    env = VecPogema(GridConfig(size=9, num_agents=20, obs_radius=2, density=0.15, seed=12, collision_system="soft",
                               max_episode_steps=64), batch=13)
    env.reset(seed=12)
    prios = _priorities(env, rng)
    for t in range(4):
        for mode in MODES:
            a = _check(env, _scores(env, rng, special_scores), prios[t % 3], mode, what=f"special step {t}", invariants=True)[0]
        env.step(a)
    env.close()


def test_soft_step_puts_every_planned_agent_on_its_next_cell():
    torch = lazy_torch()
    from pogema_amd import GridConfig, PibtPolicy, VecPogema
    gc = GridConfig(size=10, num_agents=24, obs_radius=3, density=0.2, seed=17, collision_system="soft",
                    on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=32, auto_reset=False)
    twin = VecPogema(gc, batch=32, auto_reset=False)
    env.reset(seed=17)
    twin.reset(seed=17)
    policy = PibtPolicy(env)
    rng = np.random.default_rng(17)
    strayed = overridden = 0
    for t in range(20):
        scores = _scores(env, rng)
        before = env.get_state()
        actions, next_xy, o = policy.act(scores=scores, tie_break=MODES[t % 2])
        out = env.step(actions)
        was = before["is_active"]
        assert was.any()
        assert torch.equal(env.get_state()["agents_xy"][was], next_xy[was]), f"step {t}"
        overridden += int(o.sum())
        policy.update(out[1], out[4]["episode_done"])
        # the same scores unshielded: every agent takes its argmax, and some do not arrive where it leads
        tb = twin.get_state()
        raw = scores.argmax(dim=-1)
        moves = torch.as_tensor([[0, 0], [-1, 0], [1, 0], [0, -1], [0, 1]], dtype=torch.int32, device=env.device)
        intended = tb["agents_xy"] + moves[raw]
        twin.step(raw)
        strayed += int((twin.get_state()["agents_xy"][tb["is_active"]] != intended[tb["is_active"]]).any(-1).sum())
    assert strayed > 0, "unshielded argmax actions never collided: the input shows nothing"
    assert overridden > 0 and int(policy.priority.max()) > 0
    # without scores the policy is the planner, as before
    a, n = policy.act()
    want = env.pibt_actions(priority=policy.priority)
    assert torch.equal(a, want[0]) and torch.equal(n, want[1])
    env.close()
    twin.close()


@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    """Finished (hidden) agents, lifelong retargets and auto-resets all occur between the checks."""
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=12, num_agents=10, obs_radius=3, density=0.25, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=20)
    env = VecPogema(gc, batch=12, auto_reset=True)
    env.reset(seed=7)
    rng = np.random.default_rng(11)
    prios = _priorities(env, rng)
    inactive_seen = False
    for t in range(24):
        if t % 3 == 0:
            _check(env, _scores(env, rng), prios[(t // 3) % 3], MODES[(t // 3) % 2], what=f"{collision}/{on_target} step {t}")
            inactive_seen |= bool((~env.get_state()["is_active"]).any())
        # mostly towards the targets, some noise so that agents also stand on one cell under `soft`
        env.step(mixed_actions(env, rng, p_expert=0.85))
    if on_target == "finish":
        assert inactive_seen, "no finished (hidden) agent was ever checked"
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
    for mode in MODES:
        _check(env, _scores(env, rng), prios[1], mode, what="pool reset", invariants=True)
    env.reset(seed=3)                      # other maps under the same cache
    for mode in MODES:
        _check(env, _scores(env, rng), prios[1], mode, what="pool second reset")
    maps = installed_maps(env)
    t = np.stack([np.argwhere(m == 0)[rng.permutation(int((m == 0).sum()))[:6]] for m in maps]).astype(np.int32)
    env.set_targets(t)
    flat = torch.zeros((10, 6, 5), device=env.device)
    _check(env, flat, prios[1], "distance", what="after set_targets")      # equal scores: the new targets decide
    env.close()


def test_state_untouched():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=14, num_agents=12, obs_radius=3, density=0.2, seed=31, collision_system="soft",
                    on_target="restart", max_episode_steps=32)
    env = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
    env.reset(seed=31)
    rng = np.random.default_rng(31)
    for t in range(4):
        before = env.save_state()["engine"].clone()
        for mode in MODES:
            env.shield_actions(_scores(env, rng), tie_break=mode)
            env.shield_actions(_scores(env, rng), priority=torch.as_tensor(rng.integers(0, 9, size=(8, 12)), device=env.device),
                               tie_break=mode)
            assert torch.equal(env.save_state()["engine"], before), f"step {t} {mode}"
        env.step(torch.as_tensor(rng.integers(0, 5, size=(8, 12)), device=env.device))
    env.close()


def _capture_setup():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A = 16, 10
    gc = GridConfig(size=12, num_agents=A, obs_radius=3, density=0.2, seed=4, collision_system="soft",
                    on_target="restart", max_episode_steps=24)
    env = VecPogema(gc, batch=B, auto_reset=True)
    env.reset(seed=4)
    prio = torch.zeros((B, A), dtype=torch.int32, device=env.device)
    scores = torch.zeros((B, A, 5), dtype=torch.float32, device=env.device)
    out = (torch.zeros((B, A), dtype=torch.int64, device=env.device), torch.zeros((B, A, 2), dtype=torch.int32, device=env.device),
           torch.zeros((B, A), dtype=torch.uint8, device=env.device))
    side = torch.cuda.Stream()             # the warm-up step on a side stream, as torch asks before a capture
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step(torch.zeros((B, A), dtype=torch.int64, device=env.device))
    torch.cuda.current_stream().wait_stream(side)
    return env, prio, scores, out


def _replay_and_check(env, g, prio, scores, out, mode, steps):
    torch = lazy_torch()
    rng = np.random.default_rng(4)
    B, A = env.batch, env.num_agents
    for t in range(steps):
        env.step(out[0].clone() if t % 2 else mixed_actions(env, rng, p_expert=0.8))   # the state changes, targets are redrawn
        prio.copy_(torch.as_tensor(rng.integers(-2, 3, size=(B, A)), dtype=torch.int32))
        scores.copy_(torch.as_tensor(random_scores(rng, B, A)))
        g.replay()
        _check(env, scores, prio, mode, what=f"replay {t}", got=tuple(o.clone() for o in out))


def test_default_mode_is_captured_as_the_first_call_ever():
    torch = lazy_torch()
    env, prio, scores, out = _capture_setup()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.shield_actions(scores, priority=prio, out=out)
    _replay_and_check(env, g, prio, scores, out, None, 8)
    assert env.cost_to_go_builds == 0      # no cache was ever made
    env.close()


def test_distance_mode_first_call_inside_a_capture_is_refused_and_a_later_capture_replays():
    torch = lazy_torch()
    from pogema_amd._lib import PgxError
    env, prio, scores, out = _capture_setup()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError) as ei:
        with torch.cuda.graph(g):
            env.shield_actions(scores, priority=prio, tie_break="distance", out=out)
    assert ei.value.code == -4 and "capture" in str(ei.value) and "pgx_shield_actions" in str(ei.value)
    torch.cuda.synchronize()
    env.shield_actions(scores, priority=prio, tie_break="distance", out=out)      # the eager call that allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.shield_actions(scores, priority=prio, tie_break="distance", out=out)
    _replay_and_check(env, g, prio, scores, out, "distance", 8)
    assert env.cost_to_go_builds > 0
    env.close()


def test_out_tensors_refused_arguments_and_list_view():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    B, A = 6, 9
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.1, seed=21), batch=B)
    rng = np.random.default_rng(21)
    scores = _scores(env, rng)
    with pytest.raises(PgxError) as ei:
        env.shield_actions(scores)
    assert ei.value.code == -4                           # PGX_E_STATE before a reset
    env.reset(seed=21)
    actions, next_xy, overridden = _check(env, scores, what="fresh outputs")
    oa = torch.full((B, A), 99, dtype=torch.int32, device=env.device)
    on = torch.full((B, A, 2), 99, dtype=torch.int32, device=env.device)
    oo = torch.full((B, A), 99, dtype=torch.uint8, device=env.device)
    ra, rn, ro = env.shield_actions(scores, out=(oa, on, oo))
    assert ra is oa and rn is on and ro is oo
    assert torch.equal(oa.to(torch.int64), actions) and torch.equal(on, next_xy) and torch.equal(oo, overridden)
    assert env.shield_actions(scores, dtype=torch.int8)[0].dtype == torch.int8
    bad_out = [
        (torch.empty((B, A), dtype=torch.float32, device=env.device), on, oo),
        (oa, torch.empty((B, A, 2), dtype=torch.int64, device=env.device), oo),
        (oa, on, torch.empty((B, A), dtype=torch.int8, device=env.device)),
        (oa, on, torch.empty((B, A + 1), dtype=torch.uint8, device=env.device)),
        (torch.empty((B, 2 * A), dtype=torch.int32, device=env.device)[:, ::2], on, oo),
        (oa, on, torch.empty((B, A), dtype=torch.uint8)),
        (oa, on),
        (oa, on, None),
    ]
    for out in bad_out:
        with pytest.raises(ValueError, match="out"):
            env.shield_actions(scores, out=out)
    with pytest.raises(ValueError, match="dtype"):
        env.shield_actions(scores, dtype=torch.float32)
    with pytest.raises(ValueError, match="scores"):
        env.shield_actions(scores[:, :, :4])
    with pytest.raises(ValueError, match="scores"):
        env.shield_actions(scores.cpu())
    with pytest.raises(TypeError, match="scores"):
        env.shield_actions(scores.to(torch.float64))
    with pytest.raises(TypeError, match="scores"):
        env.shield_actions(scores.cpu().numpy())
    with pytest.raises(ValueError, match="tie_break"):
        env.shield_actions(scores, tie_break="nearest")
    with pytest.raises(ValueError, match="priority"):
        env.shield_actions(scores, priority=torch.zeros((B, A + 1), dtype=torch.int32, device=env.device))
    with pytest.raises(TypeError, match="priority"):
        env.shield_actions(scores, priority=torch.zeros((B, A), dtype=torch.float32, device=env.device))
    # through the C-ABI with a handle: PGX_E_INVALID, nothing is launched; next_xy = overridden = NULL is allowed
    call, h, sp, st = env._lib.pgx_shield_actions, env._handle, scores.data_ptr(), env._stream()
    assert call(h, 0, None, 0, None, oa.data_ptr(), 1, None, None, st) == -1
    assert call(h, 0, sp, 0, None, None, 1, None, None, st) == -1
    assert call(h, 2, sp, 0, None, oa.data_ptr(), 1, None, None, st) == -1
    assert call(h, 0, sp, 3, None, oa.data_ptr(), 1, None, None, st) == -1
    assert call(h, 0, sp, 0, None, oa.data_ptr(), 5, None, None, st) == -1
    assert call(h, 0, sp + 2, 0, None, oa.data_ptr(), 1, None, None, st) == -1
    guard = torch.full((B * A + 64,), 77, dtype=torch.int32, device=env.device)
    for flags in (0, 1):
        guard.fill_(77)
        assert call(h, flags, sp, 0, None, guard[32:].data_ptr(), 1, None, None, st) == 0
        assert torch.equal(guard[32:32 + B * A].view(B, A).to(torch.int64), env.shield_actions(scores, tie_break=MODES[flags])[0])
        assert bool((guard[:32] == 77).all()) and bool((guard[32 + B * A:] == 77).all())
    env.close()

    one = pogema_v0(GridConfig(size=8, num_agents=10, obs_radius=3, density=0.0, seed=21, collision_system="soft"))
    one.reset(seed=21)
    s = rng.standard_normal((10, 5))
    acts = one.shield_actions(s)
    assert isinstance(acts, list) and len(acts) == 10 and all(isinstance(a, int) for a in acts)
    want = one._vec.shield_actions(torch.as_tensor(s.astype(np.float32)[None], device=one._vec.device))[0][0]
    assert acts == [int(a) for a in want.cpu().numpy()]
    assert isinstance(one.shield_actions(s.tolist(), priority=list(range(10))), list)
    one.step(one.shield_actions(s))
    one.close()
