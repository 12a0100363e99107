"""GPU: agent counts 257..1023 (tests/agent_counts.py), bit for bit against the CPU references.  Step and rollout
launches against the C oracle at every count: 5..16 waves per env with full and ragged last waves, the other observation
formats, the forced large-map layout and the other soft rules at four of them.  Chains and rings of all agents, which need
the closure's 9th and 10th round, in the step, the rollout launch and move_outcomes().  The episode-end reduction with
one idling agent in the first, a middle and the last wave.  The planners on a packed crowd whose pushes fail.  The
slot-based queries (expert, cost-to-go, goal directions, policy input) after a reset and after steps that finish agents.
The neighbour lists' ragged last chunk writes nothing past its rows.  tests/test_agent_counts.py shows on the CPU that
these inputs reach what they are here for."""
import functools

import numpy as np
import pytest

import agent_counts as ac
from agent_counts import AGENT_COUNTS
from move_outcomes_reference import move_outcomes_reference
from pibt_reference import check_invariants
from shield_inputs import random_scores, special_scores
from test_parity_gpu import _corridor_case
from util import (assert_rollouts_equal, c_oracle_rollout, engine_rollout, engine_rollout_launch, installed_maps, lazy_torch)

pytestmark = pytest.mark.gpu

COLLISIONS = ("priority", "block_both", "soft")


# ---- step and rollout parity at every count --------------------------------------------------------------------------------
def _kw(A, collision=None, on_target=None):
    pair = ac.pairing_of(A)
    return dict(obs_radius=ac.CASES[A][3], collision_system=collision or pair[0], on_target=on_target or pair[1],
                max_episode_steps=5, auto_reset=True, seed=1234, env_index_base=17)


@functools.lru_cache(maxsize=2)
def _oracle(A):
    """The C oracle's rollout of a count under its own pairing, shared by the tests that compare with it."""
    obstacles, agents, targets, actions, _ = ac.count_instance(A)
    return c_oracle_rollout(obstacles, agents, targets, actions, nthreads=8, **_kw(A))


def _both_launch_shapes(A, ref, what, kw=None, **extra):
    obstacles, agents, targets, actions, _ = ac.count_instance(A)
    kw = kw or _kw(A)
    assert_rollouts_equal(ref, engine_rollout(obstacles, agents, targets, actions, **kw, **extra), f"{what}: one launch per step")
    assert_rollouts_equal(ref, engine_rollout_launch(obstacles, agents, targets, actions, **kw, **extra), f"{what}: one rollout launch")


@pytest.mark.parametrize("A", AGENT_COUNTS)
def test_step_and_rollout_parity(A):
    _both_launch_shapes(A, _oracle(A), f"A={A} {ac.pairing_of(A)}")


@pytest.mark.parametrize("fmt", ["uint8", "bfloat16"])
@pytest.mark.parametrize("A", ac.EXTRA_COUNTS)
def test_other_observation_formats(A, fmt):
    _both_launch_shapes(A, _oracle(A), f"A={A} {fmt}", obs_dtype=getattr(lazy_torch(), fmt))


@pytest.mark.parametrize("A", ac.EXTRA_COUNTS)
def test_large_map_layout_forced(A, monkeypatch):
    monkeypatch.setenv("PGX_BIG", "1")
    _both_launch_shapes(A, _oracle(A), f"A={A} PGX_BIG=1")


@pytest.mark.parametrize("A", ac.EXTRA_COUNTS)
def test_soft_all_stay_index_order(A):
    from pogema_amd import Semantics
    sem = Semantics(soft_vertex="all_stay", soft_occupancy="index_order")
    obstacles, agents, targets, actions, _ = ac.count_instance(A)
    kw = dict(_kw(A, "soft", "finish"), semantics=sem)
    ref = c_oracle_rollout(obstacles, agents, targets, actions, nthreads=8, **kw)
    _both_launch_shapes(A, ref, f"A={A} soft all_stay", kw=kw)


# ---- the closure's last two rounds -------------------------------------------------------------------------------------
def _outcomes_match(obstacles, agents, targets, actions, collision, what):
    """move_outcomes(actions) on the state right after reset_from_state == the reference, all four outputs."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    A = agents.shape[1]
    env = VecPogema(GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=2, collision_system=collision,
                               on_target="nothing", max_episode_steps=64), batch=1, auto_reset=False)
    env.reset_from_state(obstacles, agents, targets)
    got = env.move_outcomes(torch.as_tensor(actions, device=env.device))
    ref = move_outcomes_reference(installed_maps(env), agents, np.ones((1, A), bool), actions, collision)
    for name, g, w in zip(("next_xy", "outcome", "blocker", "counts"), got, ref):
        g = g.cpu().numpy()
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"
    env.close()


@pytest.mark.parametrize("blocked_front", [False, True])
@pytest.mark.parametrize("A", [257, 513, 1022])
def test_longest_follow_chains(A, blocked_front):
    """test_parity_gpu.py's chains with A - 1 links: ceil(log2 A) = 9 and 10 rounds of pointer doubling, across up to 16
    waves.  A blocked head keeps the whole line where it is -- the last agent learns it in the last round."""
    acts = ac.corridor_actions(A)
    for name, order in ac.corridor_orders(A).items():
        obstacles, agents, targets = _corridor_case(A, order, blocked_front)
        for collision in COLLISIONS:
            kw = dict(obs_radius=2, collision_system=collision, on_target="nothing", max_episode_steps=64, auto_reset=False)
            what = f"chain A={A} blocked={blocked_front} {name} {collision}"
            ref = c_oracle_rollout(obstacles, agents, targets, acts, **kw)
            assert_rollouts_equal(ref, engine_rollout(obstacles, agents, targets, acts, **kw), what)
            assert_rollouts_equal(ref, engine_rollout_launch(obstacles, agents, targets, acts, **kw), what + " as one rollout launch")
            _outcomes_match(obstacles, agents, targets, acts[0], collision, what)


@pytest.mark.parametrize("A", [260, 516, 1024])
def test_rotation_cycles(A):
    """test_parity_gpu.py's ring of all agents: a chain with no head, on rings of side 66, 130 and 257."""
    from util import random_actions
    for name, order in ac.corridor_orders(A).items():
        obstacles, agents, targets, acts = ac.ring_case(A, order)
        rollout_acts = np.concatenate([acts, random_actions(3, 1, A, 2)])
        for collision in COLLISIONS:
            kw = dict(obs_radius=2, collision_system=collision, on_target="nothing", max_episode_steps=64, auto_reset=False)
            what = f"rotation A={A} {name} {collision}"
            ref = c_oracle_rollout(obstacles, agents, targets, rollout_acts, **kw)
            got = engine_rollout(obstacles, agents, targets, rollout_acts, **kw)
            assert_rollouts_equal(ref, got, what)
            assert_rollouts_equal(ref, engine_rollout_launch(obstacles, agents, targets, rollout_acts, **kw), what + " as one rollout launch")
            moved = (got["agents_xy"][0, 0] != agents[0]).any(axis=1)
            assert moved.all() if collision == "soft" else not moved.any()
            _outcomes_match(obstacles, agents, targets, acts[0], collision, what)


# ---- the episode-end reduction across 5, 9 and 16 waves -------------------------------------------------------------------
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("variant", ac.END_VARIANTS)
@pytest.mark.parametrize("A", [257, 513, 961])
def test_episode_end_needs_every_wave(A, variant, auto_reset):
    """Every agent steps onto its target in step 1, or all but one: the flags of all waves decide whether the episode
    ends, and the metrics of the step that ends it count all of them."""
    obstacles, agents, targets, acts = ac.episode_end_case(A, variant)
    for collision in COLLISIONS:
        kw = dict(obs_radius=2, collision_system=collision, on_target="finish", max_episode_steps=64, auto_reset=auto_reset,
                  seed=7, env_index_base=3)
        what = f"episode end A={A} {variant} {collision} auto_reset={auto_reset}"
        ref = c_oracle_rollout(obstacles, agents, targets, acts, **kw)
        got = engine_rollout(obstacles, agents, targets, acts, **kw)
        assert_rollouts_equal(ref, got, what)
        assert bool(got["episode_done"][0, 0]) == (variant == "all") and (variant == "all" or got["episode_done"][1, 0])
        assert_rollouts_equal(ref, engine_rollout_launch(obstacles, agents, targets, acts, **kw), what + " as one rollout launch")


# ---- the planners in a crowd ----------------------------------------------------------------------------------------------
def _crowd_env(A):
    from pogema_amd import GridConfig, VecPogema
    obstacles, agents, targets = ac.crowd_case(A)
    env = VecPogema(GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=2, collision_system="soft",
                               on_target="finish", max_episode_steps=64), batch=len(obstacles), auto_reset=False)
    env.reset_from_state(obstacles, agents, targets)
    return env


@pytest.mark.parametrize("A", [341, 512])
def test_crowd_pibt_actions(A):
    from test_pibt_gpu import _check, _priorities
    env = _crowd_env(A)
    prios = _priorities(env, np.random.default_rng(A))
    for k, prio in enumerate(prios):
        actions, _ = _check(env, prio, what=f"crowd A={A} prio#{k}", invariants=True)
    assert int((actions != 0).sum()) > env.batch * A // 4
    env.close()


@pytest.mark.parametrize("make", [random_scores, special_scores], ids=["random_scores", "special_scores"])
@pytest.mark.parametrize("A", [341, 512])
def test_crowd_shield_actions(A, make):
    torch = lazy_torch()
    from test_pibt_gpu import _priorities
    from test_shield_gpu import MODES, _check
    env = _crowd_env(A)
    rng = np.random.default_rng(A)
    scores = torch.as_tensor(make(rng, env.batch, A), device=env.device)   # the scores tests/test_agent_counts.py checks
    prios = _priorities(env, rng)
    for mode in MODES:
        for k, prio in enumerate(prios[:2]):
            _, _, o = _check(env, scores, prio, mode, what=f"crowd A={A} {make.__name__} prio#{k}", invariants=True)
            assert bool(o.any()) and not bool(o.all())
    env.close()


@pytest.mark.parametrize("A", [341, 512])
def test_crowd_pibt_plan(A):
    from test_pibt_plan_gpu import _check, _random_priority
    env = _crowd_env(A)
    st = env.get_state()
    maps, pos, active = installed_maps(env), st["agents_xy"].cpu().numpy(), st["is_active"].cpu().numpy()
    for prio in (None, _random_priority(env, np.random.default_rng(A))):
        _, path, _, _ = _check(env, 4, "finish", prio, what=f"crowd A={A} horizon 4")
        path = path.cpu().numpy()
        for b in range(env.batch):
            assert check_invariants(maps[b], pos[b], active[b], path[0, b]) == [], b
    env.close()


# ---- the slot-based queries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,name", sorted(ac.QUERY_CASES))
def test_slot_based_queries(A, name):
    """expert_actions, cost_to_go, goal_directions and policy_input against their references, on the C oracle's state (which
    the engine's get_state() must equal), after the reset and after four steps that finish some agents."""
    torch = lazy_torch()
    from cost_to_go_reference import cost_to_go_reference
    from expert_reference import expert_reference
    from goal_directions_reference import goal_directions_reference, planes
    from policy_input_reference import CHANNELS, other_goals_reference
    from pogema_amd import GridConfig, VecPogema
    from test_cost_to_go_gpu import CacheModel
    H, W, B, r = ac.QUERY_CASES[(A, name)]
    obstacles, agents, targets, actions, states = ac.query_script(A, name)
    env = VecPogema(GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=r, collision_system="priority",
                               on_target="finish", max_episode_steps=64), batch=B, auto_reset=False)
    env.reset_from_state(obstacles, agents, targets)
    model = CacheModel()
    for when, want in zip(("reset", "after 4 steps"), states):
        what = f"A={A} {name} {when}"
        if when != "reset":
            for t in range(4):
                env.step(torch.as_tensor(actions[t], device=env.device))
        st = env.get_state()
        pos, tgt, active = want["agents_xy"], want["targets_xy"], want["is_active"].astype(bool)
        assert np.array_equal(st["agents_xy"].cpu().numpy(), pos) and np.array_equal(st["targets_xy"].cpu().numpy(), tgt), what
        assert np.array_equal(st["is_active"].cpu().numpy(), active), what
        assert np.array_equal(installed_maps(env), obstacles)
        assert active.all() == (when == "reset")

        for flag in (False, True):
            got_a, got_d = env.expert_actions(agents_as_obstacles=flag)
            ref_a, ref_d = expert_reference(obstacles, pos, tgt, active, flag)
            assert np.array_equal(got_d.cpu().numpy(), ref_d), f"{what}: expert distance, agents_as_obstacles={flag}"
            assert np.array_equal(got_a.cpu().numpy(), ref_a), f"{what}: expert action, agents_as_obstacles={flag}"

        before, predicted = env.cost_to_go_builds, model.call(env)
        got = env.cost_to_go().cpu().numpy()
        assert env.cost_to_go_builds - before == predicted, f"{what}: fields built"
        assert predicted == (B * A if when == "reset" else 0)
        assert np.array_equal(got, cost_to_go_reference(obstacles, pos, tgt, active, r)), f"{what}: cost_to_go"

        bits = goal_directions_reference(obstacles, pos, tgt, active, r)
        for fmt, ref in (("bits", bits), ("uint8", planes(bits)), ("float32", planes(bits).astype(np.float32))):
            got = env.goal_directions(format=fmt).cpu().numpy()
            assert got.dtype == ref.dtype and np.array_equal(got, ref), f"{what}: goal_directions [{fmt}]"

        other = other_goals_reference(pos, tgt, active, r)[:, :, None].astype(np.float32)
        full = np.concatenate([want["obs"], other, planes(bits).astype(np.float32)], axis=2)     # CHANNELS' order
        got = env.policy_input()
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), np.delete(full, 3, axis=2)), f"{what}: default"
        for dtype in (torch.uint8, torch.bfloat16):
            got = env.policy_input(channels=CHANNELS, dtype=dtype)
            assert got.dtype == dtype and tuple(got.shape) == full.shape
            assert np.array_equal(got.float().cpu().numpy(), full), f"{what}: all eight channels as {dtype}"
    env.close()


# ---- the neighbour lists' ragged last chunk ---------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [257, 513, 769, 1023])
def test_neighbour_lists_write_only_their_rows(A):
    """Above 256 agents an env's last workgroup owns fewer than 256 rows (one row at 257, 513 and 769).  The three outputs
    equal the reference, and 256 rows' worth of guard words behind each of them keep their value: a workgroup that took
    its chunk for a full one would write the last env's surplus rows there."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, _lib
    from visible_agents_reference import visible_agents_reference
    assert ac.neighbour_chunk_rows(A)[-1] < 256
    H, W, B, _ = ac.CASES[A]
    B, K, r = 2, 5, 5
    obstacles, agents, targets, _, _ = ac.count_instance(A)
    env = VecPogema(GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=r, max_episode_steps=64), batch=B)
    env.reset_from_state(obstacles[:B], agents[:B], targets[:B])
    ref = visible_agents_reference(agents[:B], np.ones((B, A), bool), r, K)
    n, pad = B * A, 256
    gi = torch.full(((n + pad) * K,), 77, dtype=torch.int32, device=env.device)
    go = torch.full(((n + pad) * K * 2,), 77, dtype=torch.int8, device=env.device)
    gc = torch.full((n + pad,), 77, dtype=torch.int32, device=env.device)
    _lib.check(env._lib.pgx_visible_agents(env._handle, K, 0, gi.data_ptr(), go.data_ptr(), gc.data_ptr(), env._stream()))
    assert np.array_equal(gi[:n * K].view(B, A, K).cpu().numpy(), ref[0])
    assert np.array_equal(go[:n * K * 2].view(B, A, K, 2).cpu().numpy(), ref[1])
    assert np.array_equal(gc[:n].view(B, A).cpu().numpy(), ref[2])
    assert ref[2].max() > 0
    assert bool((gi[n * K:] == 77).all()) and bool((go[n * K * 2:] == 77).all()) and bool((gc[n:] == 77).all())
    env.close()
