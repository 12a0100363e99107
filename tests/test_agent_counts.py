"""CPU: the inputs of tests/test_agent_counts_gpu.py are what they claim (tests/agent_counts.py).  Every count is
admitted by the engine and placed by the host generator; the kernels' integer formulas, restated in Python, give the
waves, envs per workgroup, reservation-set sizes, neighbour chunks and closure rounds the comments name, and together
reach every layout between 257 and 1023 agents that no other suite runs; and the hand-built states have the properties
the GPU tests rely on, shown with the oracle and the references alone."""
import numpy as np
import pytest

import agent_counts as ac
from agent_counts import AGENT_COUNTS, CASES
from move_outcomes_reference import MOVED, OBSTACLE, OCCUPIED, move_outcomes_reference
from pibt_reference import check_invariants, pibt_env
from shield_inputs import random_scores, special_scores
from shield_reference import shield_env
from test_parity_gpu import _corridor_case
from util import c_oracle_rollout

COLLISIONS = ("priority", "block_both", "soft")


# ---- 1: the counts, their maps and batches ------------------------------------------------------------------------------
def test_counts_are_the_listed_ones_and_every_one_has_a_case():
    assert AGENT_COUNTS == (257, 320, 341, 342, 511, 512, 513, 640, 769, 960, 961, 1023)
    assert set(CASES) == set(AGENT_COUNTS)
    small = [a for a in AGENT_COUNTS if max(CASES[a][:2]) <= 64]
    large = [a for a in AGENT_COUNTS if max(CASES[a][:2]) > 64]
    assert len(small) == len(large) == 6
    assert all(CASES[a][0] != CASES[a][1] for a in large), "the large-layout maps are rectangular"
    assert any(CASES[a][0] > 64 for a in large) and any(CASES[a][1] > 64 for a in large), "a tall one and a wide one"
    assert all(h <= 80 and w <= 80 for h, w, _, _ in CASES.values())
    for a, size, batch in ac.LAYOUT_ROWS:
        assert CASES[a][:3] == (size, size, batch)
    assert {a for a, _, _ in ac.LAYOUT_ROWS} >= {257, 342, 512, 513, 1023}


@pytest.mark.parametrize("A", AGENT_COUNTS)
def test_every_case_is_admitted_with_the_largest_radius_that_fits(A, engine_lib):
    H, W, B, r = CASES[A]
    assert ac.config_accepted(A, H, W, B, r)
    assert r == ac.largest_radius(A, H, W, B), "the largest of 1, 5 and 15 the LDS budget admits"
    assert all(ac.config_accepted(A, H, W, B, q) for q in ac.RADII if q < r)


def test_radius_15_is_refused_somewhere_and_admitted_somewhere():
    radii = {CASES[a][3] for a in AGENT_COUNTS}
    assert radii == {5, 15}, "both sides of the LDS limit occur"
    for a, size, batch in ac.LAYOUT_ROWS:
        assert ac.radii_accepted(a, size, batch)[:2] == (1, 5), "the planners' suites run radius 1 and 5 on every row"
    assert ac.radii_accepted(1024, 64, 2) == (1, 5), "what the neighbour suite ran at 1024 agents before"
    assert ac.radii_accepted(200, 28, 3) == (1, 5, 15)


@pytest.mark.parametrize("A", AGENT_COUNTS)
def test_host_generator_places_every_instance(A):
    H, W, B, _ = CASES[A]
    obstacles, agents, targets, actions, _ = ac.count_instance(A)
    assert obstacles.shape == (B, H, W) and agents.shape == targets.shape == (B, A, 2) and actions.shape == (8, B, A)
    for b in range(B):
        assert len({tuple(c) for c in agents[b]}) == A and len({tuple(c) for c in targets[b]}) == A
        for cells in (agents[b], targets[b]):
            assert (cells >= 0).all() and (cells[:, 0] < H).all() and (cells[:, 1] < W).all()
            assert (obstacles[b][cells[:, 0], cells[:, 1]] == 0).all()
        assert 0.05 < obstacles[b].mean() < 0.15
    assert set(np.unique(actions)) == {0, 1, 2, 3, 4}


# ---- the integer formulas: what each count's comment says ---------------------------------------------------------------
#        A: (waves, lanes of the last wave, closure rounds, epb, log2n, neighbour chunk rows)
EXPECTED = {
    257: (5, 1, 9, 3, 10, [256, 1]),
    320: (5, 64, 9, 3, 10, [256, 64]),
    341: (6, 21, 9, 3, 10, [256, 85]),
    342: (6, 22, 9, 2, 10, [256, 86]),
    511: (8, 63, 9, 2, 10, [256, 255]),
    512: (8, 64, 9, 2, 10, [256, 256]),
    513: (9, 1, 10, 1, 11, [256, 256, 1]),
    640: (10, 64, 10, 1, 11, [256, 256, 128]),
    769: (13, 1, 10, 1, 11, [256, 256, 256, 1]),
    960: (15, 64, 10, 1, 11, [256, 256, 256, 192]),
    961: (16, 1, 10, 1, 11, [256, 256, 256, 193]),
    1023: (16, 63, 10, 1, 11, [256, 256, 256, 255]),
}


@pytest.mark.parametrize("A", AGENT_COUNTS)
def test_formulas_give_what_the_comments_say(A):
    B = CASES[A][2]
    T, epb, log2n, grid, last = ac.pibt_geometry(A, B)
    got = (ac.waves(A), ac.last_wave_lanes(A), ac.closure_rounds(A), epb, log2n, ac.neighbour_chunk_rows(A))
    assert got == EXPECTED[A]
    assert T == 1024 and epb * A <= T < (epb + 1) * A
    assert (1 << log2n) >= 2 * A > (1 << (log2n - 1))
    assert sum(ac.neighbour_chunk_rows(A)) == A
    assert B == {3: 5, 2: 3, 1: 2}[epb], "batch 5 where epb = 3, 3 where epb = 2, 2 where epb = 1"
    assert grid == 2 and (last < epb or epb == 1), "a second workgroup, partly filled wherever epb allows it"


def test_counts_reach_every_row_of_the_coverage_table():
    """The rows of the gap this file closes, each reached by at least one listed count."""
    by = {a: EXPECTED[a] for a in AGENT_COUNTS}
    waves = {v[0] for v in by.values()}
    # step / rollout, multi-wave: both ends of the range 5..15 and waves in between, full and ragged last waves, and 16
    # waves with a ragged last wave (961..1023)
    assert {5, 6, 8, 9, 10, 13, 15} <= waves and min(waves) == 5
    assert any(v[0] == 16 and v[1] < 64 for v in by.values())
    for lanes in (1, 63, 64):
        assert any(v[1] == lanes and 5 <= v[0] <= 15 for v in by.values()), lanes
    # closure rounds 9 and 10 (the chains that make them work are further down)
    assert {v[2] for v in by.values()} == {9, 10}
    # PIBT family at 1024 lanes: epb 3, 2 and 1, idle tail lanes, no idle lane, log2n 10 and 11, the set exactly 2A words
    assert {v[3] for v in by.values()} == {1, 2, 3}
    idle = {a: 1024 - v[3] * a for a, v in by.items()}
    assert idle[512] == 0 and idle[341] == 1 and idle[342] == 340 and idle[1023] == 1
    assert {v[4] for v in by.values()} == {10, 11}
    assert (1 << by[512][4]) == 2 * 512 and all((1 << v[4]) > 2 * a for a, v in by.items() if a != 512)
    assert any(v[4] == 11 and v[3] == 1 and CASES[a][2] == 2 for a, v in by.items())
    # outcomes_kernel's counts: envs that start in the middle of a wave (257, 514 / 342, ...)
    starts = {s for a in AGENT_COUNTS for s in ac.env_first_lanes(a, CASES[a][2])}
    assert {257, 514, 342} <= starts and any(s % 64 for s in starts)
    # neighbour lists above 256 agents: 2, 3 and 4 chunks, a one-row last chunk at each, full and 255-row last chunks
    chunks = [v[5] for v in by.values()]
    assert {len(c) for c in chunks} == {2, 3, 4}
    for n in (2, 3, 4):
        assert any(len(c) == n and c[-1] == 1 for c in chunks), n
    assert any(c[-1] == 256 for c in chunks) and any(c[-1] == 255 for c in chunks)
    assert any(c[-1] <= 64 for c in chunks) and any(64 < c[-1] <= 128 for c in chunks), "one, two ... waves return early"
    # cost-to-go builds: between 200 and 1024 stale slots per env, on both layouts
    assert all(200 < a < 1024 for a in AGENT_COUNTS)
    assert {max(CASES[a][:2]) > 64 for a in AGENT_COUNTS} == {False, True}
    assert {max(v[:2]) > 64 for v in ac.QUERY_CASES.values()} == {False, True}
    # policy_input / dir_gather: above 130 agents
    assert {a for a, _ in ac.QUERY_CASES} == {257, 513, 1023}


def test_pairings_rotate_so_that_each_meets_four_counts():
    met = {}
    for a in AGENT_COUNTS:
        met.setdefault(ac.pairing_of(a), []).append(a)
    assert set(met) == set(ac.PAIRINGS) and all(len(v) >= 4 for v in met.values()), met
    assert set(ac.EXTRA_COUNTS) == {257, 512, 513, 1023}


# ---- 2: the rollouts end episodes and move agents ---------------------------------------------------------------------
@pytest.mark.parametrize("A", AGENT_COUNTS)
def test_eight_steps_end_an_episode_in_every_env(A):
    obstacles, agents, targets, actions, r = ac.count_instance(A)
    collision, on_target = ac.pairing_of(A)
    ref = c_oracle_rollout(obstacles, agents, targets, actions, obs_radius=r, collision_system=collision, on_target=on_target,
                           max_episode_steps=5, auto_reset=True, seed=1234, env_index_base=17, nthreads=4)
    assert ref["episode_done"][4].all() and ref["truncated"][4].all(), "the time limit ends every env's episode at step 5"
    assert ref["metrics"][4].any()
    assert np.array_equal(ref["elapsed"][5], np.ones_like(ref["elapsed"][5])), "and the auto-reset starts the next one"
    moved = (ref["agents_xy"][1] != ref["agents_xy"][0]).any(-1)
    assert 0.2 < moved.mean() < 0.9, "some moves succeed and some do not"


# ---- 3: the closure's last rounds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [257, 513, 1022])
def test_a_chain_of_all_agents_moves_or_stays_as_one(A):
    """A - 1 links: ceil(log2 A) doubling rounds are needed and no fewer (8 rounds close 255 links)."""
    assert ac.closure_rounds(A) == (9 if A == 257 else 10) and A - 1 > 2 ** (ac.closure_rounds(A) - 1) - 1
    assert ac.config_accepted(A, 3, A + 2, 1, 2)
    acts = ac.corridor_actions(A)
    active = np.ones((1, A), bool)
    all_moved = {c: [] for c in COLLISIONS}
    for name, order in ac.corridor_orders(A).items():
        for blocked in (False, True):
            obstacles, agents, targets = _corridor_case(A, order, blocked)
            head = int(order[A - 1])
            for collision in COLLISIONS:
                ref = c_oracle_rollout(obstacles, agents, targets, acts, obs_radius=2, collision_system=collision,
                                       on_target="nothing", max_episode_steps=64, auto_reset=False)
                moved = (ref["agents_xy"][0, 0] != agents[0]).any(axis=1)
                next_xy, outcome, blocker, counts = move_outcomes_reference(obstacles, agents, active, acts[0], collision)
                assert np.array_equal(next_xy, ref["agents_xy"][0]), "the outcome reference and the oracle agree"
                if blocked:
                    assert not moved.any(), (name, collision)
                    assert outcome[0, head] == OBSTACLE and (np.delete(outcome[0], head) == OCCUPIED).all()
                    behind = np.empty(A, np.int64)
                    behind[order[:-1]] = order[1:]          # the agent in front of each
                    assert np.array_equal(np.delete(blocker[0], head), np.delete(behind, head))
                    assert counts[0].tolist() == [0, 0, 1, 0, A - 1, 0, 0]
                else:
                    assert moved[head]
                    all_moved[collision].append(bool(moved.all()))
                    assert (outcome[0][moved] == MOVED).all()
    assert all(all_moved["soft"]), "under soft the whole free line moves, whatever the index order"
    assert any(all_moved["priority"]) and not all(all_moved["priority"]), "under priority only when the head plans first"


@pytest.mark.parametrize("A", [260, 516, 1024])
def test_a_ring_of_all_agents_rotates_under_soft_only(A):
    n = A // 4 + 1
    assert 4 * (n - 1) == A and ac.config_accepted(A, n, n, 1, 2)
    for name, order in ac.corridor_orders(A).items():
        obstacles, agents, targets, acts = ac.ring_case(A, order)
        assert int((obstacles == 0).sum()) == A
        for collision in COLLISIONS:
            ref = c_oracle_rollout(obstacles, agents, targets, acts, obs_radius=2, collision_system=collision,
                                   on_target="nothing", max_episode_steps=64, auto_reset=False)
            moved = (ref["agents_xy"][0, 0] != agents[0]).any(axis=1)
            assert moved.all() if collision == "soft" else not moved.any(), (name, collision)


# ---- 4: the episode-end reduction --------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("A", [257, 513, 961])
def test_one_idling_agent_keeps_the_episode_open(A, auto_reset):
    assert ac.last_wave_lanes(A) == 1, "agent A - 1 is the only lane of the last wave"
    for variant in ac.END_VARIANTS:
        obstacles, agents, targets, acts = ac.episode_end_case(A, variant)
        assert len({tuple(c) for c in np.concatenate([agents[0], targets[0]])}) == 2 * A, "all cells disjoint"
        assert (np.abs(agents - targets).sum(-1) == 1).all() and not obstacles.any()
        idler = ac.idler_of(A, variant)
        if variant == "middle_idles":
            assert 0 < idler // 64 < ac.waves(A) - 1
        for collision in COLLISIONS:
            ref = c_oracle_rollout(obstacles, agents, targets, acts, obs_radius=2, collision_system=collision,
                                   on_target="finish", max_episode_steps=64, auto_reset=auto_reset, seed=7, env_index_base=3)
            if variant == "all":
                assert ref["episode_done"][0, 0] and ref["terminated"][0].all()
                assert ref["metrics"][0, 0].any()
            else:
                assert not ref["episode_done"][0, 0] and not ref["terminated"][0, 0, idler]
                assert ref["terminated"][0, 0].sum() == A - 1
                assert ref["episode_done"][1, 0] and ref["terminated"][1, 0, idler], "it ends once the idler arrives"
                assert ref["metrics"][1, 0].any()


# ---- 5: the crowded planner inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [341, 512])
def test_crowd_makes_pibt_calls_fail_in_every_env(A):
    obstacles, agents, targets = ac.crowd_case(A)
    B, side = obstacles.shape[:2]
    T, epb, log2n, grid, last = ac.pibt_geometry(A, B)
    assert grid == 2 and last < epb and not obstacles.any()
    assert 0.49 < A / (side * side) < 0.51, "the agents stand on half of the cells"
    if A == 512:
        assert (1 << log2n) == 2 * A, "one reservation per agent fills half of the set: its design point"
    active = np.ones(A, bool)
    rng = np.random.default_rng(A)
    scores = {"random": random_scores(rng, B, A), "special": special_scores(rng, B, A)}
    with ac.shared_fields(obstacles, targets):
        for b in range(B):
            assert len({tuple(c) for c in agents[b]}) == A and len({tuple(c) for c in targets[b]}) == A
            want_a, want_n = pibt_env(obstacles[b], agents[b], targets[b], active)
            a, n, _, failed = shield_env(obstacles[b], agents[b], targets[b], active, np.zeros((A, 5), np.float32), None, "distance")
            assert np.array_equal(a, want_a) and np.array_equal(n, want_n), "equal scores + distance = the planner"
            assert failed >= 1, f"env {b}: no PIBT call failed"
            assert check_invariants(obstacles[b], agents[b], active, n) == []
            assert (a != 0).sum() > A // 4, "and yet many agents move"
            for name, s in scores.items():
                for mode in (None, "distance"):
                    a, n, o, failed = shield_env(obstacles[b], agents[b], targets[b], active, s[b], None, mode)
                    assert failed >= 1, f"env {b}, {name} scores, tie_break {mode}: no PIBT call failed"
                    assert check_invariants(obstacles[b], agents[b], active, n) == []
                    assert 0 < o.sum() < A


def test_memoised_fields_are_the_plain_searches():
    """agent_counts.shared_fields hands the planners' references pibt_plan_reference's prefilled fields."""
    import pibt_plan_reference
    from expert_reference import bfs_from
    obstacles, agents, targets, _, _ = ac.count_instance(257)
    blocked = obstacles[0] != 0
    with ac.shared_fields(obstacles[:1], targets[:1, :40]):
        import pibt_reference
        assert pibt_reference.bfs_from is pibt_plan_reference._bfs_memo
        for tx, ty in targets[0, :40]:
            assert np.array_equal(pibt_reference.bfs_from(blocked, int(tx), int(ty)), bfs_from(blocked, int(tx), int(ty)))
    assert pibt_reference.bfs_from is bfs_from


# ---- 6: the states of the slot-based queries -------------------------------------------------------------------------------
@pytest.mark.parametrize("A,name", sorted(ac.QUERY_CASES))
def test_query_states_hold_inactive_agents_after_the_steps(A, name):
    H, W, B, r = ac.QUERY_CASES[(A, name)]
    assert ac.config_accepted(A, H, W, B, r) and (max(H, W) > 64) == (name == "large") and (name == "large" or max(H, W) <= 64)
    obstacles, agents, targets, actions, states = ac.query_script(A, name)
    assert actions.shape == (4, B, A) and len(states) == 2
    assert states[0]["is_active"].all()
    assert np.array_equal(states[0]["agents_xy"], agents) and np.array_equal(states[0]["targets_xy"], targets)
    after = states[1]["is_active"].astype(bool)
    assert not after.all(), "no agent finished within four steps"
    assert after.sum() > A * B // 2
    assert len({tuple(c) for c in targets[0]}) == ac.QUERY_TARGETS
    assert states[1]["obs"].shape == (B, A, 3, 2 * r + 1, 2 * r + 1)
