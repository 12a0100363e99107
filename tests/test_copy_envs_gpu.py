"""GPU: copy_envs (docs/SPEC.md S19) by its properties -- a copy at t = 0 equals a reset with duplicated rows, a copy at
t > 0 behaves like its source, on the shapes at which a row copy can go wrong; equal and unequal maps in one call; map
pools; the distance-field cache; refusals and the defined skip of out-of-range pairs; graph capture; PibtPolicy."""
import numpy as np
import pytest

from copy_envs_reference import (assert_rows_equal, component_labels, instances, make_env, random_steps,
                                 step_record, with_rows_replaced)
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

COLLISIONS = ("priority", "block_both", "soft")
ON_TARGET = ("finish", "restart", "nothing")


def _others(batch, dst):
    return np.setdiff1d(np.arange(batch), np.asarray(dst))


# ---- 1: a copy at t = 0 equals a reset with duplicated rows --------------------------------------------------------------
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("on_target, numpy_rng", [(m, False) for m in ON_TARGET] + [("finish", True), ("nothing", True)])
@pytest.mark.parametrize("collision", COLLISIONS)
def test_copy_at_reset_equals_a_reset_with_duplicated_rows(collision, on_target, numpy_rng, auto_reset):
    """Engine E installs rows S and copies; engine R installs S with row dst[k] replaced by row src[k].  Every output of
    every row is bit-identical over max_episode_steps + 3 steps.  Under on_target="restart" this is the default
    lifelong stream: the copy draws what env dst[k] draws, exactly as the duplicated row of R does.  (lifelong_rng="numpy"
    draws nothing under "finish" and "nothing"; with "restart" it is the next test.)"""
    B, A, T = 6, 5, 8
    S = instances(B, 8, 8, A, seed=11)
    src, dst = [0, 0, 4], [1, 2, 5]
    kw = dict(r=2, collision=collision, on_target=on_target, max_steps=T, auto_reset=auto_reset, numpy_rng=numpy_rng, seed=5,
              env_index_base=3)
    E = make_env(*S, **kw)
    E.copy_envs(src, dst)
    R = make_env(*with_rows_replaced(S, src, dst), **kw)
    for t, a in enumerate(random_steps(T + 3, B, A, seed=1)):
        assert_rows_equal(step_record(E, a), np.arange(B), step_record(R, a), np.arange(B), f"step {t}")
    E.close()
    R.close()


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("collision", COLLISIONS)
def test_copy_at_reset_with_numpy_generators(collision, auto_reset):
    """lifelong_rng="numpy", on_target="restart": the generators are part of the copied state (S19), so the copy draws
    its SOURCE's targets, where the duplicated row of R, a fresh reset of slot dst[k], draws from slot dst[k]'s own
    generators.  What holds, with the copy fed its source's actions: rows that are no destination equal R's throughout;
    a copy equals its source in every output while the episode lasts, its last step included; and once auto-reset has
    restored slot dst[k]'s own generators (they belong to the slot, like the default stream's key), the copy equals
    the duplicated row of R again."""
    B, A, T = 6, 5, 8
    S = instances(B, 8, 8, A, seed=12)
    src, dst = [0, 0, 4], [1, 2, 5]
    kw = dict(r=2, collision=collision, on_target="restart", max_steps=T, auto_reset=auto_reset, numpy_rng=True, seed=5,
              env_index_base=3)
    E = make_env(*S, **kw)
    E.copy_envs(src, dst)
    R = make_env(*with_rows_replaced(S, src, dst), **kw)
    keep = _others(B, dst)
    for t, a in enumerate(random_steps(T + 3, B, A, seed=2)):
        a[dst] = a[src]
        e, r = step_record(E, a), step_record(R, a)
        assert_rows_equal(e, keep, r, keep, f"step {t}, rows that are no destination")
        if t < T or not auto_reset:
            assert_rows_equal(e, dst, e, src, f"step {t}, copy against source")
        if t >= T and auto_reset:
            assert_rows_equal(e, dst, r, dst, f"step {t}, copy against the duplicated row after auto-reset")
    E.close()
    R.close()


# ---- 2 and 3: a copy at t > 0 behaves like its source, on every shape -----------------------------------------------------
def _copy_behaves_like_source(B, H, W, A, r, src, dst, *, collision, on_target, auto_reset, numpy_rng=False, T=10, warm=4,
                              seed=0, density=0.3, cache=True):
    """Engine E and its twin run `warm` steps of mostly-expert actions; E copies; both go on for T more steps, every
    destination fed its source's actions.  Rows dst[k] of E equal rows src[k] of E, rows that are no destination equal
    the twin's."""
    S = instances(B, H, W, A, seed=seed, density=density)
    kw = dict(r=r, collision=collision, on_target=on_target, max_steps=warm + T - 3, auto_reset=auto_reset,
              numpy_rng=numpy_rng, seed=seed)
    E, twin = make_env(*S, **kw), make_env(*S, **kw)
    rng = np.random.default_rng(seed)
    for t in range(warm):
        a = mixed_actions(E, rng, 0.7).cpu().numpy()
        assert_rows_equal(step_record(E, a), np.arange(B), step_record(twin, a), np.arange(B), f"warm-up step {t}")
    E.copy_envs(src, dst, cache=cache)
    src_of = np.broadcast_to(np.asarray(src), (len(dst),))
    keep = _others(B, dst)
    ended = False
    for t in range(T):
        a = mixed_actions(E, rng, 0.7).cpu().numpy()
        a[dst] = a[src_of]
        e, w = step_record(E, a), step_record(twin, a)
        assert_rows_equal(e, keep, w, keep, f"step {t} after the copy, rows that are no destination")
        if not ended:
            assert_rows_equal(e, dst, e, src_of, f"step {t} after the copy, copy against source")
        # numpy generators and auto-reset: the reset restores the generators of the SLOT (S19), so the rows part there
        ended = ended or (numpy_rng and auto_reset and bool(e["episode_done"][src_of].any()))
    if numpy_rng and auto_reset:
        assert ended, "the time limit lies inside the run"
    E.close()
    twin.close()


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("on_target, numpy_rng", [("finish", False), ("nothing", False), ("restart", True)])
@pytest.mark.parametrize("collision", COLLISIONS)
def test_copy_behaves_like_its_source(collision, on_target, numpy_rng, auto_reset):
    _copy_behaves_like_source(7, 8, 8, 5, 2, [0, 0, 3], [1, 2, 6], collision=collision, on_target=on_target,
                              auto_reset=auto_reset, numpy_rng=numpy_rng, seed=21)


# (batch, H, W, agents, radius, src, dst): every map of a case is a different random map, so the map rows are copied
_MANY_SRC = [0, 1, 2] * 6 + [0, 1]
_MANY_DST = list(range(5, 25))
SHAPES = {
    "A1": (4, 8, 8, 1, 2, [0], [3]), "A3": (4, 8, 8, 3, 2, [0, 2], [3, 1]), "A5": (4, 8, 8, 5, 2, [1], [0]),
    "A64": (3, 16, 16, 64, 2, [0], [2]), "A65": (3, 16, 16, 65, 2, [2], [0]),
    "A257": (3, 24, 24, 257, 2, [1], [2]),
    "5x7": (5, 5, 7, 4, 2, [0, 0], [4, 1]), "9x33": (5, 9, 33, 6, 3, [3, 3], [0, 2]),
    "r1": (4, 10, 10, 4, 1, [0], [1]), "r15": (4, 10, 10, 4, 15, [0], [3]),
    "batch2": (2, 8, 8, 4, 2, [1], [0]),
    "batch37": (37, 8, 8, 3, 2, _MANY_SRC, _MANY_DST),
}


@pytest.mark.parametrize("on_target, numpy_rng", [("finish", False), ("restart", True)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_where_a_row_copy_can_go_wrong(shape, on_target, numpy_rng):
    """Unaligned agent rows (A = 1, 3, 5), the wave boundary (64, 65), several waves (257), odd byte rows and bitmap rows
    of two words (5 x 7, 9 x 33), the smallest and the largest radius, one pair in a batch of two, 20 pairs from 3
    sources.  "restart" with numpy generators copies every array the engine has (draw counters, 40-byte generators,
    component tables); "finish" has agents that are no longer active."""
    B, H, W, A, r, src, dst = SHAPES[shape]
    assert len(set(dst)) == len(dst) and not set(dst) & set(src)
    _copy_behaves_like_source(B, H, W, A, r, src, dst, collision="soft", on_target=on_target, auto_reset=False,
                              numpy_rng=numpy_rng, T=6, warm=3, seed=31, density=0.1 if A > 64 else 0.3)


@pytest.mark.parametrize("collision", COLLISIONS)
def test_default_lifelong_stream_stays_keyed_on_the_destination(collision):
    """on_target="restart" with the build's counter stream: the step after the copy gives both rows the same positions,
    rewards and active flags (the move phase reads copied state only); every target the copy holds from then on lies in
    the 4-connected component of its agent's cell."""
    B, H, W, A = 6, 8, 8, 5
    S = instances(B, H, W, A, seed=41)
    E = make_env(*S, r=2, collision=collision, on_target="restart", max_steps=64, seed=9)
    rng = np.random.default_rng(41)
    for t in range(5):
        step_record(E, mixed_actions(E, rng, 0.8).cpu().numpy())
    src, dst = [0, 0, 3], [1, 2, 4]
    E.copy_envs(src, dst)
    maps = installed_maps(E)
    assert np.array_equal(maps[dst], maps[src])
    labels = [component_labels(m) for m in maps]
    for t in range(12):
        a = mixed_actions(E, rng, 0.8).cpu().numpy()
        a[dst] = a[src]
        e = step_record(E, a)
        if t == 0:
            assert_rows_equal(e, dst, e, src, "first step after the copy", fields=("agents_xy", "rewards", "is_active"))
        for b in dst:
            at, to = e["agents_xy"][b], e["targets_xy"][b]
            here, there = labels[b][at[:, 0], at[:, 1]], labels[b][to[:, 0], to[:, 1]]
            assert (here >= 0).all() and np.array_equal(here, there), f"step {t}, env {b}: a target outside the agent's component"
    E.close()


# ---- 4: equal and unequal maps in one call; map pools ------------------------------------------------------------------------
def test_equal_and_unequal_maps_in_one_call():
    """Rows 0..3 share one map, rows 4..7 have their own.  Pairs (0 -> 1), (0 -> 2) copy inside one map (the map rows are
    skipped), (4 -> 3) and (5 -> 6) bring a new map: afterwards every destination holds its source's state and map, and
    goes on like it -- with component tables that must be the source's, under numpy generators."""
    B, H, W, A = 8, 9, 9, 4
    obst, agents, targets = instances(B, H, W, A, seed=51)
    # rows 0..3: one map, and 4 A start/target pairs of ONE instance on it dealt out over the four rows
    one = instances(1, H, W, 4 * A, seed=52, density=0.2)
    obst[:4] = one[0][0]
    agents[:4], targets[:4] = one[1][0].reshape(4, A, 2), one[2][0].reshape(4, A, 2)
    E = make_env(obst, agents, targets, r=2, collision="priority", on_target="restart", max_steps=64, numpy_rng=True, seed=3)
    rng = np.random.default_rng(5)
    for t in range(3):
        step_record(E, mixed_actions(E, rng, 0.8).cpu().numpy())
    src, dst = [0, 4, 0, 5], [1, 3, 2, 6]
    before, maps0 = E.get_state(occupancy=True), installed_maps(E)
    E.copy_envs(src, dst)
    after, maps1 = E.get_state(occupancy=True), installed_maps(E)
    keep = _others(B, dst)
    for k in before:
        assert np.array_equal(after[k][dst].cpu().numpy(), before[k][src].cpu().numpy()), k
        assert np.array_equal(after[k][keep].cpu().numpy(), before[k][keep].cpu().numpy()), k
    assert np.array_equal(maps1[dst], maps0[src]) and np.array_equal(maps1[keep], maps0[keep])
    assert not np.array_equal(maps0[3], maps0[4]) and np.array_equal(maps0[1], maps0[0])
    for t in range(10):
        a = mixed_actions(E, rng, 0.8).cpu().numpy()
        a[dst] = a[src]
        e = step_record(E, a)
        assert_rows_equal(e, dst, e, src, f"step {t} after the copy")
    E.close()


def test_map_pool_index_is_copied_and_the_slot_keeps_its_draws():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A, M = 8, 3, 5
    pool = (np.random.default_rng(7).random((M, 10, 10)) < 0.2).astype(np.uint8)
    gc = GridConfig(size=10, num_agents=A, obs_radius=2, seed=2, on_target="restart", max_episode_steps=32)
    E, twin = VecPogema(gc, batch=B, map_pool=pool), VecPogema(gc, batch=B, map_pool=pool)
    E.reset(seed=2)
    twin.reset(seed=2)
    idx0 = E.map_index.cpu().numpy()
    src = int(np.flatnonzero(idx0 != idx0[0])[0])   # an env on another pool map than env 0
    rest = [b for b in range(1, B) if b != src]
    pairs_src, pairs_dst = [src, rest[0]], [0, rest[1]]
    st0, maps0 = E.get_state(), installed_maps(E)
    E.copy_envs(pairs_src, pairs_dst)
    idx1, st1, maps1 = E.map_index.cpu().numpy(), E.get_state(), installed_maps(E)
    assert np.array_equal(idx1[pairs_dst], idx0[pairs_src]) and idx1[0] != idx0[0]
    assert np.array_equal(maps1[pairs_dst], maps0[pairs_src]) and np.array_equal(maps1[pairs_dst], pool[idx1[pairs_dst]])
    for k in st0:
        assert torch.equal(st1[k][pairs_dst], st0[k][pairs_src]), k
    # the generation counter belongs to the slot: a reset of the destinations draws what the twin's slots draw
    mask = torch.zeros(B, dtype=torch.bool, device=E.device)
    mask[pairs_dst] = True
    E.reset_where(mask)
    twin.reset_where(mask)
    idx2 = E.map_index.cpu().numpy()
    assert ((idx2 >= 0) & (idx2 < M)).all() and np.array_equal(installed_maps(E)[pairs_dst], pool[idx2[pairs_dst]])
    assert np.array_equal(idx2[pairs_dst], twin.map_index.cpu().numpy()[pairs_dst])
    st2, stw = E.get_state(), twin.get_state()
    for k in st2:
        assert torch.equal(st2[k][pairs_dst], stw[k][pairs_dst]), k
    E.close()
    twin.close()


# ---- 5: the distance-field cache -------------------------------------------------------------------------------------------------
def _cache_env(seed):
    B, H, W, A = 6, 10, 10, 4
    E = make_env(*instances(B, H, W, A, seed=seed), r=2, collision="priority", on_target="finish", max_steps=64)
    rng = np.random.default_rng(seed)
    for t in range(4):
        step_record(E, mixed_actions(E, rng, 0.8).cpu().numpy())
    return E


def _assert_queries_equal_references(E):
    from cost_to_go_reference import cost_to_go_reference
    from goal_directions_reference import goal_directions_reference
    from pibt_reference import pibt_reference
    st = {k: v.cpu().numpy() for k, v in E.get_state().items()}
    args = (installed_maps(E), st["agents_xy"], st["targets_xy"], st["is_active"])
    assert np.array_equal(E.cost_to_go().cpu().numpy(), cost_to_go_reference(*args, E.obs_radius))
    assert np.array_equal(E.goal_directions(format="bits").cpu().numpy(), goal_directions_reference(*args, E.obs_radius))
    actions, next_xy = E.pibt_actions()
    want_a, want_xy = pibt_reference(*args)
    assert np.array_equal(actions.cpu().numpy(), want_a) and np.array_equal(next_xy.cpu().numpy(), want_xy)


def test_cache_rows_are_copied_and_nothing_is_rebuilt():
    E = _cache_env(61)
    E.cost_to_go()
    built = E.cost_to_go_builds
    assert built > 0
    E.copy_envs([0, 0, 3], [1, 2, 5], cache=True)
    _assert_queries_equal_references(E)
    assert E.cost_to_go_builds == built, "a query after copy_envs(cache=True) built fields"
    E.close()


def test_without_the_cache_rows_the_refresh_rebuilds_them():
    E = _cache_env(61)
    E.cost_to_go()
    built = E.cost_to_go_builds
    dst = [1, 2, 5]
    E.copy_envs([0, 0, 3], dst, cache=False)
    active = int(E.get_state()["is_active"][dst].sum())
    _assert_queries_equal_references(E)
    assert built <= E.cost_to_go_builds <= built + active
    E.close()


def test_no_cache_allocated_none_is_made():
    E = _cache_env(62)
    E.copy_envs([0, 0, 3], [1, 2, 5])
    assert E.cost_to_go_builds == 0
    active = int(E.get_state()["is_active"].sum())
    _assert_queries_equal_references(E)
    # the first query allocated the cache and built every field: copy_envs had left nothing behind
    assert E.cost_to_go_builds == active
    E.close()


# ---- 6: refusals and robustness ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_refusals_name_the_entry(on_device):
    torch = lazy_torch()
    E = make_env(*instances(6, 8, 8, 3, seed=71), r=2)
    before = E.get_state(occupancy=True)

    def conv(v):
        return torch.as_tensor(v, dtype=torch.int32, device=E.device) if on_device else v

    for src, dst, needle in (([0, 1], [2, 2], "dst[1] = 2 is given twice"), ([0, 2], [2, 3], "dst[0] = 2 is also a source"),
                             ([0, 6], [1, 2], "src[1] = 6 is outside 0..5"), ([0, 1], [2, -1], "dst[1] = -1 is outside 0..5"),
                             ([0, 1, 2], [3, 4], "src has 3 entries and dst has 2")):
        with pytest.raises(ValueError) as err:
            E.copy_envs(conv(src), conv(dst))
        assert needle in str(err.value)
    after = E.get_state(occupancy=True)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    E.close()


@pytest.mark.parametrize("bad", ["batch + 5", "-1"])
@pytest.mark.parametrize("where", ["src", "dst"])
def test_out_of_range_pair_is_skipped_without_validation(where, bad):
    """validate=False: the kernel's bounds check skips the pair with an index outside 0..batch-1; the valid pairs are
    copied, every other env is untouched, nothing is raised."""
    torch = lazy_torch()
    B = 6
    E = make_env(*instances(B, 9, 9, 5, seed=72), r=2, collision="soft", on_target="restart", numpy_rng=True)
    rng = np.random.default_rng(72)
    for t in range(3):
        step_record(E, mixed_actions(E, rng, 0.8).cpu().numpy())
    E.cost_to_go()
    index = B + 5 if bad == "batch + 5" else -1
    src, dst = [0, 3, 0], [1, 4, 2]
    (src if where == "src" else dst)[1] = index
    before, maps0 = E.get_state(occupancy=True), installed_maps(E)
    E.copy_envs(torch.tensor(src, dtype=torch.int32, device=E.device), torch.tensor(dst, dtype=torch.int32, device=E.device),
                validate=False)
    torch.cuda.synchronize()
    after, maps1 = E.get_state(occupancy=True), installed_maps(E)
    want_src, want_dst, keep = [0, 0], [1, 2], [0, 3, 4, 5]
    for k in before:
        assert torch.equal(after[k][want_dst], before[k][want_src]), k
        assert torch.equal(after[k][keep], before[k][keep]), k
    assert np.array_equal(maps1[want_dst], maps0[want_src]) and np.array_equal(maps1[keep], maps0[keep])
    _assert_queries_equal_references(E)
    E.close()


def test_src_equal_dst_leaves_the_state_bit_identical():
    torch = lazy_torch()
    E = make_env(*instances(5, 8, 8, 4, seed=73), r=2, collision="soft", on_target="restart", numpy_rng=True)
    rng = np.random.default_rng(73)
    for t in range(3):
        step_record(E, mixed_actions(E, rng, 0.8).cpu().numpy())
    blob = E.save_state()["engine"].clone()
    E.copy_envs([0, 2, 4], [0, 2, 4])
    E.copy_envs(3, [3])
    assert torch.equal(E.save_state()["engine"], blob)
    E.copy_envs([], [])
    assert torch.equal(E.save_state()["engine"], blob)
    E.close()


def test_snapshot_round_trip_is_unchanged_and_sees_the_copy():
    """save_state() / load_state() share the segment table with copy_envs: a snapshot taken after a copy restores it."""
    torch = lazy_torch()
    E = make_env(*instances(5, 8, 8, 4, seed=74), r=2, on_target="restart")
    E.copy_envs(0, [1, 3])
    snap = E.save_state()
    a = random_steps(3, 5, 4, seed=74)
    first = [step_record(E, x) for x in a]
    E.load_state(snap)
    for t, x in enumerate(a):
        assert_rows_equal(step_record(E, x), np.arange(5), first[t], np.arange(5), f"step {t} after load_state")
    E.close()


# ---- 7: graph capture ----------------------------------------------------------------------------------------------------------
def test_copy_and_step_in_one_graph():
    """copy_envs(validate=False) with int32 device tensors, then step(): captured once on one stream, replayed with
    other index contents; equals the eager sequence on a twin."""
    torch = lazy_torch()
    B, A = 16, 6
    S = instances(B, 12, 12, A, seed=81)
    kw = dict(r=3, collision="soft", on_target="finish", max_steps=12, auto_reset=True)
    eager, graphed = make_env(*S, **kw), make_env(*S, **kw)
    d_src = torch.tensor([0, 0, 5], dtype=torch.int32, device="cuda")
    d_dst = torch.tensor([1, 2, 6], dtype=torch.int32, device="cuda")
    static_actions = torch.zeros((B, A), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch's graph recipe asks
        graphed.copy_envs(d_src, d_dst, validate=False)
        graphed.step(static_actions)
    torch.cuda.current_stream().wait_stream(side)
    eager.copy_envs(d_src, d_dst, validate=False)
    eager.step(static_actions)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.copy_envs(d_src, d_dst, validate=False)
        out = graphed.step(static_actions)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for t, (src, dst) in enumerate((([3, 3, 9], [4, 8, 10]), ([15, 7, 7], [0, 11, 12]))):
        acts = torch.randint(0, 5, (B, A), generator=gen, device="cuda")
        static_actions.copy_(acts)
        d_src.copy_(torch.tensor(src, dtype=torch.int32))
        d_dst.copy_(torch.tensor(dst, dtype=torch.int32))
        g.replay()
        eager.copy_envs(src, dst)
        ref = eager.step(acts)
        for a, b in zip(out[:4], ref[:4]):
            assert torch.equal(a, b), f"replay {t}"
        assert torch.equal(out[4]["is_active"], ref[4]["is_active"])
        se, sg = eager.get_state(occupancy=True), graphed.get_state(occupancy=True)
        for k in se:
            assert torch.equal(se[k], sg[k]), f"replay {t}: {k}"
    eager.close()
    graphed.close()


# ---- 8: PibtPolicy -----------------------------------------------------------------------------------------------------------------
def test_pibt_policy_copies_its_priorities():
    torch = lazy_torch()
    from pogema_amd import PibtPolicy
    B, A = 6, 6
    E = make_env(*instances(B, 10, 10, A, seed=91), r=2, collision="soft", on_target="finish", max_steps=64)
    policy = PibtPolicy(E)
    for t in range(5):
        actions, _ = policy.act()
        _, rew, _, _, infos = E.step(actions)
        policy.update(rew, infos["episode_done"])
    assert bool((policy.priority > 0).any())
    src, dst = [0, 0, 4], [1, 2, 5]
    keep = [0, 3, 4]
    before = policy.priority.clone()
    policy.copy_envs(src, dst)
    assert torch.equal(policy.priority[dst], before[src]) and torch.equal(policy.priority[keep], before[keep])
    actions, next_xy = policy.act()
    assert torch.equal(actions[dst], actions[src]) and torch.equal(next_xy[dst], next_xy[src])
    st = E.get_state()
    for k in st:
        assert torch.equal(st[k][dst], st[k][src]), k
    # a pair the engine skips is skipped here too
    before = policy.priority.clone()
    policy.copy_envs(torch.tensor([3, B + 5]), torch.tensor([1, 2]), validate=False)
    assert torch.equal(policy.priority[1], before[3]) and torch.equal(policy.priority[[0, 2, 3, 4, 5]], before[[0, 2, 3, 4, 5]])
    E.close()
