"""GPU: plan repair (VecPogema.repair_plan / pgx_repair_plan, docs/SPEC.md S29) equals the CPU reference
(tests/repair_plan_reference.py) applied to get_state() and the installed maps, bit for bit on all five outputs: every
lane layout, both ends of the horizon's range, kept agents inside and outside the replanned agents' reach, non-square and
large maps, every collision system and on_target mode, the hand-built cases; given paths from whca_plan() and
pibt_plan(), stale ones and corrupted ones.  Everybody replanned is whca_plan() itself, a plan repaired for the tail of
its own service order is that plan again.  The call keeps whca_plan()'s contract -- state untouched, one cache refresh per
call, capturable after one eager call -- and its result passes path_conflicts() and is what rollout(actions) does."""
import numpy as np
import pytest

from repair_plan_cases import CASES, NAMES, active, expected, given, grid
from repair_plan_reference import repair_reference
from test_repair_plan import corrupt, tail_mask
from test_visible_agents_gpu import LAYOUTS
from util import generate_instances, installed_maps, lazy_torch, mixed_actions
from whca_reference import conflicts, whca_reference

pytestmark = pytest.mark.gpu


def _dev(env, array, dtype):
    torch = lazy_torch()
    return torch.as_tensor(np.ascontiguousarray(array), dtype=dtype, device=env.device)


def _check(env, paths, replan, priority, on_target, what="", dtype=None, out=None):
    """repair_plan(paths, replan, priority) == the reference on get_state() + the installed maps; returns (the five
    output tensors, the reference's arrays).  `paths` is copied first: `out` may hold it."""
    torch = lazy_torch()
    K, B, A = paths.shape[0], env.batch, env.num_agents
    given_np = paths.cpu().numpy().copy()
    kw = {} if dtype is None else {"dtype": dtype}
    got = env.repair_plan(paths, replan=replan, priority=priority, out=out, **kw)
    if out is None:
        assert got[0].dtype == (torch.int64 if dtype is None else dtype)
    assert tuple(got[0].shape) == (K, B, A)
    assert got[1].dtype == torch.int32 and tuple(got[1].shape) == (K, B, A, 2)
    for t in got[2:]:
        assert t.dtype == torch.int32 and tuple(t.shape) == (B, A)
    st = env.get_state()
    want = repair_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                            st["is_active"].cpu().numpy(), given_np, None if replan is None else replan.cpu().numpy(),
                            None if priority is None else priority.cpu().numpy(), on_target=on_target)
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy().astype(w.dtype)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: "
                               f"{g[tuple(bad[0])]} vs {w[tuple(bad[0])]}")
    return got, want


def _random_priority(env, rng, low=-3, high=4):
    torch = lazy_torch()
    return torch.as_tensor(rng.integers(low, high, size=(env.batch, env.num_agents)), dtype=torch.int32, device=env.device)


def _random_mask(env, rng, share=0.5, dtype=None):
    torch = lazy_torch()
    return _dev(env, rng.random((env.batch, env.num_agents)) < share, dtype or torch.bool)


def _corrupted(env, path_xy, rng):
    torch = lazy_torch()
    return _dev(env, corrupt(path_xy.cpu().numpy(), rng)[0], torch.int32)


def _mix(env, K, on_target, rng, what, steps=True):
    """The given paths of the random rows, each against the reference: whca_plan()'s output under other priorities and
    a random mask, with a tenth of the agents corrupted; pibt_plan()'s output; and a stale plan -- plan, two steps, then
    the plan from its third step on, padded with its last one."""
    torch = lazy_torch()
    plan = env.whca_plan(K, priority=_random_priority(env, rng))[1]
    _, want = _check(env, _corrupted(env, plan, rng), _random_mask(env, rng), _random_priority(env, rng), on_target,
                     f"{what}: whca_plan's paths, corrupted")
    seen = {"kept": int(((want[4] == 0) & (want[5] >= 0)).sum()), "replanned": int(want[4].sum()),
            "unasked": 0}
    plan = env.pibt_plan(min(K, 31))[1]
    _, want = _check(env, plan, _random_mask(env, rng, 0.2, torch.uint8), None, on_target, f"{what}: pibt_plan's paths")
    seen["kept"] += int(((want[4] == 0) & (want[5] >= 0)).sum())
    if steps:
        plan = env.whca_plan(K)[1]
        for _ in range(2):
            env.step(mixed_actions(env, rng, p_expert=0.7))
        stale = torch.cat([plan[2:], plan[-1:].expand(min(2, K), -1, -1, -1)])[:K].contiguous()
        _, want = _check(env, _corrupted(env, stale, rng), None, _random_priority(env, rng), on_target, f"{what}: a stale plan")
        seen["unasked"] = int(want[4].sum())
        seen["kept"] += int(((want[4] == 0) & (want[5] >= 0)).sum())
    return seen


@pytest.mark.parametrize("agents,size,batch", LAYOUTS)
def test_every_lane_layout_matches_reference(agents, size, batch):
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(agents)
    batch = min(batch, 24)   # the reference is a Python search per replanned agent
    K = 6 if agents < 1024 else 3
    gc = GridConfig(size=size, num_agents=agents, obs_radius=1 + agents % 5, density=0.1, seed=agents,
                    collision_system="soft", on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=batch)
    env.reset(seed=agents)
    seen = _mix(env, K, "finish", rng, f"A={agents}")
    assert seen["kept"] > 0 and seen["replanned"] > 0
    env.close()


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_both_ends_of_the_horizon(on_target):
    """K = 1, and K = 31 on a 12 x 12 map: the 63 x 63 box is larger than the map on every side."""
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=12, num_agents=8, obs_radius=2, density=0.3, seed=6, collision_system="soft",
                               on_target=on_target), batch=6)
    env.reset(seed=6)
    rng = np.random.default_rng(6)
    _mix(env, 1, on_target, rng, "K=1", steps=False)
    seen = _mix(env, 31, on_target, rng, "K=31")
    assert seen["kept"] > 0 and seen["replanned"] > 0 and seen["unasked"] > 0
    env.close()


def test_longest_horizon_inside_a_large_map():
    """K = 31 on 80 x 80 with agents in the corners and on the borders: a replanned agent's box is clipped by one or two
    edges of the map, and kept agents start both within its reach (Chebyshev distance 2K) and beyond it."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A, size, K = 2, 10, 80, 31
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
    plan = env.whca_plan(K)[1]
    mask = np.zeros((B, A), dtype=bool)
    mask[:, [0, 3, 4, 7]] = True             # two opposite corners, a border cell and an agent somewhere inside
    d = np.abs(agents[:, :, None, :] - agents[:, None, :, :]).max(axis=-1)       # [B, replanned, kept]
    pairs = mask[:, :, None] & ~mask[:, None, :]
    assert (d[pairs] <= 2 * K).any() and (d[pairs] > 2 * K).any()
    prio = _random_priority(env, np.random.default_rng(8))
    _check(env, plan, _dev(env, mask, torch.bool), prio, "nothing", what="80x80 K=31")
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
    _mix(env, 9, "nothing", rng, name)
    env.close()


@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    """Finished (hidden) agents and lifelong retargets precede the call.  Under `soft` the envs start with agents that
    share a cell; that state is repaired as well, before the steps: only the bit-exactness is asserted there."""
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
    if collision == "soft":
        _mix(env, 7, on_target, rng, f"soft/{on_target} shared cells", steps=False)
    for t in range(30):      # a few mixed steps; under finish until an agent is hidden
        env.step(mixed_actions(env, rng, p_expert=0.6))
        if t >= 3 and (on_target != "finish" or not bool(env.get_state()["is_active"].all())):
            break
    if on_target == "finish":
        assert not bool(env.get_state()["is_active"].all()), "no finished (hidden) agent"
    _mix(env, 7, on_target, rng, f"{collision}/{on_target}")
    env.close()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_cases(case):
    from pogema_amd import GridConfig, VecPogema
    torch = lazy_torch()
    A, B = len(case["agents"]), 3
    env = VecPogema(GridConfig(map="\n".join(case["map"]), num_agents=A, obs_radius=2, seed=1, collision_system="soft",
                               on_target=case["on_target"]), batch=B, auto_reset=False)
    start = case.get("start", {"agents": case["agents"]})
    env.reset_from_state(grid(case["map"]), np.array(start["agents"], dtype=np.int32), np.array(case["targets"], dtype=np.int32),
                         validate=False)
    if "step" in start:
        env.step(_dev(env, [start["step"]] * B, torch.int64))
    st = env.get_state()
    assert np.array_equal(st["agents_xy"].cpu().numpy(), np.array([case["agents"]] * B))
    assert np.array_equal(st["is_active"].cpu().numpy().astype(bool), np.array([active(case)] * B))
    paths = _dev(env, np.repeat(given(case)[:, None], B, 1), torch.int32)
    replan = None if case["replan"] is None else _dev(env, [case["replan"]] * B, torch.uint8)
    prio = None if case["priority"] is None else _dev(env, [case["priority"]] * B, torch.int32)
    got = env.repair_plan(paths, replan=replan, priority=prio)
    for name, g, w in zip(NAMES, got, expected(case)):
        w = np.repeat(w[:, None], B, 1) if name in ("actions", "path_xy") else np.repeat(w[None], B, 0)
        assert np.array_equal(g.cpu().numpy().astype(w.dtype), w), f"{case['name']}: {name}"
    env.close()


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_equivalence_with_whca_plan(on_target):
    """Property 1 against whca_plan() itself; property 2 for the last m agents of its service order; property 3."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A, K = 12, 24, 12
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                               on_target=on_target), batch=B)
    env.reset(seed=4)
    rng = np.random.default_rng(4)
    prio = _random_priority(env, rng)
    plan = env.whca_plan(K, priority=prio)
    assert int(plan[3].sum()) > 0, "no failed agent in the plan"
    junk = _dev(env, rng.integers(-2 ** 31, 2 ** 31, size=(K, B, A, 2)), torch.int32)
    ones = torch.ones((B, A), dtype=torch.bool, device=env.device)
    for paths, replan in ((junk, ones), (plan[1], ones), (junk, None)):
        got = env.repair_plan(paths, replan=replan, priority=prio)
        assert all(torch.equal(g, w) for g, w in zip(got[:4], plan))
        assert torch.equal(got[4], env.get_state()["is_active"].to(torch.int32))
    act = env.get_state()["is_active"].cpu().numpy().astype(bool)
    for m in (0, 1, A // 2, A, None):
        asked = np.zeros((B, A), dtype=bool) if m is None else tail_mask(act, prio.cpu().numpy(), m)
        replan = None if m is None else _dev(env, asked, torch.bool)
        got = env.repair_plan(plan[1], replan=replan, priority=prio)
        asked = _dev(env, asked, torch.int32)
        assert all(torch.equal(g, w) for g, w in zip(got[:3], plan[:3])), m
        assert torch.equal(got[3], plan[3] * asked) and torch.equal(got[4], asked), m
    env.close()


def test_action_dtypes_priorities_out_and_refusals():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A, K = 9, 14, 8
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.3, seed=9, collision_system="soft",
                               on_target="nothing"), batch=B)
    env.reset(seed=9)
    rng = np.random.default_rng(9)
    dev = env.device
    prio = _random_priority(env, rng)
    paths = _corrupted(env, env.whca_plan(K)[1], rng)
    replan = _random_mask(env, rng)
    base, _ = _check(env, paths, replan, prio, "nothing", what="base")
    for dtype in (torch.int8, torch.int32, torch.int64):
        got, _ = _check(env, paths, replan, prio, "nothing", what=str(dtype), dtype=dtype)
        assert torch.equal(got[0].to(torch.int64), base[0]) and all(torch.equal(g, b) for g, b in zip(got[1:], base[1:]))
        assert torch.equal(env.repair_plan(paths, replan.to(torch.uint8), prio.to(torch.int64), dtype=dtype)[0], got[0])
    make = lambda: [torch.full((K, B, A), 99, dtype=torch.int32, device=dev), torch.full((K, B, A, 2), 99, dtype=torch.int32, device=dev),
                    *(torch.full((B, A), 99, dtype=torch.int32, device=dev) for _ in range(3))]
    out = make()
    got, _ = _check(env, paths, replan, prio, "nothing", what="out=", out=tuple(out))
    assert all(g is o for g, o in zip(got, out))
    # in place: out[path_xy] is `paths`
    out = make()
    out[1] = paths.clone()
    got, _ = _check(env, out[1], replan, prio, "nothing", what="in place", out=tuple(out))
    assert got[1] is out[1] and all(torch.equal(g.to(torch.int64), b.to(torch.int64)) for g, b in zip(got, base))

    bad = {0: [torch.empty((K, B, A), dtype=torch.float32, device=dev), torch.empty((K + 1, B, A), dtype=torch.int32, device=dev),
               torch.empty((K, B, A), dtype=torch.int32)],
           1: [torch.empty((K, B, A, 2), dtype=torch.int64, device=dev), torch.empty((B, A, 2), dtype=torch.int32, device=dev)],
           2: [torch.empty((B, A), dtype=torch.int64, device=dev), torch.empty((B, A + 1), dtype=torch.int32, device=dev)],
           3: [torch.empty((B, 2 * A), dtype=torch.int32, device=dev)[:, ::2], None],
           4: [torch.empty((B, A), dtype=torch.uint8, device=dev), paths.view(-1)[:B * A].view(B, A),
               paths.view(-1)[-B * A:].view(B, A)]}
    for k, tensors in bad.items():
        for t in tensors:
            o = make()
            o[k] = t
            with pytest.raises(ValueError, match="out"):
                env.repair_plan(paths, out=tuple(o))
    with pytest.raises(ValueError, match="out must be"):
        env.repair_plan(paths, out=tuple(make()[:4]))
    big = torch.zeros(2 * paths.numel(), dtype=torch.int32, device=dev)
    inside = big[:paths.numel()].view(K, B, A, 2)
    o = make()
    o[1] = big[2:2 + paths.numel()].view(K, B, A, 2)
    with pytest.raises(ValueError, match=r"out\[path_xy\] overlaps paths"):
        env.repair_plan(inside, out=tuple(o))
    for wrong in (paths.to(torch.int64), paths.cpu().numpy(), None):
        with pytest.raises(TypeError, match="paths must be an int32"):
            env.repair_plan(wrong)
    for wrong in (paths[0], paths[:, :-1], paths.cpu(), torch.zeros((32, B, A, 2), dtype=torch.int32, device=dev),
                  torch.zeros((0, B, A, 2), dtype=torch.int32, device=dev),
                  torch.zeros((K, B, A, 4), dtype=torch.int32, device=dev)[..., ::2]):
        with pytest.raises(ValueError, match="paths must be .*got shape"):
            env.repair_plan(wrong)
    for wrong in (replan.to(torch.int32), replan.to(torch.float32), replan.cpu().numpy()):
        with pytest.raises(TypeError, match="replan must be a bool or uint8"):
            env.repair_plan(paths, replan=wrong)
    for wrong in (replan[:, :-1], replan.cpu(), torch.zeros((A, B), dtype=torch.bool, device=dev).t()):
        with pytest.raises(ValueError, match="replan must be"):
            env.repair_plan(paths, replan=wrong)

    # through the C-ABI: PGX_E_INVALID, nothing is launched; replan, priority and four outputs may be NULL
    from pogema_amd import _lib
    call, h, s = env._lib.pgx_repair_plan, env._handle, env._stream()
    acts = torch.full((K * B * A + 64,), 77, dtype=torch.int32, device=dev)
    a, p, u8 = acts[32:].data_ptr(), paths.data_ptr(), replan.data_ptr()
    refused = {
        "paths": (h, 0, K, None, u8, None, a, 1, None, None, None, None, s),
        "actions": (h, 0, K, p, u8, None, None, 1, None, None, None, None, s),
        "horizon 0": (h, 0, 0, p, u8, None, a, 1, None, None, None, None, s),
        "horizon 32": (h, 0, 32, p, u8, None, a, 1, None, None, None, None, s),
        "flags": (h, 1, K, p, u8, None, a, 1, None, None, None, None, s),
        "action_dtype": (h, 0, K, p, u8, None, a, 3, None, None, None, None, s),
        "paths ": (h, 0, K, p + 2, u8, None, a, 1, None, None, None, None, s),
        "actions ": (h, 0, K, p, u8, None, a + 2, 1, None, None, None, None, s),
        "priority": (h, 0, K, p, u8, prio.data_ptr() + 1, a, 1, None, None, None, None, s),
        "path_xy": (h, 0, K, p, u8, None, a, 1, p + 2, None, None, None, s),
        "arrival": (h, 0, K, p, u8, None, a, 1, None, a + 1, None, None, s),
        "failed": (h, 0, K, p, u8, None, a, 1, None, None, a + 2, None, s),
        "replanned": (h, 0, K, p, u8, None, a, 1, None, None, None, a + 3, s),
    }
    for name, args in refused.items():
        assert call(*args) == -1, name
        msg = env._lib.pgx_last_error().decode()
        assert "pgx_repair_plan" in msg and name.split()[0] in msg, (name, msg)
    assert call(h, 0, K, p, u8, prio.data_ptr(), a, 1, None, None, None, None, s) == 0
    assert torch.equal(acts[32:32 + K * B * A].view(K, B, A).to(torch.int64), base[0])
    assert bool((acts[:32] == 77).all()) and bool((acts[32 + K * B * A:] == 77).all())
    assert call(h, 0, K, p, None, None, a, 1, None, None, None, None, s) == 0
    assert torch.equal(acts[32:32 + K * B * A].view(K, B, A).to(torch.int64), env.repair_plan(paths)[0])
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
    junk = torch.full((7, 8, 12, 2), -1, dtype=torch.int32, device=env.device)
    first = env.repair_plan(junk)                             # allocates the cache: one field per active agent
    n = env.cost_to_go_builds
    assert n == 8 * 12, n
    again = env.repair_plan(first[1], replan=torch.ones((8, 12), dtype=torch.uint8, device=env.device),
                            priority=torch.zeros((8, 12), dtype=torch.int64, device=env.device))
    env.repair_plan(first[1])
    env.whca_plan(31)
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
    dev = env.device
    prio = torch.zeros((B, A), dtype=torch.int32, device=dev)
    paths = torch.zeros((K, B, A, 2), dtype=torch.int32, device=dev)
    replan = torch.zeros((B, A), dtype=torch.bool, device=dev)
    out = (torch.zeros((K, B, A), dtype=torch.int64, device=dev), torch.zeros((K, B, A, 2), dtype=torch.int32, device=dev),
           *(torch.zeros((B, A), dtype=torch.int32, device=dev) for _ in range(3)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step(torch.zeros((B, A), dtype=torch.int64, device=dev))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError) as ei:
        with torch.cuda.graph(g):
            env.repair_plan(paths, replan=replan, priority=prio, out=out)
    assert ei.value.code == -4 and "capture" in str(ei.value) and "pgx_repair_plan" in str(ei.value)
    torch.cuda.synchronize()
    env.repair_plan(paths, replan=replan, priority=prio, out=out)     # the eager call that allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.repair_plan(paths, replan=replan, priority=prio, out=out)
    rng = np.random.default_rng(4)
    for t in range(3):
        env.step(out[0][0].clone() if t % 2 else mixed_actions(env, rng, p_expert=0.8))   # the state changes
        prio.copy_(torch.as_tensor(rng.integers(-2, 3, size=(B, A)), dtype=torch.int32))
        paths.copy_(_corrupted(env, env.pibt_plan(K)[1], rng))                             # ... and the given paths
        replan.copy_(_random_mask(env, rng, 0.3))
        g.replay()
        got = [o.clone() for o in out]
        want, _ = _check(env, paths, replan, prio, "restart", what=f"replay {t}")
        assert all(torch.equal(x, y) for x, y in zip(got, want)), f"replay {t}"
    env.close()


def test_refused_before_reset_and_list_view():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=10, num_agents=9, obs_radius=3, density=0.1, seed=21, collision_system="soft"), batch=6)
    with pytest.raises(PgxError) as ei:
        env.repair_plan(torch.zeros((3, 6, 9, 2), dtype=torch.int32, device=env.device))
    assert ei.value.code == -4 and "pgx_repair_plan" in str(ei.value)       # PGX_E_STATE before a reset
    env.close()
    from pogema_amd import PipelinedVecPogema
    assert not hasattr(PipelinedVecPogema, "repair_plan") and not hasattr(PipelinedVecPogema, "whca_plan")

    one = pogema_v0(GridConfig(size=8, num_agents=10, obs_radius=3, density=0.0, seed=21, collision_system="soft"))
    one.reset(seed=21)
    given_paths = one._vec.whca_plan(4)[1][:, 0].cpu().numpy().tolist()
    plan = one.repair_plan(given_paths)
    assert isinstance(plan, list) and len(plan) == 4 and all(len(row) == 10 and all(isinstance(a, int) for a in row) for row in plan)
    assert plan == one.whca_plan(4)
    mask = [i % 2 == 0 for i in range(10)]
    again = one.repair_plan(given_paths, replan=mask, priority=list(range(10)))
    vec = one._vec
    want = vec.repair_plan(torch.as_tensor([given_paths], dtype=torch.int32, device=vec.device).transpose(0, 1).contiguous(),
                           replan=torch.as_tensor([mask], device=vec.device),
                           priority=torch.arange(10, device=vec.device)[None])[0]
    assert again == want[:, 0].cpu().numpy().tolist()
    for row in again:
        one.step(row)
    one.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------
E2E = dict(size=16, agents=16, batch=48, K=16, seed=4)


def test_repair_passes_path_conflicts_and_is_what_rollout_does():
    """soft / finish: whca_plan(K)'s plan, a seeded random half of the agents replanned under random priorities.  Kept rows
    are unchanged; in the envs where neither the given plan nor the repair has a failed agent the result has no vertex
    and no edge conflict by path_conflicts()' own count, and rollout(actions) walks it: every agent still active afterwards
    stands on path_xy[K - 1], every agent with arrival >= 1 has finished."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    c = E2E
    K, B, A = c["K"], c["batch"], c["agents"]
    obstacles, agents, targets = generate_instances(B, c["size"], c["size"], A, 0.3, c["seed"])
    rng = np.random.default_rng(c["seed"])
    mask = np.zeros((B, A), dtype=bool)
    for b in range(B):
        mask[b, rng.permutation(A)[:A // 2]] = True
    prio = rng.integers(-3, 4, size=(B, A))
    everyone = np.ones((B, A), dtype=bool)
    # the seed was chosen with the references alone: at most a quarter of the envs hold a failed agent
    plan = whca_reference(obstacles, agents, targets, everyone, K, None, "finish")
    ref = repair_reference(obstacles, agents, targets, everyone, plan[1], mask, prio, "finish")
    ref_left_out = int(((plan[3].sum(axis=1) > 0) | (ref[3].sum(axis=1) > 0)).sum())
    assert 4 * ref_left_out <= B, ref_left_out

    gc = GridConfig(map=obstacles[0].tolist(), num_agents=A, obs_radius=3, seed=c["seed"], collision_system="soft",
                    on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=B, auto_reset=False)
    env.reset_from_state(obstacles, agents, targets)
    given_actions, given_path, _, given_failed = env.whca_plan(K)
    assert np.array_equal(given_path.cpu().numpy(), plan[1])
    replan = _dev(env, mask, torch.bool)
    actions, path_xy, arrival, failed, replanned = env.repair_plan(given_path, replan=replan, priority=_dev(env, prio, torch.int32))
    for name, g, w in zip(NAMES, (actions, path_xy, arrival, failed, replanned), ref):
        assert np.array_equal(g.cpu().numpy().astype(w.dtype), w), name
    assert torch.equal(replanned, replan.to(torch.int32))
    assert torch.equal(path_xy[:, ~replan], given_path[:, ~replan]) and torch.equal(actions[:, ~replan], given_actions[:, ~replan])
    clean = (failed.sum(dim=1) == 0) & (given_failed.sum(dim=1) == 0)
    left_out = B - int(clean.sum())
    print(f"repair end to end: {left_out} of {B} envs left out for holding a failed agent")
    assert 4 * left_out <= B, left_out
    count = env.path_conflicts(path_xy, kinds=("vertex", "edge"))[3]
    assert int(count[clean].sum()) == 0
    assert not torch.equal(path_xy, given_path), "the repair changed nothing"

    env.rollout(actions, obs_slots=0)
    st = env.get_state()
    on = st["is_active"] & clean.view(-1, 1)
    assert bool(on.any())
    assert torch.equal(st["agents_xy"][on], path_xy[K - 1][on])
    assert not bool((st["is_active"] & (arrival >= 1) & clean.view(-1, 1)).any())
    env.close()
