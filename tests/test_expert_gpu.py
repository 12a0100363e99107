"""GPU: the shortest-path expert (VecPogema.expert_actions / pgx_expert_actions) equals the CPU reference
(tests/expert_reference.py) bit for bit -- distance and action -- on the small (<= 64 x 64) and the large-map layout,
after resets and after steps of every collision system and on_target mode; it leaves the engine state alone and can be
captured in a HIP graph."""
import numpy as np
import pytest

from expert_reference import expert_reference
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu


def _check(env, agents_as_obstacles, envs=None, what=""):
    """expert_actions() of every env (or of `envs`) == the reference on get_state() and the installed maps."""
    got_a, got_d = env.expert_actions(agents_as_obstacles=agents_as_obstacles)
    st = env.get_state()
    ref_a, ref_d = expert_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                                    st["is_active"].cpu().numpy(), agents_as_obstacles, envs=envs)
    got_a, got_d = got_a.cpu().numpy(), got_d.cpu().numpy()
    rows = slice(None) if envs is None else list(envs)
    bad = np.argwhere((got_d[rows] != ref_d[rows]) | (got_a[rows] != ref_a[rows]))
    assert bad.size == 0, (f"{what} flag={agents_as_obstacles}: {len(bad)} mismatches, first (row, agent) {bad[0].tolist()}: "
                           f"distance {got_d[rows][tuple(bad[0])]} vs {ref_d[rows][tuple(bad[0])]}, "
                           f"action {got_a[rows][tuple(bad[0])]} vs {ref_a[rows][tuple(bad[0])]}")
    return got_d


@pytest.mark.parametrize("size,batch,agents", [(2, 8, 1), (8, 16, 6), (31, 8, 12), (32, 8, 16), (33, 6, 12), (63, 4, 16),
                                               (64, 4, 16), (65, 3, 8), (100, 2, 6), (256, 1, 4)])
def test_square_maps_match_reference(size, batch, agents):
    from pogema_amd import GridConfig, VecPogema
    density = 0.0 if size == 2 else 0.3
    gc = GridConfig(size=size, num_agents=agents, obs_radius=3, density=density, seed=size, collision_system="soft",
                    max_episode_steps=256)
    env = VecPogema(gc, batch=batch)
    env.reset(seed=size)
    rng = np.random.default_rng(size)
    for flag in (False, True):
        _check(env, flag, what=f"size {size} reset")
    for _ in range(6):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    for flag in (False, True):
        _check(env, flag, what=f"size {size} after 6 steps")
    env.close()


def test_1024_map_few_agents():
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=1024, num_agents=2, obs_radius=2, density=0.3, seed=5, max_episode_steps=256)
    env = VecPogema(gc, batch=1)
    env.reset(seed=5)
    rng = np.random.default_rng(5)
    for flag in (False, True):
        _check(env, flag, what="1024 reset")
    for _ in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    for flag in (False, True):
        _check(env, flag, what="1024 after 3 steps")
    env.close()


MAPS = {
    "one_row": ".#.......#......",
    "wide": "\n".join("".join("#" if (x * 13 + y * 5) % 17 == 0 else "." for y in range(68)) for x in range(3)),
    "tall": "\n".join(("." * 5 if i % 7 else ".##..") for i in range(70)),
    "odd": "\n".join("".join("#" if (x * 7 + y * 3) % 11 == 0 else "." for y in range(40)) for x in range(13)),
}


@pytest.mark.parametrize("name", sorted(MAPS))
def test_map_strings_match_reference(name):
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(map=MAPS[name], num_agents=3, obs_radius=2, seed=3, collision_system="priority",
                    max_episode_steps=128)
    env = VecPogema(gc, batch=8)
    env.reset(seed=3)
    rng = np.random.default_rng(3)
    for t in range(8):
        if t % 4 == 0:
            for flag in (False, True):
                _check(env, flag, what=f"{name} step {t}")
        env.step(mixed_actions(env, rng, p_expert=0.7))
    env.close()


@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=12, num_agents=10, obs_radius=3, density=0.25, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=40)
    env = VecPogema(gc, batch=24, auto_reset=True)
    env.reset(seed=7)
    rng = np.random.default_rng(11)
    inactive_seen = False
    for t in range(16):
        if t % 3 == 0:
            for flag in (False, True):
                d = _check(env, flag, what=f"{collision}/{on_target} step {t}")
            inactive_seen |= bool((~env.get_state()["is_active"]).any())
        env.step(mixed_actions(env, rng, p_expert=0.85))
    if on_target == "finish":
        assert inactive_seen, "no finished (hidden) agent was ever checked"
    assert (d >= 0).any()
    env.close()


def test_empty_outside_false():
    from pogema_amd import GridConfig, VecPogema
    for size in (20, 70):
        gc = GridConfig(size=size, num_agents=6, obs_radius=4, density=0.3, seed=2, empty_outside=False,
                        max_episode_steps=64)
        env = VecPogema(gc, batch=4)
        env.reset(seed=2)
        rng = np.random.default_rng(2)
        for _ in range(2):
            for flag in (False, True):
                _check(env, flag, what=f"empty_outside=False size {size}")
            env.step(mixed_actions(env, rng, p_expert=0.7))
        env.close()


def test_configs2_full_batch():
    """BASELINE configs[2]: 8192 envs of 64 x 64 with 64 agents.  Sampled envs against the reference; the whole batch
    against what any shortest path must satisfy (grid graphs are bipartite: d >= Manhattan distance, same parity)."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=64, num_agents=64, obs_radius=5, density=0.3, seed=0)
    env = VecPogema(gc, batch=8192)
    env.reset(seed=0)
    rng = np.random.default_rng(0)
    sample = sorted(rng.choice(8192, size=6, replace=False).tolist()) + [0, 8191]
    st = env.get_state()
    ag, tg = st["agents_xy"].long(), st["targets_xy"].long()
    man = (ag - tg).abs().sum(-1)
    for flag in (False, True):
        d = torch.as_tensor(_check(env, flag, envs=sample, what="configs[2]"), device=env.device).long()
        a, _ = env.expert_actions(agents_as_obstacles=flag)
        reach = d >= 0
        assert bool(((d[reach] >= man[reach]) & ((d[reach] - man[reach]) % 2 == 0)).all())
        assert bool(((a == 0) == (d <= 0)).all())
        assert bool(((d == 0) == (man == 0)).all())
        if not flag:  # the generator places every start and target in one component
            assert bool(reach.all())
    env.close()


def test_dtypes_out_buffers_and_list_view():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    gc = GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21)
    env = VecPogema(gc, batch=6)
    env.reset(seed=21)
    a64, d64 = env.expert_actions()
    assert a64.dtype == torch.int64 and d64.dtype == torch.int32 and tuple(a64.shape) == (6, 5)
    for dt in (torch.int8, torch.int32):
        a, d = env.expert_actions(dtype=dt)
        assert a.dtype == dt and torch.equal(a.long(), a64) and torch.equal(d, d64)
    for dt in (torch.int8, torch.int32, torch.int64):
        oa = torch.full((6, 5), 99, dtype=dt, device=env.device)
        od = torch.full((6, 5), 99, dtype=torch.int32, device=env.device)
        ra, rd = env.expert_actions(out=(oa, od))
        assert ra is oa and rd is od
        assert torch.equal(oa.long(), a64) and torch.equal(od, d64)
    with pytest.raises(ValueError):
        env.expert_actions(out=(torch.empty((6, 5), dtype=torch.float32, device=env.device), od))
    with pytest.raises(ValueError):
        env.expert_actions(out=(oa, torch.empty((6, 4), dtype=torch.int32, device=env.device)))
    with pytest.raises(ValueError):
        env.expert_actions(dtype=torch.float32)
    with pytest.raises(ValueError):
        env.expert_actions(out=(oa, None))
    env.close()

    one = pogema_v0(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21))
    one.reset(seed=21)
    acts = one.expert_actions()
    assert isinstance(acts, list) and len(acts) == 5 and all(isinstance(x, int) for x in acts)
    va, _ = one._vec.expert_actions()
    assert acts == va[0].cpu().tolist()
    one.step(one.expert_actions(agents_as_obstacles=True))
    one.close()


def test_expert_before_reset_is_refused():
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=8, num_agents=2, obs_radius=2, seed=1), batch=2)
    with pytest.raises(PgxError) as ei:
        env.expert_actions()
    assert ei.value.code == -4  # PGX_E_STATE, as pgx_step before a reset
    env.close()


@pytest.mark.parametrize("size", [24, 80])
def test_single_agent_follows_expert_to_its_target(size):
    from pogema_amd import GridConfig, pogema_v0
    gc = GridConfig(size=size, num_agents=1, obs_radius=3, density=0.3, seed=17, on_target="finish",
                    max_episode_steps=4 * size * size)
    env = pogema_v0(gc)
    env.reset(seed=17)
    _, dist = env._vec.expert_actions()
    d = int(dist[0, 0])
    assert d > 0
    for t in range(1, d + 1):
        _, _, term, trunc, _ = env.step(env.expert_actions())
        assert term[0] == (t == d) and not trunc[0], f"step {t} of {d}"
    env.close()


def test_state_untouched():
    """get_state() and the next step()'s outputs are identical with and without a preceding expert_actions()."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    for size, coll in ((20, "soft"), (90, "block_both")):
        gc = GridConfig(size=size, num_agents=12, obs_radius=3, density=0.3, seed=31, collision_system=coll,
                        max_episode_steps=32)
        a = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
        b = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
        a.reset(seed=31)
        b.reset(seed=31)
        rng = np.random.default_rng(31)
        for t in range(6):
            acts = torch.as_tensor(rng.integers(0, 5, size=(8, 12)), device=a.device)
            a.expert_actions()
            a.expert_actions(agents_as_obstacles=True)
            sa, sb = a.get_state(occupancy=True), b.get_state(occupancy=True)
            for k in sa:
                assert torch.equal(sa[k], sb[k]), f"size {size} step {t}: {k}"
            assert np.array_equal(installed_maps(a), installed_maps(b))
            ra, rb = a.step(acts), b.step(acts)
            for x, y in zip(ra[:4], rb[:4]):
                assert torch.equal(x, y), f"size {size} step {t}"
            assert torch.equal(ra[4]["is_active"], rb[4]["is_active"])
        a.close()
        b.close()


@pytest.mark.parametrize("size", [16, 72])
def test_expert_then_step_in_hip_graph(size):
    """expert_actions() -> step(those actions) captured once in a HIP graph; replays equal the eager run of a twin."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A = 32, 8
    gc = GridConfig(size=size, num_agents=A, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                    max_episode_steps=24)
    eager = VecPogema(gc, batch=B, auto_reset=True)
    graphed = VecPogema(gc, batch=B, auto_reset=True)
    eager.reset(seed=4)
    graphed.reset(seed=4)
    acts = torch.zeros((B, A), dtype=torch.int64, device="cuda")
    dist = torch.zeros((B, A), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch's graph recipe asks
        graphed.expert_actions(agents_as_obstacles=True, out=(acts, dist))
        graphed.step(acts)
    torch.cuda.current_stream().wait_stream(side)
    ea, _ = eager.expert_actions(agents_as_obstacles=True)
    eager.step(ea)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.expert_actions(agents_as_obstacles=True, out=(acts, dist))
        out = graphed.step(acts)
    for t in range(30):
        g.replay()
        ea, ed = eager.expert_actions(agents_as_obstacles=True)
        ref = eager.step(ea)
        assert torch.equal(acts, ea) and torch.equal(dist, ed), f"step {t}"
        for x, y in zip(out[:4], ref[:4]):
            assert torch.equal(x, y), f"step {t}"
    se, sg = eager.get_state(), graphed.get_state()
    for k in se:
        assert torch.equal(se[k], sg[k])
    eager.close()
    graphed.close()


def test_lds_limit_is_only_raised_across_live_handles():
    """The dynamic-LDS opt-in belongs to the kernel function, shared by every handle: creating a small large-layout env
    after a 1024-side one must not lower it below what the first one launches with."""
    from pogema_amd import GridConfig, VecPogema
    big = VecPogema(GridConfig(size=1024, num_agents=2, obs_radius=2, density=0.3, seed=8, max_episode_steps=64), batch=1)
    big.reset(seed=8)
    small = VecPogema(GridConfig(size=65, num_agents=4, obs_radius=2, density=0.3, seed=8), batch=2)
    small.reset(seed=8)
    for flag in (False, True):
        _check(big, flag, what="1024 after a 65-side handle was created")
        _check(small, flag, what="65 next to a 1024-side handle")
    small.close()
    big.close()


def test_large_map_staged_with_deep_staging():
    """1024 x 600: 19 words per row, 19456 in all -- the free bitmap is staged in LDS and each thread stages 32 words of
    the visited set per iteration (the layout between 256 x 256 and 1024 x 1024)."""
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(600)
    grid = (rng.random((1024, 600)) < 0.25).astype(int).tolist()
    env = VecPogema(GridConfig(map=grid, num_agents=2, obs_radius=2, seed=6, max_episode_steps=64), batch=1)
    env.reset(seed=6)
    for flag in (False, True):
        _check(env, flag, what="1024 x 600")
    env.close()


def test_more_searches_than_one_launch_grid():
    """The large layout's workgroups loop over the (env, agent) slots once there are more than 2^20 of them."""
    from pogema_amd import GridConfig, VecPogema
    B, A = 16400, 64                       # 1 049 600 slots > 2^20
    env = VecPogema(GridConfig(size=65, num_agents=A, obs_radius=2, density=0.3, seed=9, max_episode_steps=64), batch=B)
    env.reset(seed=9)
    for flag in (False, True):
        _check(env, flag, envs=[0, 8191, B - 2, B - 1], what="2^20+ slots")
    env.close()


def test_first_flagged_call_on_a_large_map_is_refused_inside_capture():
    """The large layout's occupancy scratch is allocated by the first call with agents_as_obstacles; inside a graph
    capture that call is refused with a named error instead of allocating, and works eagerly afterwards."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=70, num_agents=4, obs_radius=2, density=0.3, seed=12), batch=4)
    env.reset(seed=12)
    acts = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
    dist = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    env.expert_actions(out=(acts, dist))  # without the flag: no scratch needed
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError, match="outside graph capture") as ei:
        with torch.cuda.graph(g):
            env.expert_actions(agents_as_obstacles=True, out=(acts, dist))
    assert ei.value.code == -4
    torch.cuda.synchronize()
    for flag in (True, False):
        _check(env, flag, what="after the refused capture")
    env.close()
