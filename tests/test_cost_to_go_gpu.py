"""GPU: cost-to-go windows (VecPogema.cost_to_go / pgx_cost_to_go, docs/SPEC.md S11) equal the CPU reference
(tests/cost_to_go_reference.py) bit for bit on get_state() and the installed maps -- both build layouts, 2- and 4-byte
fields, every collision system and on_target mode -- the field cache rebuilds exactly what its contract says, the engine
state is left alone, and a graph replay equals the eager run."""
import numpy as np
import pytest

from cost_to_go_reference import cost_to_go_reference
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu


def _check(env, envs=None, what=""):
    """cost_to_go() of every env (or of `envs`) == the reference; centres == expert distance; inactive agents all -1."""
    got = env.cost_to_go().cpu().numpy()
    st = env.get_state()
    active = st["is_active"].cpu().numpy()
    r = env.obs_radius
    ref = cost_to_go_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(), active, r,
                               envs=envs)
    rows = slice(None) if envs is None else list(envs)
    bad = np.argwhere(got[rows] != ref[rows])
    assert bad.size == 0, (f"{what}: {len(bad)} mismatches, first (row, agent, u, v) {bad[0].tolist()}: "
                           f"{got[rows][tuple(bad[0])]} vs {ref[rows][tuple(bad[0])]}")
    _, dist = env.expert_actions()
    dist = dist.cpu().numpy()
    assert np.array_equal(got[rows][..., r, r][active[rows]], dist[rows][active[rows]]), what
    assert (got[rows][~active[rows]] == -1).all(), what
    return got


class CacheModel:
    """Host model of the cache contract: which fields a call must build."""

    def __init__(self):
        self.maps = self.tags = self.fresh = None

    def call(self, env):
        st = env.get_state()
        maps = installed_maps(env)
        tgt = st["targets_xy"].cpu().numpy()
        active = st["is_active"].cpu().numpy()
        if self.maps is None:
            self.maps = maps.copy()
            self.tags = np.full(tgt.shape, -1, dtype=np.int64)
            self.fresh = np.zeros(active.shape, dtype=bool)   # the slot holds a field
        self.fresh[(self.maps != maps).reshape(maps.shape[0], -1).any(1)] = False
        self.maps = maps.copy()
        stale = active & (~self.fresh | (self.tags != tgt).any(-1))
        self.tags[stale] = tgt[stale]
        self.fresh |= stale
        return int(stale.sum())


def _call_and_count(env, model):
    before = env.cost_to_go_builds
    env.cost_to_go()
    return env.cost_to_go_builds - before, model.call(env)


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
    _check(env, what=f"size {size} reset")
    for _ in range(6):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, what=f"size {size} after 6 steps")
    env.close()


@pytest.mark.parametrize("H,W,agents", [(257, 256, 3), (1024, 600, 2), (1024, 1024, 2), (40, 130, 5), (130, 40, 5)])
def test_rectangular_and_large_maps(H, W, agents):
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(H * 7 + W)
    grid = (rng.random((H, W)) < 0.25).astype(int).tolist()
    env = VecPogema(GridConfig(map=grid, num_agents=agents, obs_radius=2, seed=6, max_episode_steps=64), batch=1)
    env.reset(seed=6)
    _check(env, what=f"{H} x {W} reset")
    for _ in range(2):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, what=f"{H} x {W} after steps")
    env.close()


@pytest.mark.parametrize("radius", [1, 5, 15])
def test_obs_radius(radius):
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=40, num_agents=12, obs_radius=radius, density=0.3, seed=radius, max_episode_steps=64)
    env = VecPogema(gc, batch=6)
    env.reset(seed=radius)
    rng = np.random.default_rng(radius)
    _check(env, what=f"radius {radius}")
    for _ in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, what=f"radius {radius} after steps")
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
            _check(env, what=f"{collision}/{on_target} step {t}")
            inactive_seen |= bool((~env.get_state()["is_active"]).any())
        env.step(mixed_actions(env, rng, p_expert=0.85))
    if on_target == "finish":
        assert inactive_seen, "no finished (hidden) agent was ever checked"
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
            _check(env, what=f"empty_outside=False size {size}")
            env.step(mixed_actions(env, rng, p_expert=0.7))
        env.close()


def _serpentine(H, W):
    """One-cell corridors: every even row free, odd rows walls with one gap at alternating ends."""
    m = np.ones((H, W), dtype=np.uint8)
    m[0::2] = 0
    for x in range(1, H, 2):
        m[x, W - 1 if (x // 2) % 2 == 0 else 0] = 0
    return m


@pytest.mark.parametrize("H,W,floor", [(256, 256, 32767), (1024, 600, 65535)])
def test_serpentine_long_distances(H, W, floor):
    """Distances above 32767 on the 2-byte path (sign bugs) and above 65535 on the 4-byte path."""
    from pogema_amd import GridConfig, VecPogema
    m = _serpentine(H, W)
    last = H - 1 if H % 2 else H - 2
    end_col = W - 1 if (last // 2) % 2 == 0 else 0
    agents = np.array([[0, 0], [last, end_col], [H // 2 if (H // 2) % 2 == 0 else H // 2 + 1, W // 2]], dtype=np.int32)
    targets = np.array([[last, end_col], [0, 0], [0, W - 1]], dtype=np.int32)
    env = VecPogema(GridConfig(map=m.tolist(), num_agents=3, obs_radius=3, seed=1, max_episode_steps=64), batch=1)
    env.reset_from_state(m[None], agents[None], targets[None])
    got = _check(env, what=f"serpentine {H} x {W}")
    assert got[0, 0, 3, 3] > floor and got[0, 1, 3, 3] > floor
    assert got.max() > floor
    env.close()


def test_configs1_full_batch():
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=16, num_agents=8, obs_radius=5, density=0.3, seed=0), batch=1024)
    env.reset(seed=0)
    _check(env, what="configs[1]")
    env.close()


def test_configs2_sample():
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=64, num_agents=64, obs_radius=5, density=0.3, seed=0), batch=8192)
    env.reset(seed=0)
    rng = np.random.default_rng(0)
    sample = sorted(set(rng.choice(8192, size=256, replace=False).tolist()) | {0, 8191})
    _check(env, envs=sample, what="configs[2]")
    assert env.cost_to_go_builds == 8192 * 64
    env.close()


def test_repeat_call_and_set_targets():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    for size in (16, 80):
        env = VecPogema(GridConfig(size=size, num_agents=8, obs_radius=3, density=0.3, seed=4), batch=6)
        env.reset(seed=4)
        model = CacheModel()
        got, want = _call_and_count(env, model)
        assert got == want == 6 * 8
        assert _call_and_count(env, model) == (0, 0)
        # move k active agents' targets to other free cells
        st = env.get_state()
        tgt = st["targets_xy"].cpu().numpy().copy()
        maps = installed_maps(env)
        rng = np.random.default_rng(size)
        moved = [(0, 1), (2, 5), (5, 0), (5, 7)]
        for b, i in moved:
            free = np.argwhere(maps[b] == 0)
            free = free[(free != tgt[b, i]).any(1)]
            tgt[b, i] = free[rng.integers(len(free))]
        env.set_targets(torch.as_tensor(tgt))
        got, want = _call_and_count(env, model)
        assert got == want == len(moved)
        _check(env, what=f"size {size} after set_targets")
        assert _call_and_count(env, model) == (0, 0)
        env.close()


def test_reset_where_rebuilds_those_envs():
    from pogema_amd import GridConfig, VecPogema
    for size in (16, 72):
        env = VecPogema(GridConfig(size=size, num_agents=6, obs_radius=3, density=0.3, seed=5), batch=8)
        env.reset(seed=5)
        model = CacheModel()
        _call_and_count(env, model)
        mask = np.zeros(8, dtype=bool)
        mask[[1, 4, 6]] = True
        env.reset_where(mask)
        got, want = _call_and_count(env, model)
        assert got == want == 3 * 6  # every agent of the 3 envs: their maps changed
        _check(env, what=f"size {size} after reset_where")
        env.close()


@pytest.mark.parametrize("size", [12, 70])
def test_restart_builds_exactly_the_changed_targets(size):
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=size, num_agents=8, obs_radius=3, density=0.2, seed=9, on_target="restart",
                    max_episode_steps=10**6)
    env = VecPogema(gc, batch=16)
    env.reset(seed=9)
    model = CacheModel()
    _call_and_count(env, model)
    rng = np.random.default_rng(9)
    total = 0
    for t in range(12):
        before = env.get_state()["targets_xy"].clone()
        env.step(mixed_actions(env, rng, p_expert=0.95))
        after = env.get_state()["targets_xy"]
        got, want = _call_and_count(env, model)
        assert got == want == int((before != after).any(-1).sum()), f"step {t}"
        total += got
    assert total > 0, "no lifelong draw happened"
    _check(env, what="restart")
    env.close()


@pytest.mark.parametrize("auto_reset", [True, "regenerate"])
def test_auto_reset(auto_reset):
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A = 12, 6
    gc = GridConfig(size=14, num_agents=A, obs_radius=3, density=0.3, seed=3, on_target="finish", max_episode_steps=6)
    env = VecPogema(gc, batch=B, auto_reset=auto_reset)
    env.reset(seed=3)
    model = CacheModel()
    assert _call_and_count(env, model) == (B * A, B * A)
    rng = np.random.default_rng(3)
    for t in range(14):
        env.step(torch.as_tensor(rng.integers(0, 5, size=(B, A)), device=env.device))
        got, want = _call_and_count(env, model)
        assert got == want, f"step {t}"
        if auto_reset is True:
            assert got == 0, f"step {t}: auto-reset to the initial state rebuilt {got} fields"
    _check(env, what=f"auto_reset={auto_reset}")
    if auto_reset == "regenerate":
        assert env.cost_to_go_builds > B * A
    env.close()


def test_load_state_of_another_map_rebuilds():
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=20, num_agents=5, obs_radius=3, density=0.3, seed=8), batch=6)
    env.reset(seed=1)
    snap = env.save_state()
    env.reset(seed=2)
    model = CacheModel()
    _call_and_count(env, model)
    env.load_state(snap)
    got, want = _call_and_count(env, model)
    assert got == want == 6 * 5
    _check(env, what="after load_state")
    env.close()


def test_map_pool():
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(13)
    pool = (rng.random((3, 16, 16)) < 0.2).astype(np.uint8)
    env = VecPogema(GridConfig(size=16, num_agents=4, obs_radius=3, density=0.2, seed=13), batch=10, map_pool=pool)
    env.reset(seed=13)
    model = CacheModel()
    _call_and_count(env, model)
    env.reset(seed=14)
    got, want = _call_and_count(env, model)
    assert got == want
    _check(env, what="map pool")
    env.close()


def test_state_untouched():
    """get_state() and the next step()'s outputs are identical with and without a preceding cost_to_go()."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    for size, coll, on_target in ((20, "soft", "restart"), (90, "block_both", "finish")):
        gc = GridConfig(size=size, num_agents=12, obs_radius=3, density=0.3, seed=31, collision_system=coll,
                        on_target=on_target, max_episode_steps=32)
        a = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
        b = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
        a.reset(seed=31)
        b.reset(seed=31)
        rng = np.random.default_rng(31)
        for t in range(6):
            acts = torch.as_tensor(rng.integers(0, 5, size=(8, 12)), device=a.device)
            a.cost_to_go()
            sa, sb = a.get_state(occupancy=True), b.get_state(occupancy=True)
            for k in sa:
                assert torch.equal(sa[k], sb[k]), f"size {size} step {t}: {k}"
            assert np.array_equal(installed_maps(a), installed_maps(b))
            ra, rb = a.step(acts), b.step(acts)
            for x, y in zip(ra[:4], rb[:4]):
                assert torch.equal(x, y), f"size {size} step {t}"
        a.close()
        b.close()


@pytest.mark.parametrize("size", [16, 72])
def test_graph_replay_equals_eager(size):
    """cost_to_go() -> step() captured once after an eager call; replays (with lifelong rebuilds) equal a twin's eager
    run, windows and build count included."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A = 16, 6
    gc = GridConfig(size=size, num_agents=A, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                    on_target="restart", max_episode_steps=10**6)
    eager = VecPogema(gc, batch=B)
    graphed = VecPogema(gc, batch=B)
    eager.reset(seed=4)
    graphed.reset(seed=4)
    w = 7
    win = torch.zeros((B, A, w, w), dtype=torch.int32, device="cuda")
    acts = torch.zeros((B, A), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream: allocates the cache
        graphed.cost_to_go(out=win)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.cost_to_go(out=win)
        out = graphed.step(acts)
    for t in range(40):
        # both follow the expert (their states are equal), so that agents reach targets and lifelong draws rebuild fields
        a, _ = eager.expert_actions()
        acts.copy_(a)
        g.replay()
        ref_w = eager.cost_to_go()
        ref = eager.step(a)
        assert torch.equal(win, ref_w), f"step {t}"
        for x, y in zip(out[:4], ref[:4]):
            assert torch.equal(x, y), f"step {t}"
    torch.cuda.synchronize()
    assert graphed.cost_to_go_builds == eager.cost_to_go_builds > B * A
    _check(graphed, what="after replays")
    eager.close()
    graphed.close()


def test_first_call_inside_capture_is_refused():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=70, num_agents=4, obs_radius=2, density=0.3, seed=12), batch=4)
    env.reset(seed=12)
    win = torch.zeros((4, 4, 5, 5), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError, match="bytes") as ei:
        with torch.cuda.graph(g):
            env.cost_to_go(out=win)
    assert ei.value.code == -4
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == 0
    _check(env, what="after the refused capture")
    env.close()


def test_out_buffer_list_view_and_errors():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21), batch=6)
    with pytest.raises(PgxError) as ei:
        env.cost_to_go()
    assert ei.value.code == -4  # before a reset, like step()
    env.reset(seed=21)
    w = env.cost_to_go()
    assert w.dtype == torch.int32 and tuple(w.shape) == (6, 5, 7, 7)
    o = torch.full((6, 5, 7, 7), 99, dtype=torch.int32, device=env.device)
    assert env.cost_to_go(out=o) is o and torch.equal(o, w)
    for bad in (torch.empty((6, 5, 7, 7), dtype=torch.int64, device=env.device),
                torch.empty((6, 5, 7, 6), dtype=torch.int32, device=env.device),
                torch.empty((6, 5, 7, 14), dtype=torch.int32, device=env.device)[..., ::2]):
        with pytest.raises(ValueError):
            env.cost_to_go(out=bad)
    env.close()

    one = pogema_v0(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21))
    one.reset(seed=21)
    views = one.cost_to_go()
    assert isinstance(views, list) and len(views) == 5
    assert all(isinstance(v, np.ndarray) and v.shape == (7, 7) and v.dtype == np.int32 for v in views)
    full = one._vec.cost_to_go()[0].cpu().numpy()
    assert all(np.array_equal(views[i], full[i]) for i in range(5))
    one.close()
