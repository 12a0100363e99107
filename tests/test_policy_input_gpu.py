"""GPU: the policy input (VecPogema.policy_input / pgx_policy_input, docs/SPEC.md S18), bit for bit: planes 0-2 equal
observe(), planes 4-7 equal goal_directions(), plane 3 equals the CPU reference (tests/policy_input_reference.py) on
get_state(); any selection and order of channels is the same planes picked from the full eight; the four dtypes carry
the same bits; a misaligned `out` changes nothing and nothing is written around it; the engine state is left alone, the
field cache is only touched by a direction channel, and a graph replay equals the eager run."""
import numpy as np
import pytest

from policy_input_reference import CHANNELS, other_goals_reference
from util import lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

OBS = ("obstacles", "agents", "target")
DIRS = ("up", "down", "left", "right")


def _other_goals(env):
    st = env.get_state()
    return other_goals_reference(st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                                 st["is_active"].cpu().numpy(), env.obs_radius)


def _check(env, what):
    """policy_input() on the env's current state against observe(), goal_directions() and the reference."""
    torch = lazy_torch()
    w, shape = env.window, (env.batch, env.num_agents)
    obs = env.observe(out=torch.empty(env.obs_shape, dtype=torch.float32, device=env.device))
    got = env.policy_input(channels=OBS)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape + (3, w, w)
    for c, name in enumerate(OBS):
        assert torch.equal(got[:, :, c], obs[:, :, c]), f"{what}: plane {name} differs from observe()"
    assert torch.equal(got, obs), what
    planes = env.goal_directions()
    assert torch.equal(env.policy_input(channels=DIRS), planes), f"{what}: the four direction planes together"
    for c, name in enumerate(DIRS):
        one = env.policy_input(channels=(name,))
        assert tuple(one.shape) == shape + (1, w, w)
        assert torch.equal(one[:, :, 0], planes[:, :, c]), f"{what}: plane {name} alone differs from goal_directions()"
    assert torch.equal(env.policy_input(), torch.cat((obs, planes), 2)), f"{what}: the default seven planes"
    ref = torch.as_tensor(_other_goals(env), device=env.device).to(torch.float32)
    assert torch.equal(env.policy_input(channels=("other_goals",))[:, :, 0], ref), f"{what}: other_goals"
    return obs


def _run(gc, batch, seed, what, steps=4):
    from pogema_amd import VecPogema
    env = VecPogema(gc, batch=batch)
    env.reset(seed=seed)
    rng = np.random.default_rng(seed)
    _check(env, f"{what} reset")
    for _ in range(steps):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, f"{what} after {steps} steps")
    return env


# ---- 1 + 2: planes 0-2 equal observe(), planes 4-7 equal goal_directions() -------------------------------------------
@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    """Every collision system under every on_target mode; under `finish` hidden agents are among the observers."""
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=12, num_agents=10, obs_radius=3, density=0.25, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=64)
    env = VecPogema(gc, batch=7)             # 70 slots: no multiple of 4, every call ends in the tail path
    env.reset(seed=7)
    rng = np.random.default_rng(11)
    hidden = False
    for t in range(13):
        if t % 4 == 0:
            _check(env, f"{collision}/{on_target} step {t}")
            hidden |= not bool(env.get_state()["is_active"].all())
        env.step(mixed_actions(env, rng, p_expert=0.85))
    if on_target == "finish":
        assert hidden, "no hidden agent was ever an observer"
    env.close()


def test_soft_ghosts_are_honoured():
    """Q2, the literal `soft_occupancy`: an agent that followed a higher-index agent stands on its cell but is missing
    from the occupancy array.  Random actions until the state holds such an agent -- an active agent whose own cell is
    clear in get_state(occupancy=True) -- then the `agents` plane must leave it out exactly as observe() does."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=8, num_agents=12, obs_radius=2, density=0.1, seed=5, collision_system="soft", on_target="nothing",
                    max_episode_steps=1000)
    env = VecPogema(gc, batch=8)
    env.reset(seed=5)
    rng = np.random.default_rng(5)
    r, ghosts = env.obs_radius, 0
    for t in range(48):
        env.step(torch.as_tensor(rng.integers(0, 5, size=(8, 12)), device=env.device))
        st = env.get_state(occupancy=True)
        xy = st["agents_xy"].long() + r
        b = torch.arange(8, device=env.device).view(8, 1).expand(8, 12)
        ghosts = int(((st["occupancy"][b, xy[..., 0], xy[..., 1]] == 0) & st["is_active"]).sum())
        if ghosts:
            break
    assert ghosts, "no ghost within 48 random steps: pick another seed"
    obs = _check(env, f"soft, {ghosts} ghosts after {t + 1} steps")
    centre = obs[:, :, 1, r, r]
    assert int((centre == 0).sum()) >= ghosts, "a ghost does not see itself at its window's centre"
    env.close()


def test_empty_outside_false():
    from pogema_amd import GridConfig
    gc = GridConfig(size=10, num_agents=6, obs_radius=4, density=0.3, seed=2, empty_outside=False, max_episode_steps=64)
    env = _run(gc, 3, 2, "empty_outside=False")
    # (an agent within r - 2 cells of the border sees cells beyond the ring around the map)
    assert bool((env.get_state()["agents_xy"] <= env.obs_radius - 2).any())
    env.close()


def test_non_square_map_and_map_smaller_than_the_window():
    from pogema_amd import GridConfig
    rng = np.random.default_rng(3)
    grid = (rng.random((9, 23)) < 0.2).astype(int).tolist()
    _run(GridConfig(map=grid, num_agents=7, obs_radius=3, seed=3, max_episode_steps=64), 3, 3, "9 x 23").close()
    _run(GridConfig(size=12, num_agents=5, obs_radius=15, density=0.2, seed=4, max_episode_steps=64), 3, 4,
         "12 x 12 under a 31 x 31 window").close()


@pytest.mark.parametrize("radius", [1, 2, 5, 15])
def test_obs_radius(radius):
    """W^2 = 9, 25, 121, 961; 3 x 6 = 18 slots leave a tail in every format."""
    from pogema_amd import GridConfig
    gc = GridConfig(size=20, num_agents=6, obs_radius=radius, density=0.3, seed=radius, on_target="restart",
                    max_episode_steps=64)
    _run(gc, 3, radius, f"radius {radius}", steps=3).close()


@pytest.mark.parametrize("agents,batch", [(1, 5), (3, 3), (64, 2), (65, 3), (130, 2)])
def test_agents_per_env(agents, batch):
    """One lane, a partial wave, exactly one wave, just over one wave and three waves of the per-agent loop; 5, 9 and 195
    slots are no multiple of the slots per range."""
    from pogema_amd import GridConfig
    gc = GridConfig(size=24, num_agents=agents, obs_radius=2, density=0.1, seed=agents, collision_system="soft",
                    on_target="finish", max_episode_steps=64)
    _run(gc, batch, agents, f"A={agents}", steps=3).close()


# ---- 3: other_goals equals the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("on_target", ["finish", "restart"])
def test_other_goals_match_reference(on_target):
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=16, num_agents=12, obs_radius=2, density=0.2, seed=13, on_target=on_target, max_episode_steps=64)
    env = VecPogema(gc, batch=8)
    env.reset(seed=13)
    rng = np.random.default_rng(13)
    for _ in range(6):
        env.step(mixed_actions(env, rng, p_expert=0.8))
    ref = _other_goals(env)
    active = env.get_state()["is_active"].cpu().numpy()
    edge = np.ones((5, 5), dtype=bool)
    edge[1:-1, 1:-1] = False
    # the reference alone says that the state exercises the definition
    assert ref[:, :, ~edge].any(), "no set cell strictly inside a window"
    assert ref[:, :, edge].any(), "no set cell on a window's edge (a clamped target)"
    per_observer = ref.reshape(8, 12, -1).sum(-1)
    assert (per_observer >= 2).any(), "no observer with two or more set cells"
    assert ((per_observer == 0) & active).any(), "no active observer with an all-zero plane"
    assert not ref[~active].any()
    if on_target == "finish":
        assert not active.all(), "no hidden agent"
    got = env.policy_input(channels=("other_goals",))
    assert torch.equal(got[:, :, 0], torch.as_tensor(ref, device=env.device).to(torch.float32))
    # PRIMAL's four planes: the observation, then the other agents' goals
    primal = env.policy_input(channels=OBS + ("other_goals",))
    assert torch.equal(primal[:, :, :3], env.observe()) and torch.equal(primal[:, :, 3], got[:, :, 0])
    env.close()


# ---- 4, 5, 6: selection and order, dtypes, out= --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moved_env():
    """One engine a few steps into its episodes, shared by the tests that only read it."""
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=16, num_agents=9, obs_radius=3, density=0.25, seed=17, on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=5)             # 45 slots: a tail in every format
    env.reset(seed=17)
    rng = np.random.default_rng(17)
    for _ in range(5):
        env.step(mixed_actions(env, rng, p_expert=0.8))
    full = env.policy_input(channels=CHANNELS)
    yield env, full
    env.close()


SELECTIONS = [(7, 3, 0, 5, 1, 6, 2, 4), (3,), (6,), (2, 0), (7, 4), (1, 3, 5, 7, 0), (4, 0, 3, 2, 6)]


def test_selection_and_order(moved_env):
    torch = lazy_torch()
    env, full = moved_env
    assert tuple(full.shape) == (5, 9, 8, 7, 7) and all(bool(full[:, :, c].any()) for c in range(8))
    assert set(full.unique().tolist()) == {0.0, 1.0}
    assert {len(s) for s in SELECTIONS} == {1, 2, 5, 8}
    for sel in SELECTIONS:
        got = env.policy_input(channels=[CHANNELS[k] for k in sel])
        want = full.index_select(2, torch.as_tensor(sel, device=env.device))
        assert torch.equal(got, want), sel


@pytest.mark.parametrize("bf16_engine", [False, True])
def test_dtypes(moved_env, bf16_engine):
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    if bf16_engine:                          # the dtype is chosen per call, whatever the observation format of the engine
        gc = GridConfig(size=16, num_agents=9, obs_radius=3, density=0.25, seed=17, max_episode_steps=64)
        env = VecPogema(gc, batch=5, obs_dtype=torch.bfloat16)
        env.reset(seed=17)
        env.step(mixed_actions(env, np.random.default_rng(17), p_expert=0.8))
        assert env.observe().dtype == torch.bfloat16
    else:
        env = moved_env[0]
    for channels in (CHANNELS, CHANNELS[:7], OBS + ("other_goals",), ("agents", "up", "target")):  # C = 8, 7, 4, 3
        f32 = env.policy_input(channels=channels)
        assert f32.dtype == torch.float32 and bool(f32.any())
        for dtype in (torch.float16, torch.bfloat16, torch.uint8):
            got = env.policy_input(channels=channels, dtype=dtype)
            assert got.dtype == dtype and got.shape == f32.shape
            assert torch.equal(got, f32.to(dtype)), (channels, dtype)
    if bf16_engine:
        assert torch.equal(env.policy_input(channels=OBS, dtype=torch.bfloat16), env.observe())
        env.close()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16", "uint8"])
def test_out_aligned_and_misaligned(moved_env, dtype):
    """A caller's tensor is returned as it is; a view one element into a larger buffer is no longer 16-byte aligned and
    takes the element-wise stores: the same planes, and the guard elements around it keep their value."""
    torch = lazy_torch()
    env, _ = moved_env
    dtype = getattr(torch, dtype)
    for channels in (CHANNELS, CHANNELS[:7], ("other_goals", "agents", "left")):
        want = env.policy_input(channels=channels, dtype=dtype)
        assert want.data_ptr() % 16 == 0
        own = torch.full(want.shape, 7, dtype=dtype, device=env.device)
        assert env.policy_input(channels=channels, dtype=dtype, out=own) is own and torch.equal(own, want)
        n = want.numel()
        buf = torch.full((n + 16,), 7, dtype=dtype, device=env.device)
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + n].view(want.shape)
        assert view.data_ptr() % 16 == want.element_size()
        assert env.policy_input(channels=channels, dtype=dtype, out=view) is view
        assert torch.equal(view, want)
        assert bool((buf[:1] == 7).all()) and bool((buf[1 + n:] == 7).all())


def test_refusals(moved_env):
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    env, full = moved_env
    with pytest.raises(ValueError, match="'goals'.*'other_goals'"):
        env.policy_input(channels=("obstacles", "goals"))
    with pytest.raises(ValueError, match="given twice"):
        env.policy_input(channels=("up", "up"))
    with pytest.raises(ValueError, match="dtype"):
        env.policy_input(dtype=torch.int32)
    shape = tuple(full.shape)
    for bad in (torch.empty(shape, dtype=torch.float16, device=env.device),
                torch.empty(shape[:2] + (7,) + shape[3:], dtype=torch.float32, device=env.device),
                torch.empty(shape[:-1] + (14,), dtype=torch.float32, device=env.device)[..., ::2],
                torch.empty(shape, dtype=torch.float32)):
        with pytest.raises(ValueError, match="out must be"):
            env.policy_input(channels=CHANNELS, out=bad)
    fresh = VecPogema(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21), batch=2)
    with pytest.raises(PgxError) as ei:
        fresh.policy_input(channels=OBS)
    assert ei.value.code == -4               # before a reset, like step()
    fresh.close()


# ---- 7: read-only, the cache, graph capture -----------------------------------------------------------------------------
def _snapshot(env):
    """The engine's snapshot in a zero-filled blob: save_state() leaves the padding between the 16-byte aligned segments
    as torch.empty gave it, so two of its blobs of one state need not be equal byte for byte."""
    torch = lazy_torch()
    from pogema_amd import _lib
    blob = torch.zeros(int(env._lib.pgx_snapshot_bytes(env._handle)), dtype=torch.uint8, device=env.device)
    _lib.check(env._lib.pgx_save_snapshot(env._handle, blob.data_ptr(), env._stream()))
    return blob


def test_state_untouched():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=14, num_agents=11, obs_radius=3, density=0.25, seed=31, collision_system="soft",
                    on_target="restart", max_episode_steps=32)
    env = VecPogema(gc, batch=6, auto_reset=True)
    env.reset(seed=31)
    rng = np.random.default_rng(31)
    for t in range(4):
        env.step(torch.as_tensor(rng.integers(0, 5, size=(6, 11)), device=env.device))
        before, blob = env.get_state(occupancy=True), _snapshot(env)
        env.policy_input(channels=CHANNELS if t % 2 else OBS + ("other_goals",), dtype=(torch.float32, torch.uint8)[t % 2])
        after = env.get_state(occupancy=True)
        for k in before:
            assert torch.equal(before[k], after[k]), f"step {t}: {k}"
        assert torch.equal(blob, _snapshot(env)), f"step {t}: the snapshot changed"
    env.close()


def test_no_direction_channel_no_cache_and_capture_as_first_call():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=16, num_agents=6, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                    on_target="nothing", max_episode_steps=10**6)
    env = VecPogema(gc, batch=6)
    env.reset(seed=4)
    channels = OBS + ("other_goals",)
    out = torch.zeros((6, 6, 4, 7, 7), dtype=torch.float32, device=env.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                # the engine's first query, and it is captured: nothing to allocate
        env.policy_input(channels=channels, out=out)
    rng = np.random.default_rng(4)
    for t in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.7))
        out.zero_()
        g.replay()
        assert torch.equal(out, env.policy_input(channels=channels)), f"replay after step {t}"
    assert bool(out.any())
    assert env.cost_to_go_builds == 0
    # the first use of the cache still allocates it and builds every field: nothing had been allocated before
    env.policy_input(channels=("up",))
    assert env.cost_to_go_builds == 36
    env.close()


def test_direction_channels_share_the_cache_and_replay():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    gc = GridConfig(size=16, num_agents=6, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                    on_target="nothing", max_episode_steps=10**6)
    env = VecPogema(gc, batch=6)
    env.reset(seed=4)
    out = torch.zeros((6, 6, 7, 7, 7), dtype=torch.float32, device=env.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError, match="bytes") as ei:   # the first user of the cache allocates it: not inside a capture
        with torch.cuda.graph(g):
            env.policy_input(out=out)
    assert ei.value.code == -4
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == 0
    eager = env.policy_input()               # eager: allocates the cache, builds every field
    assert env.cost_to_go_builds == 36
    env.policy_input(out=out)
    env.goal_directions()
    assert env.cost_to_go_builds == 36, "a second call on an unchanged state built fields"
    assert torch.equal(out, eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.policy_input(out=out)
    rng = np.random.default_rng(4)
    for t in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.7))
        out.zero_()
        g.replay()
        assert torch.equal(out, env.policy_input()), f"replay after step {t}"
    env.close()


# ---- 8: the list view ---------------------------------------------------------------------------------------------------
def test_list_view():
    torch = lazy_torch()
    from pogema_amd import GridConfig, pogema_v0
    one = pogema_v0(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21))
    one.reset(seed=21)
    one.step([1, 2, 3, 4, 0])
    for channels, C in ((None, 7), (CHANNELS, 8), (("other_goals", "agents"), 2)):
        views = one.policy_input() if channels is None else one.policy_input(channels)
        assert isinstance(views, list) and len(views) == 5
        assert all(isinstance(v, np.ndarray) and v.shape == (C, 7, 7) and v.dtype == np.uint8 for v in views)
        kw = {} if channels is None else {"channels": channels}
        row = one._vec.policy_input(dtype=torch.uint8, **kw)[0].cpu().numpy()
        assert all(np.array_equal(views[i], row[i]) for i in range(5))
    assert any(v.any() for v in views)
    one.close()
