"""GPU: the global state (VecPogema.global_state / pgx_global_state, docs/SPEC.md S20), bit for bit: `obstacles` equals
pgx_get_map, `agents` the interior of get_state(occupancy=True), the other three planes the CPU reference
(tests/global_state_reference.py) on get_state(), with the ghost bit of the engine's `active` byte recovered from the
occupancy array; any selection and order of channels is the same planes picked from the full five; the four dtypes carry
the same values; a misaligned `out` changes nothing and nothing is written around it; the engine state is left alone, no
distance field is built, and a graph replay equals the eager run."""
import numpy as np
import pytest

from global_state_reference import CHANNELS, global_state_reference
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

BINARY = ("obstacles", "agents", "targets")


def _active_byte(env, st):
    """The engine's `active` byte per agent from get_state(occupancy=True): 0 hidden, 1 active, 3 an active agent whose
    own cell is clear in the occupancy array (Q2's ghost)."""
    torch = lazy_torch()
    r = env.obs_radius
    xy = st["agents_xy"].long() + r
    b = torch.arange(env.batch, device=env.device).view(-1, 1).expand(env.batch, env.num_agents)
    on_cell = st["occupancy"][b, xy[..., 0], xy[..., 1]] != 0
    active = st["is_active"]
    return torch.where(active, torch.where(on_cell, 1, 3), 0).cpu().numpy()


def _check(env, what, dtype=None):
    """global_state() on the env's current state against pgx_get_map, the occupancy array and the reference; returns the
    number of ghosts the state holds."""
    torch = lazy_torch()
    dtype = dtype or torch.float32
    B, H, W, r = env.batch, env.height, env.width, env.obs_radius
    got = env.global_state(channels=CHANNELS, dtype=dtype)
    assert got.dtype == dtype and tuple(got.shape) == (B, 5, H, W), what
    got = got.cpu().to(torch.float32).numpy().astype(np.int64)
    maps = installed_maps(env)
    st = env.get_state(occupancy=True)
    assert np.array_equal(got[:, 0], maps), f"{what}: obstacles differ from pgx_get_map"
    occ = st["occupancy"][:, r:r + H, r:r + W].cpu().numpy()
    assert np.array_equal(got[:, 1], occ), f"{what}: agents differ from the occupancy array"
    byte = _active_byte(env, st)
    ref = global_state_reference(maps, st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(), byte)
    for c in range(5):
        assert np.array_equal(got[:, c], ref[:, c]), f"{what}: plane {CHANNELS[c]} differs from the reference"
    default = env.global_state()
    assert default.dtype == torch.float32 and tuple(default.shape) == (B, 3, H, W)
    assert np.array_equal(default.cpu().numpy(), ref[:, :3].astype(np.float32)), f"{what}: the default three planes"
    return int((byte == 3).sum())


# ---- 1: modes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=12, num_agents=10, obs_radius=3, density=0.25, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=64)
    env = VecPogema(gc, batch=7)
    env.reset(seed=7)
    rng = np.random.default_rng(11)
    hidden = False
    for t in range(13):
        if t % 4 == 0:
            _check(env, f"{collision}/{on_target} step {t}")
            hidden |= not bool(env.get_state()["is_active"].all())
        env.step(mixed_actions(env, rng, p_expert=0.85))
    if on_target == "finish":
        assert hidden, "no hidden agent was ever in the state"
    env.close()


# ---- 2: ghosts -------------------------------------------------------------------------------------------------------------
def test_soft_ghosts_are_honoured():
    """Q2, the literal `soft_occupancy`: random actions until an active agent's own cell is clear in the occupancy array;
    then `agents` is not "every active agent's cell", while the ghost's target is still in `targets`."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=8, num_agents=12, obs_radius=2, density=0.1, seed=5, collision_system="soft", on_target="nothing",
                    max_episode_steps=1000)
    env = VecPogema(gc, batch=8)
    env.reset(seed=5)
    rng = np.random.default_rng(5)
    ghosts = 0
    for t in range(48):
        env.step(torch.as_tensor(rng.integers(0, 5, size=(8, 12)), device=env.device))
        ghosts = int((_active_byte(env, env.get_state(occupancy=True)) == 3).sum())
        if ghosts:
            break
    assert ghosts, "no ghost within 48 random steps: pick another seed"
    assert _check(env, f"soft, {ghosts} ghosts after {t + 1} steps") == ghosts
    st = env.get_state()
    planes = env.global_state(channels=("agents", "targets"), dtype=torch.uint8)
    assert int(planes[:, 0].sum()) == int(st["is_active"].sum()) - ghosts    # (soft: no two agents share a cell)
    b = torch.arange(8, device=env.device).view(8, 1).expand(8, 12)
    txy = st["targets_xy"].long()
    assert bool((planes[:, 1][b, txy[..., 0], txy[..., 1]] == 1).all()), "an active agent's target is missing"
    env.close()


# ---- 3: shapes -------------------------------------------------------------------------------------------------------------
def _map_env(grid, agents, r, batch, seed, **kw):
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(map=grid.astype(int).tolist(), num_agents=agents, obs_radius=r, seed=seed,
                               max_episode_steps=64, **kw), batch=batch)
    env.reset(seed=seed)
    return env


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_odd_plane_size_misaligns_every_later_plane(dtype):
    """9 x 13 = 117 elements per plane: in a 1- or 2-byte format no plane after the first starts on a 16-byte boundary."""
    torch = lazy_torch()
    rng = np.random.default_rng(3)
    env = _map_env(rng.random((9, 13)) < 0.2, 7, 3, 3, 3)
    _check(env, f"9 x 13 {dtype} reset", getattr(torch, dtype))
    for _ in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, f"9 x 13 {dtype} after 3 steps", getattr(torch, dtype))
    env.close()


def test_wide_map_rows_span_bitmap_words():
    """40 x 70 under r = 5: a padded bitmap row has three words, and a map row starts at bit 5 of the first."""
    rng = np.random.default_rng(4)
    env = _map_env(rng.random((40, 70)) < 0.3, 9, 5, 3, 4)
    assert (env.width + 2 * env.obs_radius + 31) // 32 == 3
    _check(env, "40 x 70 reset")
    for _ in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, "40 x 70 after 3 steps")
    env.close()


def test_several_bands_agents_on_band_edges():
    """A map of three bands by the published cell budget (the last one short), two envs, agents and targets put on the
    first and the last row of every band."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, _lib
    W = 120
    R = _lib.GLOBAL_BAND_CELLS // W          # rows per band
    H = 2 * R + 5
    assert R >= 2 and -(-H // R) == 3
    rng = np.random.default_rng(6)
    obst = (rng.random((2, H, W)) < 0.15).astype(np.uint8)
    rows = [0, R - 1, R, 2 * R - 1, 2 * R, H - 1]
    obst[:, rows, :] = 0
    A = 2 * len(rows)
    agents = np.zeros((2, A, 2), dtype=np.int32)
    targets = np.zeros((2, A, 2), dtype=np.int32)
    for b in range(2):
        for k, row in enumerate(rows):       # two agents per edge row; their targets on the edge rows in reverse order
            agents[b, 2 * k], agents[b, 2 * k + 1] = (row, 3 + b), (row, W - 1 - b)
            targets[b, 2 * k], targets[b, 2 * k + 1] = (rows[-1 - k], 7 + b), (rows[-1 - k], 0)
    env = VecPogema(GridConfig(map=obst[0].astype(int).tolist(), num_agents=A, obs_radius=2, max_episode_steps=64), batch=2)
    env.reset_from_state(obst, agents, targets, validate=False)
    _check(env, "three bands")
    got = env.global_state(channels=("agent_ids", "target_ids"), dtype=torch.float16).cpu().float().numpy()
    for b in range(2):
        for i in range(A):
            assert got[b, 0, agents[b, i, 0], agents[b, i, 1]] == i + 1
            assert got[b, 1, targets[b, i, 0], targets[b, i, 1]] == i + 1
    assert int((got[:, 0] != 0).sum()) == 2 * A and int((got[:, 1] != 0).sum()) == 2 * A
    env.close()


def test_one_row_map():
    rng = np.random.default_rng(8)
    env = _map_env(np.zeros((1, 9), dtype=bool), 3, 2, 3, 8)
    _check(env, "1 x 9 reset")
    for _ in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, "1 x 9 after 3 steps")
    env.close()


# ---- 4: agent counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agents,batch,dtypes", [(1, 5, ("float32",)), (65, 3, ("float32",)), (300, 2, ("float16", "float32"))])
def test_agents_per_env(agents, batch, dtypes):
    """One lane, just over one wave, and more agents than the workgroup has lanes (two rounds of the per-agent loop)."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=40, num_agents=agents, obs_radius=2, density=0.1, seed=agents, collision_system="soft",
                    on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=batch)
    env.reset(seed=agents)
    rng = np.random.default_rng(agents)
    for _ in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    for dtype in dtypes:
        _check(env, f"A={agents} {dtype}", getattr(torch, dtype))
    if agents == 300:
        for dtype, limit in ((torch.uint8, "255"), (torch.bfloat16, "256")):
            for channels in (("agent_ids",), ("obstacles", "target_ids")):
                with pytest.raises(ValueError, match=f"at most {limit}"):
                    env.global_state(channels=channels, dtype=dtype)
            narrow = env.global_state(dtype=dtype)   # the binary planes hold any count
            assert torch.equal(narrow.float(), env.global_state())
    env.close()


def test_a1024():
    """The `a1024` row of the parity matrix: PGX_MAX_AGENTS on a 52 x 52 map, four rounds of the per-agent loop."""
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=52, num_agents=1024, obs_radius=2, density=0.05, seed=5, max_episode_steps=64)
    env = VecPogema(gc, batch=1)
    env.reset(seed=5)
    env.step(mixed_actions(env, np.random.default_rng(5), p_expert=0.7))
    _check(env, "a1024")
    env.close()


# ---- 5, 6: selection and order, dtypes, out= -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moved_env():
    """One engine a few steps into its episodes, shared by the tests that only read it: a 9 x 13 map, so that in the narrow
    formats the planes after the first are misaligned whatever `out` is."""
    torch = lazy_torch()
    rng = np.random.default_rng(17)
    env = _map_env(rng.random((9, 13)) < 0.2, 9, 3, 5, 17, on_target="finish")
    for _ in range(5):
        env.step(mixed_actions(env, rng, p_expert=0.8))
    full = env.global_state(channels=CHANNELS)
    assert full.dtype == torch.float32
    yield env, full
    env.close()


PERMUTATIONS = [(3, 4, 0, 1, 2), (2, 0, 4), (4, 1, 3, 0)]   # ids before binaries; a mix; another mix


def test_selection_and_order(moved_env):
    torch = lazy_torch()
    env, full = moved_env
    assert tuple(full.shape) == (5, 5, 9, 13) and all(bool(full[:, c].any()) for c in range(5))
    assert float(full[:, 3:].max()) > 1.0
    for c, name in enumerate(CHANNELS):
        one = env.global_state(channels=(name,))
        assert tuple(one.shape) == (5, 1, 9, 13) and torch.equal(one[:, 0], full[:, c]), name
    for sel in PERMUTATIONS:
        got = env.global_state(channels=[CHANNELS[k] for k in sel])
        assert torch.equal(got, full.index_select(1, torch.as_tensor(sel, device=env.device))), sel


def test_dtypes(moved_env):
    torch = lazy_torch()
    env, full = moved_env
    for channels in (CHANNELS, BINARY, ("target_ids", "agents")):
        f32 = env.global_state(channels=channels)
        for dtype in (torch.float16, torch.bfloat16, torch.uint8):
            got = env.global_state(channels=channels, dtype=dtype)
            assert got.dtype == dtype and got.shape == f32.shape
            assert torch.equal(got.to(torch.float32), f32), (channels, dtype)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16", "uint8"])
def test_out_aligned_and_misaligned(moved_env, dtype):
    """A caller's tensor is returned as it is; a view one element into a larger buffer is no longer 16-byte aligned: the
    same planes, and the guard elements around it keep their value."""
    torch = lazy_torch()
    env, _ = moved_env
    dtype = getattr(torch, dtype)
    for channels in (CHANNELS, BINARY, ("agent_ids",)):
        want = env.global_state(channels=channels, dtype=dtype)
        assert want.data_ptr() % 16 == 0
        own = torch.full(want.shape, 7, dtype=dtype, device=env.device)
        assert env.global_state(channels=channels, dtype=dtype, out=own) is own and torch.equal(own, want)
        n = want.numel()
        buf = torch.full((n + 32,), 7, dtype=dtype, device=env.device)
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + n].view(want.shape)
        assert view.data_ptr() % 16 == want.element_size()
        assert env.global_state(channels=channels, dtype=dtype, out=view) is view
        assert torch.equal(view, want)
        assert bool((buf[:1] == 7).all()) and bool((buf[1 + n:] == 7).all())


def test_refusals(moved_env):
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    env, full = moved_env
    with pytest.raises(ValueError, match="'target'.*'target_ids'"):
        env.global_state(channels=("obstacles", "target"))
    with pytest.raises(ValueError, match="given twice"):
        env.global_state(channels=("agents", "agents"))
    with pytest.raises(ValueError, match="dtype"):
        env.global_state(dtype=torch.int32)
    shape = tuple(full.shape)
    for bad in (torch.empty(shape, dtype=torch.float16, device=env.device),
                torch.empty(shape[:1] + (4,) + shape[2:], dtype=torch.float32, device=env.device),
                torch.empty(shape[:-1] + (26,), dtype=torch.float32, device=env.device)[..., ::2],
                torch.empty(shape, dtype=torch.float32)):
        with pytest.raises(ValueError, match="out must be"):
            env.global_state(channels=CHANNELS, out=bad)
    # 10: before a reset, like step()
    fresh = VecPogema(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21), batch=2)
    with pytest.raises(PgxError) as ei:
        fresh.global_state()
    assert ei.value.code == -4
    fresh.close()


# ---- 7: the state is left alone --------------------------------------------------------------------------------------------
def _snapshot(env):
    """The engine's snapshot in a zero-filled blob (save_state() leaves the padding between segments as torch.empty gave it)."""
    torch = lazy_torch()
    from pogema_amd import _lib
    blob = torch.zeros(int(env._lib.pgx_snapshot_bytes(env._handle)), dtype=torch.uint8, device=env.device)
    _lib.check(env._lib.pgx_save_snapshot(env._handle, blob.data_ptr(), env._stream()))
    return blob


def test_state_untouched_and_next_step_equals_a_twins():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=14, num_agents=11, obs_radius=3, density=0.25, seed=31, collision_system="soft",
                    on_target="restart", max_episode_steps=32)
    env, twin = VecPogema(gc, batch=6, auto_reset=True), VecPogema(gc, batch=6, auto_reset=True)
    env.reset(seed=31)
    twin.reset(seed=31)
    rng = np.random.default_rng(31)
    for t in range(4):
        actions = torch.as_tensor(rng.integers(0, 5, size=(6, 11)), device=env.device)
        got, want = env.step(actions), twin.step(actions)    # the twin never calls global_state()
        for k, (x, y) in enumerate(zip(got[:4], want[:4])):
            assert torch.equal(x, y), f"step {t}: output {k} differs from the twin's"
        before, blob = env.get_state(occupancy=True), _snapshot(env)
        env.global_state(channels=CHANNELS if t % 2 else BINARY, dtype=(torch.float32, torch.uint8)[t % 2])
        after = env.get_state(occupancy=True)
        for k in before:
            assert torch.equal(before[k], after[k]), f"step {t}: {k}"
        assert torch.equal(blob, _snapshot(env)), f"step {t}: the snapshot changed"
    assert env.cost_to_go_builds == 0
    env.close()
    twin.close()


# ---- 8: graph capture ------------------------------------------------------------------------------------------------------
def test_capture_as_first_call_after_reset():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=16, num_agents=6, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                    on_target="nothing", max_episode_steps=10**6)
    env = VecPogema(gc, batch=6)
    env.reset(seed=4)
    out = torch.zeros((6, 5, 16, 16), dtype=torch.float32, device=env.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                # the engine's first call after reset, and it is captured: nothing to allocate
        env.global_state(channels=CHANNELS, out=out)
    rng = np.random.default_rng(4)
    for t in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.7))
        out.zero_()
        g.replay()
        assert torch.equal(out, env.global_state(channels=CHANNELS)), f"replay after step {t}"
    assert bool(out[:, 1].any()) and bool(out[:, 4].any())
    env.close()


# ---- 9: fresh maps ---------------------------------------------------------------------------------------------------------
def test_regenerated_pool_maps_and_copies():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(3)
    pool = (rng.random((6, 10, 11)) < 0.2).astype(np.uint8)
    pool[np.arange(6), 0, np.arange(6)] = 1              # no two maps are equal
    pool[np.arange(6), 1, np.arange(6)] = 0
    gc = GridConfig(num_agents=4, obs_radius=2, seed=21, on_target="finish", max_episode_steps=3)
    env = VecPogema(gc, batch=12, auto_reset="regenerate", map_pool=pool)
    env.reset(seed=21)
    first = env.map_index.cpu().numpy()
    for _ in range(7):                       # two episode ends per env
        env.step(torch.as_tensor(rng.integers(0, 5, size=(12, 4)), device=env.device))
    now = env.map_index.cpu().numpy()
    assert (now != first).any(), "no env drew another map: the first reset's maps would pass"
    assert np.array_equal(env.global_state(channels=("obstacles",), dtype=torch.uint8)[:, 0].cpu().numpy(), pool[now])
    _check(env, "after regeneration")
    env.step(torch.as_tensor(rng.integers(1, 5, size=(12, 4)), device=env.device))
    before = env.global_state(channels=CHANNELS)
    src, dst = [0, 1, 2], [5, 6, 7]
    assert not torch.equal(before[src], before[dst])
    env.copy_envs(src, dst)
    after = env.global_state(channels=CHANNELS)
    assert torch.equal(after[dst], before[src]) and torch.equal(after[src], before[src])
    keep = [b for b in range(12) if b not in dst]
    assert torch.equal(after[keep], before[keep])
    _check(env, "after copy_envs")
    env.close()


# ---- the list view -----------------------------------------------------------------------------------------------------------
def test_list_view():
    torch = lazy_torch()
    from pogema_amd import GridConfig, pogema_v0
    one = pogema_v0(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21))
    one.reset(seed=21)
    one.step([1, 2, 3, 4, 0])
    for channels, C in ((None, 3), (CHANNELS, 5), (("target_ids", "agents"), 2)):
        planes = one.global_state() if channels is None else one.global_state(channels)
        assert isinstance(planes, np.ndarray) and planes.shape == (C, 16, 16) and planes.dtype == np.uint8
        kw = {} if channels is None else {"channels": channels}
        assert np.array_equal(planes, one._vec.global_state(dtype=torch.uint8, **kw)[0].cpu().numpy())
    assert planes.any()
    as_float = one.global_state(CHANNELS, dtype=np.float32)
    assert as_float.dtype == np.float32 and np.array_equal(as_float, one.global_state(CHANNELS).astype(np.float32))
    with pytest.raises(ValueError, match="dtype"):
        one.global_state(dtype=np.int32)
    one.close()
