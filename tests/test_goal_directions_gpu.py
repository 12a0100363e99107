"""GPU: direction-to-goal planes (VecPogema.goal_directions / pgx_goal_directions, docs/SPEC.md S14) equal the CPU
reference (tests/goal_directions_reference.py) bit for bit on get_state() and the installed maps -- both field-build
layouts, 2- and 4-byte fields, every collision system and on_target mode, slot counts that leave a tail -- in all three
formats; a misaligned `out` changes nothing; the shared field cache follows S11's contract; the engine state is left
alone; a graph replay equals the eager run; the grid-stride loop runs."""
import os
import re

import numpy as np
import pytest

from goal_directions_reference import goal_directions_reference, planes
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("float32", "uint8", "bits")
# one env per line covers every collision system and every on_target mode
MODES = (("priority", "finish"), ("block_both", "restart"), ("soft", "nothing"))


def _reference(env, envs=None):
    st = env.get_state()
    return goal_directions_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                                     st["is_active"].cpu().numpy(), env.obs_radius, envs=envs)


def _check(env, what="", envs=None):
    """Every format of goal_directions() == the reference, bit for bit; returns the reference's masks."""
    torch = lazy_torch()
    ref = _reference(env, envs)
    rows = slice(None) if envs is None else list(envs)
    w = env.window
    for fmt in FORMATS:
        got = env.goal_directions(format=fmt)
        if fmt == "bits":
            assert got.dtype == torch.uint8 and tuple(got.shape) == (env.batch, env.num_agents, w, w)
            want = ref
        else:
            assert got.dtype == (torch.float32 if fmt == "float32" else torch.uint8)
            assert tuple(got.shape) == (env.batch, env.num_agents, 4, w, w)
            want = planes(ref).astype(np.float32 if fmt == "float32" else np.uint8)
        got = got.cpu().numpy()
        bad = np.argwhere(got[rows] != want[rows])
        assert bad.size == 0, (f"{what} [{fmt}]: {len(bad)} mismatches, first {bad[0].tolist()}: "
                               f"{got[rows][tuple(bad[0])]} vs {want[rows][tuple(bad[0])]}")
    return ref


def _reset_and_steps(gc, batch, seed, what, steps=4):
    from pogema_amd import VecPogema
    env = VecPogema(gc, batch=batch)
    env.reset(seed=seed)
    rng = np.random.default_rng(seed)
    _check(env, what=f"{what} reset")
    for _ in range(steps):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, what=f"{what} after {steps} steps")
    env.close()


# sides 64 and 65 switch between the two field-build layouts; with batch 3 the slot counts 3, 18 and 39 are no multiple
# of 4 or 16, so that every call ends in the tail path
@pytest.mark.parametrize("size", [2, 8, 31, 32, 33, 63, 64, 65])
def test_square_maps_match_reference(size):
    from pogema_amd import GridConfig
    for k, agents in enumerate((1, 6, 13)):
        collision, on_target = MODES[(k + size) % 3]
        if size == 2:
            agents = 1                       # four cells: the whole halo is outside the map
        gc = GridConfig(size=size, num_agents=agents, obs_radius=3, density=0.0 if size == 2 else 0.3, seed=size,
                        collision_system=collision, on_target=on_target, max_episode_steps=256)
        _reset_and_steps(gc, 3, size + k, f"size {size} A={agents} {collision}/{on_target}")


@pytest.mark.parametrize("k,agents", enumerate((1, 6, 13)))
@pytest.mark.parametrize("H,W,batch", [(40, 130, 3), (130, 40, 3), (257, 256, 2)])
def test_rectangular_and_wide_cell_maps(H, W, batch, k, agents):
    """257 x 256 has more than 65536 cells: 4-byte fields.  Its 2, 12 and 26 slots give those kernels a lone tail, full
    4-slot ranges without a tail, and a full 16-slot range followed by a tail."""
    from pogema_amd import GridConfig
    rng = np.random.default_rng(H * 7 + W)
    grid = (rng.random((H, W)) < 0.25).astype(int).tolist()
    collision, on_target = MODES[k]
    gc = GridConfig(map=grid, num_agents=agents, obs_radius=2, seed=6, collision_system=collision, on_target=on_target,
                    max_episode_steps=64)
    _reset_and_steps(gc, batch, 6 + k, f"{H} x {W} A={agents} {collision}/{on_target}")


@pytest.mark.parametrize("radius", [1, 2, 5, 15])
def test_obs_radius(radius):
    """W^2 = 9, 25, 121, 961: never a multiple of 4, so the agents' windows start at every alignment."""
    from pogema_amd import GridConfig
    for k, agents in enumerate((1, 6, 13)):
        collision, on_target = MODES[(k + radius) % 3]
        gc = GridConfig(size=20, num_agents=agents, obs_radius=radius, density=0.3, seed=radius,
                        collision_system=collision, on_target=on_target, max_episode_steps=64)
        _reset_and_steps(gc, 3, radius + k, f"radius {radius} A={agents}", steps=3)


@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=12, num_agents=10, obs_radius=3, density=0.25, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=40)
    env = VecPogema(gc, batch=24, auto_reset=True)
    env.reset(seed=7)
    rng = np.random.default_rng(11)
    inactive_checked = False
    for t in range(16):
        if t % 3 == 0:
            ref = _check(env, what=f"{collision}/{on_target} step {t}")
            active = env.get_state()["is_active"].cpu().numpy()
            inactive_checked |= bool((~active).any())
            assert (ref[~active] == 0).all()
        env.step(mixed_actions(env, rng, p_expert=0.85))
    if on_target == "finish":
        assert inactive_checked, "no finished (hidden) agent was ever checked"
    env.close()


def test_formats_agree():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=24, num_agents=13, obs_radius=4, density=0.3, seed=3), batch=5)
    env.reset(seed=3)
    bits = env.goal_directions(format="bits")
    u8 = env.goal_directions(format="uint8")
    f32 = env.goal_directions()              # the default
    assert f32.dtype == torch.float32
    assert bool(bits.any()) and int(bits.max()) < 16
    shifts = torch.arange(4, device=env.device, dtype=torch.int32).view(1, 1, 4, 1, 1)
    assert torch.equal(u8, ((bits.unsqueeze(2).to(torch.int32) >> shifts) & 1).to(torch.uint8))
    assert torch.equal(f32, u8.to(torch.float32))
    env.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("agents,batch", [(6, 3), (16, 4)])
def test_misaligned_out(fmt, agents, batch):
    """`out` one element past a 16-byte boundary, and the one-byte formats also four bytes past it: the same result as
    an aligned one, nothing written around it."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=16, num_agents=agents, obs_radius=3, density=0.3, seed=5), batch=batch)
    env.reset(seed=5)
    want = env.goal_directions(format=fmt)
    assert want.data_ptr() % 16 == 0
    n = want.numel()
    fill = 7
    for shift in ((1,) if fmt == "float32" else (1, 4)):
        buf = torch.full((n + 8,), fill, dtype=want.dtype, device=env.device)
        assert buf.data_ptr() % 16 == 0
        view = buf[shift:shift + n].view(want.shape)
        assert view.data_ptr() % 16 == shift * want.element_size()
        assert env.goal_directions(format=fmt, out=view) is view
        assert torch.equal(view, want)
        assert bool((buf[:shift] == fill).all()) and bool((buf[shift + n:] == fill).all())
    env.close()


def test_centre_cell_is_the_expert_action():
    from pogema_amd import GridConfig, VecPogema
    for size in (16, 70):
        env = VecPogema(GridConfig(size=size, num_agents=13, obs_radius=3, density=0.3, seed=8, on_target="finish",
                                   max_episode_steps=64), batch=6)
        env.reset(seed=8)
        rng = np.random.default_rng(8)
        r = env.obs_radius
        for _ in range(4):
            centre = env.goal_directions(format="bits")[:, :, r, r].cpu().numpy().astype(np.int64)
            actions, dist = (t.cpu().numpy() for t in env.expert_actions())
            lowest = np.zeros_like(centre)
            for a in (4, 3, 2, 1):
                lowest[(centre >> (a - 1)) & 1 == 1] = a
            assert np.array_equal(lowest, actions)
            assert np.array_equal(centre == 0, dist <= 0)
            env.step(mixed_actions(env, rng, p_expert=0.9))
        env.close()


def test_obstacle_target_gives_all_zero():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=16, num_agents=6, obs_radius=3, density=0.3, seed=9), batch=4)
    env.reset(seed=9)
    maps = installed_maps(env)
    tgt = env.get_state()["targets_xy"].cpu().numpy().copy()
    hit = [(0, 2), (3, 5)]
    for b, i in hit:
        tgt[b, i] = np.argwhere(maps[b] != 0)[0]
    env.set_targets(torch.as_tensor(tgt))
    ref = _check(env, what="obstacle targets")
    got = env.goal_directions(format="bits").cpu().numpy()
    for b, i in hit:
        assert (got[b, i] == 0).all()
    assert ref.any()
    env.close()


def test_cache_contract():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    for size in (16, 80):
        B, A = 5, 6
        gc = GridConfig(size=size, num_agents=A, obs_radius=3, density=0.3, seed=4)
        # a first call on a fresh env allocates the cache and builds every field
        env = VecPogema(gc, batch=B)
        env.reset(seed=4)
        assert env.cost_to_go_builds == 0
        _check(env, what=f"size {size} first call")
        assert env.cost_to_go_builds == B * A
        env.close()
        # after cost_to_go() nothing is left to build; set_targets makes exactly the moved agents' fields stale
        env = VecPogema(gc, batch=B)
        env.reset(seed=4)
        env.cost_to_go()
        assert env.cost_to_go_builds == B * A
        env.goal_directions()
        assert env.cost_to_go_builds == B * A
        tgt = env.get_state()["targets_xy"].cpu().numpy().copy()
        maps = installed_maps(env)
        rng = np.random.default_rng(size)
        moved = [(0, 1), (2, 5), (4, 0)]
        for b, i in moved:
            free = np.argwhere(maps[b] == 0)
            free = free[(free != tgt[b, i]).any(1)]
            tgt[b, i] = free[rng.integers(len(free))]
        env.set_targets(torch.as_tensor(tgt))
        env.goal_directions(format="bits")
        assert env.cost_to_go_builds == B * A + len(moved)
        _check(env, what=f"size {size} after set_targets")
        assert env.cost_to_go_builds == B * A + len(moved)
        env.close()


def test_first_call_inside_capture_is_refused():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=20, num_agents=4, obs_radius=2, density=0.3, seed=12), batch=4)
    env.reset(seed=12)
    out = torch.zeros((4, 4, 4, 5, 5), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError, match="bytes") as ei:
        with torch.cuda.graph(g):
            env.goal_directions(out=out)
    assert ei.value.code == -4
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == 0
    _check(env, what="after the refused capture")
    env.close()


def test_state_untouched():
    """get_state() and the next step()'s outputs are identical with and without a preceding goal_directions()."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    for size, coll, on_target in ((20, "soft", "restart"), (70, "block_both", "finish")):
        gc = GridConfig(size=size, num_agents=13, obs_radius=3, density=0.3, seed=31, collision_system=coll,
                        on_target=on_target, max_episode_steps=32)
        a = VecPogema(gc, batch=6, auto_reset=True, reuse_buffers=False)
        b = VecPogema(gc, batch=6, auto_reset=True, reuse_buffers=False)
        a.reset(seed=31)
        b.reset(seed=31)
        rng = np.random.default_rng(31)
        for t in range(5):
            acts = torch.as_tensor(rng.integers(0, 5, size=(6, 13)), device=a.device)
            before = a.get_state(occupancy=True)
            a.goal_directions(format=FORMATS[t % 3])
            sa, sb = a.get_state(occupancy=True), b.get_state(occupancy=True)
            for k in sa:
                assert torch.equal(sa[k], before[k]) and torch.equal(sa[k], sb[k]), f"size {size} step {t}: {k}"
            assert np.array_equal(installed_maps(a), installed_maps(b))
            ra, rb = a.step(acts), b.step(acts)
            for x, y in zip(ra[:4], rb[:4]):
                assert torch.equal(x, y), f"size {size} step {t}"
        a.close()
        b.close()


@pytest.mark.parametrize("size", [16, 72])
def test_graph_replay_equals_eager(size):
    """goal_directions() captured once after an eager call; replays after further steps (and after new targets, which
    make fields stale) equal the eager result on the same state."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A = 6, 6
    gc = GridConfig(size=size, num_agents=A, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                    on_target="nothing", max_episode_steps=10**6)
    env = VecPogema(gc, batch=B)
    env.reset(seed=4)
    outs = {fmt: torch.zeros_like(env.goal_directions(format=fmt)) for fmt in FORMATS}  # eager: allocates the cache
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fmt in FORMATS:
            env.goal_directions(format=fmt, out=outs[fmt])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for fmt in FORMATS:
            env.goal_directions(format=fmt, out=outs[fmt])
    built = env.cost_to_go_builds
    maps = installed_maps(env)
    for t in range(8):
        a, _ = env.expert_actions()
        env.step(a)
        if t == 4:                           # every agent gets the first or the last free cell, whichever is new to it
            old = env.get_state()["targets_xy"].cpu().numpy()
            free = [np.argwhere(m == 0) for m in maps]
            new = np.stack([np.where((old[b] == free[b][0]).all(-1, keepdims=True), free[b][-1], free[b][0])
                            for b in range(B)])
            env.set_targets(torch.as_tensor(new))
        for o in outs.values():
            o.zero_()
        g.replay()
        if t == 4:
            torch.cuda.synchronize()
            assert env.cost_to_go_builds == built + B * A, "the replay did not rebuild the stale fields"
        for fmt in FORMATS:
            assert torch.equal(outs[fmt], env.goal_directions(format=fmt)), f"step {t} [{fmt}]"
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == built + B * A
    _check(env, what="after replays")
    env.close()


def test_grid_stride_loop():
    """More slot ranges than twice the grid cap in every format, so that every workgroup loops.  The bits format has the
    fewest ranges, 16 slots each; obs_radius 1 on a small map keeps the field cache and the output at a few MB."""
    from pogema_amd import GridConfig, VecPogema
    src = open(os.path.join(ROOT, "pogema_amd", "csrc", "pgx_directions.hip")).read()
    cap = int(re.search(r"DIR_MAX_GRID\s*=\s*(\d+)\s*;", src).group(1))
    B, A = 11001, 6
    assert B * A % 16 and (B * A + 15) // 16 > 2 * cap, "the shape no longer outruns DIR_MAX_GRID twice: raise the batch"
    env = VecPogema(GridConfig(size=6, num_agents=A, obs_radius=1, density=0.2, seed=2, max_episode_steps=64), batch=B)
    env.reset(seed=2)
    _check(env, what="grid-stride reset")
    env.step(mixed_actions(env, np.random.default_rng(2), p_expert=0.7))
    ref = _check(env, what="grid-stride after a step")
    assert ref[-1].any() or ref[-2].any()
    env.close()


def test_out_buffer_list_view_and_errors():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21), batch=6)
    with pytest.raises(PgxError) as ei:
        env.goal_directions()
    assert ei.value.code == -4  # before a reset, like step()
    env.reset(seed=21)
    with pytest.raises(ValueError, match="format"):
        env.goal_directions(format="int32")
    for fmt, dtype, shape in (("float32", torch.float32, (6, 5, 4, 7, 7)), ("uint8", torch.uint8, (6, 5, 4, 7, 7)),
                              ("bits", torch.uint8, (6, 5, 7, 7))):
        d = env.goal_directions(format=fmt)
        assert d.dtype == dtype and tuple(d.shape) == shape
        o = torch.full(shape, 9, dtype=dtype, device=env.device)
        assert env.goal_directions(format=fmt, out=o) is o and torch.equal(o, d)
        wrong = torch.float32 if dtype == torch.uint8 else torch.uint8
        for bad in (torch.empty(shape, dtype=wrong, device=env.device),
                    torch.empty(shape[:-1] + (6,), dtype=dtype, device=env.device),
                    torch.empty(shape[:-1] + (14,), dtype=dtype, device=env.device)[..., ::2],
                    torch.empty(shape, dtype=dtype)):
            with pytest.raises(ValueError):
                env.goal_directions(format=fmt, out=bad)
    # the 7-channel input of DHC-style policies: the observation, then the four planes
    x = torch.cat([env.observe(), env.goal_directions()], dim=2)
    assert x.dtype == torch.float32 and tuple(x.shape) == (6, 5, 7, 7, 7)
    env.close()

    one = pogema_v0(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21))
    one.reset(seed=21)
    views = one.goal_directions()
    assert isinstance(views, list) and len(views) == 5
    assert all(isinstance(v, np.ndarray) and v.shape == (4, 7, 7) and v.dtype == np.uint8 for v in views)
    full = one._vec.goal_directions(format="uint8")[0].cpu().numpy()
    assert all(np.array_equal(views[i], full[i]) for i in range(5))
    assert any(v.any() for v in views)
    one.close()
