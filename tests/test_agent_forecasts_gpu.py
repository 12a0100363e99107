"""GPU: agent forecasts (VecPogema.agent_forecasts / pgx_agent_forecasts, docs/SPEC.md S24) equal the CPU reference
(tests/agent_forecasts_reference.py) bit for bit on get_state() and the installed maps -- the hand-built cases, both
field-build layouts, 2- and 4-byte fields, every collision system and on_target mode, every radius class, more than 32
visible agents, agent counts up to 1024, slot counts that leave a tail -- in all three formats; `planes=False` and offset
views change nothing; the shared field cache follows S11's contract; the engine state is left alone; a graph replay
equals the eager run; the grid-stride loops run."""
import os
import re

import numpy as np
import pytest

from agent_counts import LAYOUT_ROWS, radii_accepted
from agent_forecasts_cases import CASES, expected
from agent_forecasts_reference import agent_forecasts_reference, rows
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("float32", "uint8", "rows")
# one env per line covers every collision system and every on_target mode
MODES = (("priority", "finish"), ("block_both", "restart"), ("soft", "nothing"))


def _reference(env, K, envs=None):
    st = env.get_state()
    return agent_forecasts_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                                     st["is_active"].cpu().numpy(), env.obs_radius, K, envs=envs)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} mismatches, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _as(fmt, planes):
    """The reference's uint8 planes in format `fmt`."""
    return rows(planes) if fmt == "rows" else planes.astype(np.float32 if fmt == "float32" else np.uint8)


def _check(env, what="", steps=(3,), formats=FORMATS):
    """agent_forecasts() == the reference, bit for bit, for every K of `steps` in every format of `formats`.  The
    reference is computed once, for the largest K: the first K steps of a forecast are the K-step forecast.  Returns it."""
    torch = lazy_torch()
    w = env.window
    ref_planes, ref_cells = _reference(env, max(steps))
    for K in steps:
        for fmt in formats:
            planes, cells = env.agent_forecasts(steps=K, format=fmt)
            tag = f"{what} [{fmt}, steps {K}]"
            assert planes.dtype == {"float32": torch.float32, "uint8": torch.uint8, "rows": torch.int32}[fmt]
            assert tuple(planes.shape) == (env.batch, env.num_agents, K, w) + (() if fmt == "rows" else (w,))
            assert cells.dtype == torch.int16 and tuple(cells.shape) == (env.batch, env.num_agents, K, 2)
            _same(planes, _as(fmt, ref_planes[:, :, :K]), tag + " planes")
            _same(cells, ref_cells[:, :, :K], tag + " cells")
    return ref_planes, ref_cells


def _reset_and_steps(gc, batch, seed, what, steps=4, ks=(3,)):
    from pogema_amd import VecPogema
    env = VecPogema(gc, batch=batch)
    env.reset(seed=seed)
    rng = np.random.default_rng(seed)
    _check(env, what=f"{what} reset", steps=ks)
    for _ in range(steps):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    ref = _check(env, what=f"{what} after {steps} steps", steps=ks)
    env.close()
    return ref


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_shared_cases(case):
    """The hand-built cases, installed through GridConfig(map, agents_xy, targets_xy) at batch 2: all three formats with
    K = 1, 3 and 8 against the reference, and with the case's own K against the arrays the case writes out."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(map="\n".join(case["map"]), agents_xy=case.get("start_xy", case["agents_xy"]),
                    targets_xy=case["targets_xy"], obs_radius=case["r"],
                    on_target="finish" if "actions" in case else "nothing", max_episode_steps=64)
    env = VecPogema(gc, batch=2)
    env.reset(seed=0)
    if "actions" in case:
        env.step(torch.as_tensor([case["actions"]] * 2, device=env.device))
    assert env.get_state()["is_active"][0].cpu().numpy().astype(bool).tolist() == case["is_active"]
    _check(env, what=case["name"], steps=(1, 3, 8))
    want_planes, want_cells = expected(case)
    for fmt in FORMATS:
        planes, cells = env.agent_forecasts(steps=case["steps"], format=fmt)
        for b in range(2):
            _same(planes[b], _as(fmt, want_planes), f"{case['name']} [{fmt}] planes")
            _same(cells[b], want_cells, f"{case['name']} [{fmt}] cells")
    env.close()


# sides 64 and 65 switch between the two field-build layouts; with batch 3 the slot counts 3, 18 and 39 are no multiple
# of 16, so that every call ends in the tail path
@pytest.mark.parametrize("size", [2, 8, 33, 64, 65])
def test_square_maps_match_reference(size):
    from pogema_amd import GridConfig
    for k, agents in enumerate((1, 6, 13)):
        collision, on_target = MODES[(k + size) % 3]
        if size == 2:
            agents = 1                       # four cells: every step looks outside the map
        gc = GridConfig(size=size, num_agents=agents, obs_radius=3, density=0.0 if size == 2 else 0.3, seed=size,
                        collision_system=collision, on_target=on_target, max_episode_steps=256)
        _reset_and_steps(gc, 3, size + k, f"size {size} A={agents} {collision}/{on_target}", ks=(3, 8) if k == 2 else (3,))


def test_wide_cell_map():
    """257 x 256 has more than 65536 cells: 4-byte fields."""
    from pogema_amd import GridConfig
    rng = np.random.default_rng(257 * 7 + 256)
    grid = (rng.random((257, 256)) < 0.25).astype(int).tolist()
    gc = GridConfig(map=grid, num_agents=6, obs_radius=2, seed=6, collision_system="block_both", on_target="restart",
                    max_episode_steps=64)
    planes, cells = _reset_and_steps(gc, 2, 7, "257 x 256", ks=(8,))
    assert (cells[:, :, 0] != cells[:, :, -1]).any()


@pytest.mark.parametrize("radius", [1, 2, 5, 15])
def test_obs_radius(radius):
    """W = 3, 5, 11, 31: the planes and the row words start at every alignment, and the ranges of the gather hold 64
    slots or, at W = 31 with K = 8, 32."""
    from pogema_amd import GridConfig
    for k, agents in enumerate((1, 6, 13)):
        collision, on_target = MODES[(k + radius) % 3]
        gc = GridConfig(size=20, num_agents=agents, obs_radius=radius, density=0.3, seed=radius,
                        collision_system=collision, on_target=on_target, max_episode_steps=64)
        planes, _ = _reset_and_steps(gc, 3, radius + k, f"radius {radius} A={agents}", steps=3, ks=(3, 8) if k == 2 else (3,))
    assert planes.any() or radius == 1


def test_bit_30_of_a_row_word_and_never_the_sign_bit():
    """obs_radius 15: agent 1 walks down column 15 of an open 20 x 20 map, 15 columns to the right of agent 0, which draws
    it in bit 30 of its row words; agent 0 walks down column 0, which agent 1 draws in bit 0."""
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(map="\n".join(["." * 20] * 20), agents_xy=[[10, 0], [5, 15]], targets_xy=[[13, 0], [9, 15]],
                    obs_radius=15, on_target="nothing", max_episode_steps=64)
    env = VecPogema(gc, batch=2)
    env.reset(seed=0)
    ref_planes, ref_cells = _check(env, what="bit 30", steps=(3, 8))
    assert ref_cells[0, 1, :4].tolist() == [[6, 15], [7, 15], [8, 15], [9, 15]]
    words = env.agent_forecasts(steps=8, format="rows")[0].cpu().numpy()
    assert (words[:, 0] == 1 << 30).sum() == 2 * 8 and (words[:, 1] & 1).any() and (words >= 0).all()
    env.close()


def test_more_than_32_visible_agents():
    """40 agents on 8 x 8 with obs_radius 7: every window holds the whole map, every observer sees 39 agents -- more
    than a visible_agents() list holds -- and every one of them is drawn."""
    from pogema_amd import GridConfig
    rng = np.random.default_rng(40)
    grid = (rng.random((8, 8)) < 0.1).astype(int)
    free = np.argwhere(grid == 0)
    # (the random placement wants 2 x 40 distinct cells, more than the map has: targets may lie on other agents' starts)
    gc = GridConfig(map=grid.tolist(), agents_xy=free[rng.permutation(len(free))[:40]].tolist(),
                    targets_xy=free[rng.permutation(len(free))[:40]].tolist(), obs_radius=7, collision_system="soft",
                    on_target="nothing", max_episode_steps=64)
    planes, cells = _reset_and_steps(gc, 2, 40, "40 agents", steps=2, ks=(3,))
    assert (cells >= 0).all(), "all 40 are active, and 39 > 32 of them stand in every window"
    for i in (0, 39):
        others = np.delete(cells[0, :, 0], i, axis=0)
        assert planes[0, i, 0].sum() == len({tuple(c) for c in others.tolist()})


def test_one_row_of_300_agents():
    from pogema_amd import GridConfig
    gc = GridConfig(size=32, num_agents=300, obs_radius=2, density=0.2, seed=30, collision_system="soft",
                    on_target="nothing", max_episode_steps=64)
    planes, _ = _reset_and_steps(gc, 2, 30, "300 agents", steps=2)
    assert planes.any()


@pytest.mark.parametrize("agents,size,batch", [LAYOUT_ROWS[0], (1024, 64, 2)])
def test_many_agents(agents, size, batch):
    """257 and 1024 agents on tests/agent_counts.py's maps, at the radii the engine admits: the lanes of a wave stride
    over an env's agents 5 and 16 times."""
    from pogema_amd import GridConfig, VecPogema
    assert agents in (257, 1024)
    radii = radii_accepted(agents, size, batch)
    assert radii == ((1, 5, 15) if agents == 257 else (1, 5))
    rng = np.random.default_rng(agents)
    for r in radii:
        gc = GridConfig(size=size, num_agents=agents, obs_radius=r, density=0.1, seed=agents + r,
                        collision_system="soft", on_target="finish", max_episode_steps=64)
        env = VecPogema(gc, batch=batch)
        env.reset(seed=agents + r)
        if r == radii[-1]:
            for _ in range(2):
                env.step(mixed_actions(env, rng, p_expert=0.8))
        planes, _ = _check(env, what=f"A={agents} r={r}", steps=(2,), formats=(FORMATS[r % 3],))
        assert planes.any()
        env.close()


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "pogema_amd", "csrc", "pgx_agent_forecasts.hip")).read()
    return int(re.search(rf"{name}\s*=\s*(\d+)\s*;", src).group(1))


def test_many_ranges_and_a_tail():
    """200 x 13 = 2600 slots: 40 full ranges of the gather and a tail of 40 slots, 10 full ranges of the walk and a tail
    of 40: no multiple of 16."""
    from pogema_amd import GridConfig, VecPogema
    B, A = 200, 13
    slots, walk = _kernel_constant("FC_SLOTS"), _kernel_constant("WALK_SLOTS")
    assert slots % 16 == 0 and B * A > 8 * walk and B * A % slots % 16 and B * A % walk % 16
    env = VecPogema(GridConfig(size=8, num_agents=A, obs_radius=2, density=0.1, seed=2, max_episode_steps=64), batch=B)
    env.reset(seed=2)
    _check(env, what="many ranges reset")
    env.step(mixed_actions(env, np.random.default_rng(2), p_expert=0.7))
    planes, _ = _check(env, what="many ranges after a step", steps=(2,))
    assert planes[-1].any() or planes[-2].any()
    env.close()


def _torch_composition(env, K):
    """The same result from what the engine exports otherwise, on the device, for K <= obs_radius + 1 (the walk stays
    inside the agent's own goal_directions() window, whose masks are exact up to its edge): K rounds of gather and
    compare over the masks for the cells, a pairwise visibility test and one scatter for the planes.  Returns
    (planes uint8 [B, A, K, w, w], cells int16 [B, A, K, 2])."""
    torch = lazy_torch()
    B, A, w, r = env.batch, env.num_agents, env.window, env.obs_radius
    assert K <= r + 1
    dev = env.device
    st = env.get_state()
    pos, active = st["agents_xy"].long(), st["is_active"].bool()
    flat = env.goal_directions(format="bits").view(B * A, w * w).long()
    delta = torch.zeros((16, 2), dtype=torch.int64, device=dev)            # by the mask's lowest bit: the move's (du, dv)
    for low, d in ((1, (-1, 0)), (2, (1, 0)), (4, (0, -1)), (8, (0, 1))):
        delta[low] = torch.tensor(d)
    u = torch.full((B * A,), r, dtype=torch.int64, device=dev)
    v = u.clone()
    cells = []
    for _ in range(K):
        m = flat.gather(1, (u * w + v).unsqueeze(1)).squeeze(1)
        d = delta[m & -m]
        u, v = u + d[:, 0], v + d[:, 1]
        cells.append(pos + torch.stack((u - r, v - r), -1).view(B, A, 2))
    cells = torch.stack(cells, 2)                                                 # [B, A, K, 2]
    cells = torch.where(active.view(B, A, 1, 1), cells, torch.full_like(cells, -1))
    off = pos.view(B, 1, A, 2) - pos.view(B, A, 1, 2)                             # [b, i, j]: j seen from i
    seen = (off.abs() <= r).all(-1) & active.view(B, A, 1) & active.view(B, 1, A) & ~torch.eye(A, dtype=torch.bool, device=dev)
    rel = cells.view(B, 1, A, K, 2) - pos.view(B, A, 1, 1, 2) + r                 # [b, i, j, s]: window cell of q_j(s)
    inside = ((rel >= 0) & (rel < w)).all(-1) & seen.unsqueeze(-1)
    b, i, _, s = torch.nonzero(inside, as_tuple=True)
    uv = rel[inside]
    planes = torch.zeros((B, A, K, w, w), dtype=torch.uint8, device=dev)
    planes[b, i, s, uv[:, 0], uv[:, 1]] = 1
    return planes, cells.to(torch.int16)


def test_grid_stride_loops():
    """More ranges than the grid cap in both launches, so that workgroups loop: 41000 x 13 slots on 8 x 8 maps with
    obs_radius 1 and K = 2 keep the field cache and the outputs at some tens of MB.  The whole batch is compared on the
    device with the torch composition, and the first two and the last two envs, which the first and the last workgroups
    hold, with the CPU reference."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A, K = 41000, 13, 2
    slots, walk, cap = _kernel_constant("FC_SLOTS"), _kernel_constant("WALK_SLOTS"), _kernel_constant("FC_MAX_GRID")
    assert B * A % slots and (B * A + slots - 1) // slots > cap and (B * A + walk - 1) // walk > cap, \
        "the shape no longer outruns FC_MAX_GRID: raise the batch"
    env = VecPogema(GridConfig(size=8, num_agents=A, obs_radius=1, density=0.1, seed=2, max_episode_steps=64), batch=B)
    env.reset(seed=2)
    env.step(mixed_actions(env, np.random.default_rng(2), p_expert=0.7))
    w = env.window
    planes, cells = _torch_composition(env, K)
    assert bool(planes[-1].any()) or bool(planes[-2].any())
    ends = [0, 1, B - 2, B - 1]
    ref_planes, ref_cells = _reference(env, K, envs=ends)
    for fmt in FORMATS:
        got = env.agent_forecasts(steps=K, format=fmt)
        if fmt == "rows":
            bit = torch.arange(w, device=env.device)
            want = (planes.int() << bit).sum(-1).to(torch.int32)
        else:
            want = planes.to(got[0].dtype)
        assert torch.equal(got[0], want) and torch.equal(got[1], cells)
        for b in ends:
            _same(got[0][b], _as(fmt, ref_planes[b]), f"grid-stride env {b} [{fmt}] planes")
            _same(got[1][b], ref_cells[b], f"grid-stride env {b} [{fmt}] cells")
    env.close()


def test_inactive_agents_and_ghosts():
    """on_target="finish": agents that arrived are hidden, have no forecast and are not drawn; `soft`: an agent that
    is missing from the occupancy array (a ghost) forecasts, is drawn and observes like every active agent."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=8, num_agents=12, obs_radius=2, density=0.1, seed=5, on_target="finish",
                               max_episode_steps=1000), batch=8)
    env.reset(seed=5)
    for _ in range(6):
        env.step(env.expert_actions()[0])
    active = env.get_state()["is_active"].cpu().numpy().astype(bool)
    assert (~active).any() and active.any()
    planes, cells = _check(env, what="finish")
    assert (cells[~active] == -1).all() and not planes[~active].any() and (cells[active] >= 0).all() and planes.any()
    env.close()
    # tests/test_policy_input_gpu.py's ghost hunt
    env = VecPogema(GridConfig(size=8, num_agents=12, obs_radius=2, density=0.1, seed=5, collision_system="soft",
                               on_target="nothing", max_episode_steps=1000), batch=8)
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
    _check(env, what=f"soft, {ghosts} ghosts after {t + 1} steps")
    env.close()


def test_planes_false_gives_the_same_cells():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=24, num_agents=13, obs_radius=4, density=0.3, seed=3), batch=5)
    env.reset(seed=3)
    for K in (1, 3, 8):
        _, cells = env.agent_forecasts(steps=K)
        for fmt in FORMATS:
            none, c2 = env.agent_forecasts(steps=K, format=fmt, planes=False)
            assert none is None and torch.equal(c2, cells)
        co = torch.full_like(cells, 9)
        got = env.agent_forecasts(steps=K, planes=False, out=(co,))
        assert got[0] is None and got[1] is co and torch.equal(co, cells)
    with pytest.raises(ValueError, match="out must be"):
        env.agent_forecasts(planes=False, out=(cells, cells))
    env.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("agents,batch", [(6, 3), (16, 4)])
def test_offset_views(fmt, agents, batch):
    """`planes` as a view one element past a 16-byte boundary (uint8 planes also four) and `cells` one int16 (2 bytes)
    past one: the same result as fresh tensors, nothing written around them."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=16, num_agents=agents, obs_radius=3, density=0.3, seed=5), batch=batch)
    env.reset(seed=5)
    want = env.agent_forecasts(format=fmt)
    assert want[0].data_ptr() % 16 == 0 and bool(want[0].any())
    fill = 7
    for shift in ((1, 4) if fmt == "uint8" else (1,)):
        bufs, views = [], []
        for t, sh in zip(want, (shift, 1)):
            buf = torch.full((t.numel() + 8,), fill, dtype=t.dtype, device=env.device)
            assert buf.data_ptr() % 16 == 0
            bufs.append(buf)
            views.append(buf[sh:sh + t.numel()].view(t.shape))
        assert views[1].data_ptr() % 16 == 2
        got = env.agent_forecasts(format=fmt, out=tuple(views))
        for g, v, t, buf, sh in zip(got, views, want, bufs, (shift, 1)):
            assert g is v and torch.equal(v, t)
            assert bool((buf[:sh] == fill).all()) and bool((buf[sh + t.numel():] == fill).all())
    env.close()


def test_out_buffers_list_view_and_errors():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21), batch=6)
    with pytest.raises(PgxError) as ei:
        env.agent_forecasts()
    assert ei.value.code == -4  # before a reset, like step()
    env.reset(seed=21)
    with pytest.raises(ValueError, match="format"):
        env.agent_forecasts(format="bits")
    for bad in (0, -1, 9, 2.0, True, "3", None):
        with pytest.raises(ValueError, match=r"1\.\.8"):
            env.agent_forecasts(steps=bad)
    env.agent_forecasts(steps=8)
    K = 2
    cells = torch.empty((6, 5, K, 2), dtype=torch.int16, device=env.device)
    for fmt, dtype, shape in (("float32", torch.float32, (6, 5, K, 7, 7)), ("uint8", torch.uint8, (6, 5, K, 7, 7)),
                              ("rows", torch.int32, (6, 5, K, 7))):
        want = env.agent_forecasts(steps=K, format=fmt)
        o = torch.full(shape, 9, dtype=dtype, device=env.device)
        got = env.agent_forecasts(steps=K, format=fmt, out=(o, cells))
        assert got[0] is o and got[1] is cells
        assert all(torch.equal(g, t) for g, t in zip(got, want))
        wrong = torch.float32 if dtype != torch.float32 else torch.uint8
        for bad in (torch.empty(shape, dtype=wrong, device=env.device),
                    torch.empty(shape[:-1] + (6,), dtype=dtype, device=env.device),
                    torch.empty(shape[:-1] + (14,), dtype=dtype, device=env.device)[..., ::2],
                    torch.empty((6, 5, 3) + shape[3:], dtype=dtype, device=env.device),
                    torch.empty(shape, dtype=dtype)):
            with pytest.raises(ValueError, match=r"out\[planes\]"):
                env.agent_forecasts(steps=K, format=fmt, out=(bad, cells))
        for bad in (cells.to(torch.int32), cells[:, :4], torch.empty((6, 5, 3, 2), dtype=torch.int16, device=env.device)):
            with pytest.raises(ValueError, match=r"out\[cells\]"):
                env.agent_forecasts(steps=K, format=fmt, out=(o, bad))
        with pytest.raises(ValueError, match="out must be"):
            env.agent_forecasts(steps=K, format=fmt, out=(o,))
        with pytest.raises(ValueError, match=r"out\[planes\] is None"):
            env.agent_forecasts(steps=K, format=fmt, out=(None, cells))
    env.close()

    one = pogema_v0(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21))
    one.reset(seed=21)
    views = one.agent_forecasts()
    assert isinstance(views, list) and len(views) == 5
    full = [t[0].cpu().numpy() for t in one._vec.agent_forecasts(format="uint8")]
    for i, (planes, xy) in enumerate(views):
        assert isinstance(planes, np.ndarray) and planes.shape == (3, 7, 7) and planes.dtype == np.uint8
        assert np.array_equal(planes, full[0][i])
        assert isinstance(xy, list) and len(xy) == 3 and xy == [tuple(int(v) for v in c) for c in full[1][i]]
        assert all(type(c) is tuple and all(type(v) is int for v in c) for c in xy)
    assert len(one.agent_forecasts(steps=1)[0][1]) == 1 and one.agent_forecasts(steps=1)[0][0].shape == (1, 7, 7)
    one.close()


def test_cache_contract():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    for size in (16, 80):
        B, A = 5, 6
        gc = GridConfig(size=size, num_agents=A, obs_radius=3, density=0.3, seed=4)
        # a first call on a fresh env allocates the cache and builds every field; a second one builds nothing
        env = VecPogema(gc, batch=B)
        env.reset(seed=4)
        assert env.cost_to_go_builds == 0
        env.agent_forecasts(planes=False)
        assert env.cost_to_go_builds == B * A
        _check(env, what=f"size {size} second call")
        assert env.cost_to_go_builds == B * A
        env.close()
        # the cache is cost_to_go()'s: after it nothing is left to build; set_targets makes the moved agents' fields stale
        env = VecPogema(gc, batch=B)
        env.reset(seed=4)
        env.cost_to_go()
        assert env.cost_to_go_builds == B * A
        env.agent_forecasts()
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
        env.agent_forecasts(format="rows")
        assert env.cost_to_go_builds == B * A + len(moved)
        _check(env, what=f"size {size} after set_targets")
        env.cost_to_go()
        assert env.cost_to_go_builds == B * A + len(moved)
        env.close()


def test_regenerated_pool_maps_and_copies():
    """A map-pool regenerate installs other maps and a copy_envs other states: the forecasts follow both, also from a
    graph captured before."""
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
    outs = tuple(torch.zeros_like(t) for t in env.agent_forecasts(format="uint8"))   # eager: allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.agent_forecasts(format="uint8", out=outs)
    for _ in range(7):                       # two episode ends per env
        env.step(torch.as_tensor(rng.integers(0, 5, size=(12, 4)), device=env.device))
    assert (env.map_index.cpu().numpy() != first).any(), "no env drew another map: the first reset's maps would pass"
    want = _check(env, what="after regeneration", formats=("uint8",))
    g.replay()
    for o, t in zip(outs, want):
        _same(o, t, "replay after regeneration")
    env.step(torch.as_tensor(rng.integers(1, 5, size=(12, 4)), device=env.device))
    before = env.agent_forecasts(format="uint8")
    src, dst = [0, 1, 2], [5, 6, 7]
    assert not torch.equal(before[1][src], before[1][dst])
    env.copy_envs(src, dst)
    want = _check(env, what="after copy_envs", formats=("uint8",))
    assert np.array_equal(want[1][dst], before[1][src].cpu().numpy()) and np.array_equal(want[0][dst], before[0][src].cpu().numpy())
    g.replay()
    for o, t in zip(outs, want):
        _same(o, t, "replay after copy_envs")
    env.close()


def test_first_call_inside_capture_is_refused():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=20, num_agents=4, obs_radius=2, density=0.3, seed=12), batch=4)
    env.reset(seed=12)
    out = (torch.zeros((4, 4, 3, 5, 5), dtype=torch.float32, device="cuda"),
           torch.zeros((4, 4, 3, 2), dtype=torch.int16, device="cuda"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError, match="bytes") as ei:
        with torch.cuda.graph(g):
            env.agent_forecasts(out=out)
    assert ei.value.code == -4
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == 0
    _check(env, what="after the refused capture")
    env.close()


def test_following_the_expert_visits_the_cells():
    """One agent per env under on_target="nothing": K steps of expert_actions() visit cells[0..K-1]."""
    from pogema_amd import GridConfig, VecPogema
    K = 8
    env = VecPogema(GridConfig(size=16, num_agents=1, obs_radius=3, density=0.3, seed=17, on_target="nothing",
                               max_episode_steps=10**6), batch=24)
    env.reset(seed=17)
    planes, cells = (t.cpu().numpy() for t in env.agent_forecasts(steps=K, format="uint8"))
    assert not planes.any(), "nobody else is there"
    p0 = env.get_state()["agents_xy"].cpu().numpy()
    assert (cells[:, 0, 0] != p0[:, 0]).any() and (cells[:, 0, -1] == cells[:, 0, -2]).all(-1).any(), "some move, some have arrived"
    for s in range(K):
        env.step(env.expert_actions()[0])
        assert np.array_equal(env.get_state()["agents_xy"].cpu().numpy()[:, 0], cells[:, 0, s]), f"step {s + 1}"
    env.close()


def test_state_untouched():
    """get_state() and the next step()'s outputs are identical with and without a preceding agent_forecasts()."""
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
            a.agent_forecasts(steps=(1, 3, 8)[t % 3], format=FORMATS[t % 3], planes=t != 3)
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
    """agent_forecasts() captured once after an eager call, on one stream; replays after further steps (and after new
    targets, which make fields stale) equal the eager result on the same state."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A = 6, 6
    gc = GridConfig(size=size, num_agents=A, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                    on_target="nothing", max_episode_steps=10**6)
    env = VecPogema(gc, batch=B)
    env.reset(seed=4)
    outs = tuple(torch.zeros_like(t) for t in env.agent_forecasts(format="rows"))  # eager: allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.agent_forecasts(format="rows", out=outs)
    built = env.cost_to_go_builds
    maps = installed_maps(env)
    for t in range(6):
        a, _ = env.expert_actions()
        env.step(a)
        if t == 3:                           # every agent gets the first or the last free cell, whichever is new to it
            old = env.get_state()["targets_xy"].cpu().numpy()
            free = [np.argwhere(m == 0) for m in maps]
            new = np.stack([np.where((old[b] == free[b][0]).all(-1, keepdims=True), free[b][-1], free[b][0])
                            for b in range(B)])
            env.set_targets(torch.as_tensor(new))
        for o in outs:
            o.zero_()
        g.replay()
        if t == 3:
            torch.cuda.synchronize()
            assert env.cost_to_go_builds == built + B * A, "the replay did not rebuild the stale fields"
        for o, e in zip(outs, env.agent_forecasts(format="rows")):
            assert torch.equal(o, e), f"step {t}"
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == built + B * A
    _check(env, what="after replays")
    env.close()
