"""GPU: path-to-goal planes and sub-goals (VecPogema.goal_paths / pgx_goal_paths, docs/SPEC.md S22) equal the CPU
reference (tests/goal_paths_reference.py) bit for bit on get_state() and the installed maps -- the hand-built cases, both
field-build layouts, 2- and 4-byte fields, every collision system and on_target mode, slot counts that leave a tail --
in all three formats, capped and uncapped; `planes=False` and offset views change nothing; the shared field cache follows
S11's contract; the identities with expert_actions() and cost_to_go() hold; the engine state is left alone; a graph
replay equals the eager run; the grid-stride loop runs."""
import os
import re

import numpy as np
import pytest

from goal_paths_cases import CASES, expected
from goal_paths_reference import goal_paths_reference, rows
from util import installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("float32", "uint8", "rows")
# one env per line covers every collision system and every on_target mode
MODES = (("priority", "finish"), ("block_both", "restart"), ("soft", "nothing"))


def _reference(env, steps=None):
    st = env.get_state()
    return goal_paths_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                                st["is_active"].cpu().numpy(), env.obs_radius, steps=steps)


def _reference_envs(env, envs):
    """The reference of these environments alone (the other rows are zero)."""
    st = env.get_state()
    return goal_paths_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                                st["is_active"].cpu().numpy(), env.obs_radius, envs=envs)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} mismatches, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def _check(env, what="", steps=(None,), formats=FORMATS):
    """goal_paths() == the reference, bit for bit, for every cap of `steps` in every format of `formats`; returns the
    reference of the last cap."""
    torch = lazy_torch()
    w = env.window
    for cap in steps:
        ref_planes, ref_subgoal, ref_length = ref = _reference(env, cap)
        for fmt in formats:
            planes, subgoal, length = env.goal_paths(steps=cap, format=fmt)
            tag = f"{what} [{fmt}, steps {cap}]"
            assert planes.dtype == {"float32": torch.float32, "uint8": torch.uint8, "rows": torch.int32}[fmt]
            assert tuple(planes.shape) == (env.batch, env.num_agents, w) + (() if fmt == "rows" else (w,))
            _same(planes, rows(ref_planes) if fmt == "rows" else ref_planes.astype(np.float32 if fmt == "float32" else np.uint8),
                  tag + " planes")
            _same(subgoal, ref_subgoal, tag + " subgoal")
            _same(length, ref_length, tag + " length")
    return ref


def _reset_and_steps(gc, batch, seed, what, steps=4):
    from pogema_amd import VecPogema
    env = VecPogema(gc, batch=batch)
    env.reset(seed=seed)
    rng = np.random.default_rng(seed)
    _check(env, what=f"{what} reset", steps=(None, 3))
    for _ in range(steps):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    ref = _check(env, what=f"{what} after {steps} steps", steps=(3, None))
    env.close()
    return ref


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_shared_cases(case):
    """The hand-built cases, installed through GridConfig(map, agents_xy, targets_xy): all three formats with steps
    None, 1 and 3 against the reference, and with the case's own cap against the arrays the case writes out."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(map="\n".join(case["map"]), agents_xy=case.get("start_xy", case["agents_xy"]),
                    targets_xy=case["targets_xy"], obs_radius=case["r"], on_target="finish", max_episode_steps=64)
    env = VecPogema(gc, batch=2)
    env.reset(seed=0)
    if "actions" in case:
        env.step(torch.as_tensor([case["actions"]] * 2, device=env.device))
        assert env.get_state()["is_active"][0].cpu().numpy().astype(bool).tolist() == case["is_active"]
    _check(env, what=case["name"], steps=(None, 1, 3))
    want = expected(case)
    for fmt in FORMATS:
        planes, subgoal, length = env.goal_paths(steps=case["steps"], format=fmt)
        for b in range(2):
            _same(planes[b], rows(want[0]) if fmt == "rows" else want[0].astype(np.float32 if fmt == "float32" else np.uint8),
                  f"{case['name']} [{fmt}] planes")
            _same(subgoal[b], want[1], f"{case['name']} [{fmt}] subgoal")
            _same(length[b], want[2], f"{case['name']} [{fmt}] length")
    env.close()


# sides 64 and 65 switch between the two field-build layouts; with batch 3 the slot counts 3, 18 and 39 are no multiple
# of 4 or 16, so that every call ends in the tail path
@pytest.mark.parametrize("size", [2, 8, 33, 64, 65])
def test_square_maps_match_reference(size):
    from pogema_amd import GridConfig
    for k, agents in enumerate((1, 6, 13)):
        collision, on_target = MODES[(k + size) % 3]
        if size == 2:
            agents = 1                       # four cells: the whole halo is outside the map
        gc = GridConfig(size=size, num_agents=agents, obs_radius=3, density=0.0 if size == 2 else 0.3, seed=size,
                        collision_system=collision, on_target=on_target, max_episode_steps=256)
        _reset_and_steps(gc, 3, size + k, f"size {size} A={agents} {collision}/{on_target}")


def test_wide_cell_map():
    """257 x 256 has more than 65536 cells: 4-byte fields.  12 slots: full 4-slot ranges, a lone 16-slot tail."""
    from pogema_amd import GridConfig
    rng = np.random.default_rng(257 * 7 + 256)
    grid = (rng.random((257, 256)) < 0.25).astype(int).tolist()
    gc = GridConfig(map=grid, num_agents=6, obs_radius=2, seed=6, collision_system="block_both", on_target="restart",
                    max_episode_steps=64)
    ref = _reset_and_steps(gc, 2, 7, "257 x 256")
    assert ref[2].any()


@pytest.mark.parametrize("radius", [1, 2, 5, 15])
def test_obs_radius(radius):
    """W = 3, 5, 11, 31: the windows and the row masks start at every alignment; 31 fills a row word up to bit 30."""
    from pogema_amd import GridConfig
    for k, agents in enumerate((1, 6, 13)):
        collision, on_target = MODES[(k + radius) % 3]
        gc = GridConfig(size=20, num_agents=agents, obs_radius=radius, density=0.3, seed=radius,
                        collision_system=collision, on_target=on_target, max_episode_steps=64)
        ref = _reset_and_steps(gc, 3, radius + k, f"radius {radius} A={agents}", steps=3)
    if radius == 15:
        assert ref[2].max() > 3, "the whole map is inside the window: some path is longer than the cap of the other calls"


def test_one_row_of_300_agents():
    from pogema_amd import GridConfig
    gc = GridConfig(size=32, num_agents=300, obs_radius=2, density=0.2, seed=30, collision_system="soft",
                    on_target="nothing", max_episode_steps=64)
    ref = _reset_and_steps(gc, 2, 30, "300 agents", steps=2)
    assert ref[2].any()


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "pogema_amd", "csrc", "pgx_goal_paths.hip")).read()
    return int(re.search(rf"{name}\s*=\s*(\d+)\s*;", src).group(1))


def test_many_ranges_and_a_tail():
    """700 x 13 = 9100 slots: 35 full ranges of the kernel and a tail of 140 slots that is no multiple of 16."""
    from pogema_amd import GridConfig, VecPogema
    B, A = 700, 13
    slots = _kernel_constant("PATH_SLOTS")
    assert B * A > 8 * slots and B * A % slots % 16
    env = VecPogema(GridConfig(size=8, num_agents=A, obs_radius=2, density=0.1, seed=2, max_episode_steps=64), batch=B)
    env.reset(seed=2)
    _check(env, what="many ranges reset")
    env.step(mixed_actions(env, np.random.default_rng(2), p_expert=0.7))
    ref = _check(env, what="many ranges after a step", steps=(2,))
    assert ref[2][-1].any() or ref[2][-2].any()
    env.close()


def test_grid_stride_loop():
    """More ranges than the grid cap, so that workgroups loop: 41000 x 13 slots on 8 x 8 maps with obs_radius 1 keep the
    field cache and the outputs at some tens of MB.  The whole batch is compared on the device with the composition of
    goal_directions("bits") -- W^2 - 1 = 8 rounds of gather, compare and scatter state the uncapped walk -- and the first
    and the last envs, which the first and the last workgroup hold, with the CPU reference."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A = 41000, 13
    slots, cap = _kernel_constant("PATH_SLOTS"), _kernel_constant("PATH_MAX_GRID")
    assert B * A % slots and (B * A + slots - 1) // slots > cap, "the shape no longer outruns PATH_MAX_GRID: raise the batch"
    env = VecPogema(GridConfig(size=8, num_agents=A, obs_radius=1, density=0.1, seed=2, max_episode_steps=64), batch=B)
    env.reset(seed=2)
    env.step(mixed_actions(env, np.random.default_rng(2), p_expert=0.7))
    w, r, n = env.window, env.obs_radius, B * A
    flat = env.goal_directions(format="bits").view(n, w * w).long()
    delta = torch.zeros((16, 2), dtype=torch.int64, device=env.device)     # by the mask's lowest bit: the move's (du, dv)
    for low, d in ((1, (-1, 0)), (2, (1, 0)), (4, (0, -1)), (8, (0, 1))):
        delta[low] = torch.tensor(d)
    u = torch.full((n,), r, dtype=torch.int64, device=env.device)
    v, length, alive = u.clone(), torch.zeros_like(u), torch.ones_like(u, dtype=torch.bool)
    planes = torch.zeros((n, w * w), dtype=torch.uint8, device=env.device)
    for _ in range(w * w - 1):
        m = flat.gather(1, (u * w + v).unsqueeze(1)).squeeze(1)
        d = delta[m & -m]
        nu, nv = u + d[:, 0], v + d[:, 1]
        alive = alive & (m != 0) & (nu >= 0) & (nu < w) & (nv >= 0) & (nv < w)
        u, v = torch.where(alive, nu, u), torch.where(alive, nv, v)
        at = (u * w + v).unsqueeze(1)            # (an agent that has stopped rewrites the cell under its cursor as it is)
        planes.scatter_(1, at, torch.where(alive.unsqueeze(1), 1, planes.gather(1, at)).to(torch.uint8))
        length += alive
    subgoal = torch.stack((u - r, v - r), -1).to(torch.int8).view(B, A, 2)
    assert bool(length.view(B, A)[-1].any()) or bool(length.view(B, A)[-2].any())
    ref = _reference_envs(env, [0, 1, B - 2, B - 1])
    for fmt in FORMATS:
        got = env.goal_paths(format=fmt)
        if fmt == "rows":
            bit = torch.arange(w, device=env.device)
            want = (planes.view(B, A, w, w).int() << bit).sum(-1).to(torch.int32)
        else:
            want = planes.view(B, A, w, w).to(got[0].dtype)
        assert torch.equal(got[0], want) and torch.equal(got[1], subgoal) and torch.equal(got[2], length.view(B, A).int())
        for b in (0, 1, B - 2, B - 1):
            _same(got[0][b], rows(ref[0][b]) if fmt == "rows" else ref[0][b].astype(np.float32 if fmt == "float32" else np.uint8),
                  f"grid-stride env {b} [{fmt}] planes")
            _same(got[1][b], ref[1][b], f"grid-stride env {b} [{fmt}] subgoal")
            _same(got[2][b], ref[2][b], f"grid-stride env {b} [{fmt}] length")
    env.close()


def test_planes_false_gives_the_same_subgoals_and_lengths():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=24, num_agents=13, obs_radius=4, density=0.3, seed=3), batch=5)
    env.reset(seed=3)
    for cap in (None, 2):
        _, subgoal, length = env.goal_paths(steps=cap)
        for fmt in FORMATS:
            none, s2, l2 = env.goal_paths(steps=cap, format=fmt, planes=False)
            assert none is None and torch.equal(s2, subgoal) and torch.equal(l2, length)
        so, lo = torch.full_like(subgoal, 9), torch.full_like(length, 9)
        got = env.goal_paths(steps=cap, planes=False, out=(so, lo))
        assert got[0] is None and got[1] is so and got[2] is lo and torch.equal(so, subgoal) and torch.equal(lo, length)
    assert bool(length.any())
    with pytest.raises(ValueError, match="out must be"):
        env.goal_paths(planes=False, out=(subgoal, subgoal, length))
    env.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("agents,batch", [(6, 3), (16, 4)])
def test_offset_views(fmt, agents, batch):
    """`planes`, `subgoal` and `length` as views one element past a 16-byte boundary (uint8 planes also four): the same
    result as fresh tensors, nothing written around them."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=16, num_agents=agents, obs_radius=3, density=0.3, seed=5), batch=batch)
    env.reset(seed=5)
    want = env.goal_paths(format=fmt)
    assert want[0].data_ptr() % 16 == 0 and bool(want[0].any())
    fill = 7
    for shift in ((1, 4) if fmt == "uint8" else (1,)):
        bufs, views = [], []
        for t in want:
            buf = torch.full((t.numel() + 8,), fill, dtype=t.dtype, device=env.device)
            assert buf.data_ptr() % 16 == 0
            bufs.append(buf)
            views.append(buf[shift:shift + t.numel()].view(t.shape))
        got = env.goal_paths(format=fmt, out=tuple(views))
        for g, v, t, buf in zip(got, views, want, bufs):
            assert g is v and torch.equal(v, t)
            assert bool((buf[:shift] == fill).all()) and bool((buf[shift + t.numel():] == fill).all())
    env.close()


def test_out_buffers_list_view_and_errors():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, pogema_v0
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21), batch=6)
    with pytest.raises(PgxError) as ei:
        env.goal_paths()
    assert ei.value.code == -4  # before a reset, like step()
    env.reset(seed=21)
    with pytest.raises(ValueError, match="format"):
        env.goal_paths(format="bits")
    for bad in (0, -1, 961, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"1\.\.960"):
            env.goal_paths(steps=bad)
    env.goal_paths(steps=960)
    subgoal = torch.empty((6, 5, 2), dtype=torch.int8, device=env.device)
    length = torch.empty((6, 5), dtype=torch.int32, device=env.device)
    for fmt, dtype, shape in (("float32", torch.float32, (6, 5, 7, 7)), ("uint8", torch.uint8, (6, 5, 7, 7)),
                              ("rows", torch.int32, (6, 5, 7))):
        want = env.goal_paths(format=fmt)
        o = torch.full(shape, 9, dtype=dtype, device=env.device)
        got = env.goal_paths(format=fmt, out=(o, subgoal, length))
        assert got[0] is o and got[1] is subgoal and got[2] is length
        assert all(torch.equal(g, t) for g, t in zip(got, want))
        wrong = torch.float32 if dtype != torch.float32 else torch.uint8
        for bad in (torch.empty(shape, dtype=wrong, device=env.device),
                    torch.empty(shape[:-1] + (6,), dtype=dtype, device=env.device),
                    torch.empty(shape[:-1] + (14,), dtype=dtype, device=env.device)[..., ::2],
                    torch.empty(shape, dtype=dtype)):
            with pytest.raises(ValueError, match=r"out\[planes\]"):
                env.goal_paths(format=fmt, out=(bad, subgoal, length))
        with pytest.raises(ValueError, match=r"out\[subgoal\]"):
            env.goal_paths(format=fmt, out=(o, subgoal.to(torch.int32), length))
        with pytest.raises(ValueError, match=r"out\[length\]"):
            env.goal_paths(format=fmt, out=(o, subgoal, length[:, :4]))
        with pytest.raises(ValueError, match="out must be"):
            env.goal_paths(format=fmt, out=(o, subgoal))
    env.close()

    one = pogema_v0(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21))
    one.reset(seed=21)
    views = one.goal_paths()
    assert isinstance(views, list) and len(views) == 5
    full = [t[0].cpu().numpy() for t in one._vec.goal_paths(format="uint8")]
    for i, (plane, xy, n) in enumerate(views):
        assert isinstance(plane, np.ndarray) and plane.shape == (7, 7) and plane.dtype == np.uint8
        assert np.array_equal(plane, full[0][i]) and xy == tuple(int(v) for v in full[1][i]) and n == int(full[2][i])
        assert type(n) is int and all(type(v) is int for v in xy)
    assert any(n for _, _, n in views)
    capped = one.goal_paths(steps=1)
    assert all(n <= 1 for _, _, n in capped)
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
        env.goal_paths(planes=False)
        assert env.cost_to_go_builds == B * A
        _check(env, what=f"size {size} second call")
        assert env.cost_to_go_builds == B * A
        env.close()
        # the cache is cost_to_go()'s: after it nothing is left to build; set_targets makes the moved agents' fields stale
        env = VecPogema(gc, batch=B)
        env.reset(seed=4)
        env.cost_to_go()
        assert env.cost_to_go_builds == B * A
        env.goal_paths()
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
        env.goal_paths(format="rows")
        assert env.cost_to_go_builds == B * A + len(moved)
        _check(env, what=f"size {size} after set_targets")
        env.cost_to_go()
        assert env.cost_to_go_builds == B * A + len(moved)
        env.close()


def test_first_call_inside_capture_is_refused():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=20, num_agents=4, obs_radius=2, density=0.3, seed=12), batch=4)
    env.reset(seed=12)
    out = (torch.zeros((4, 4, 5, 5), dtype=torch.float32, device="cuda"),
           torch.zeros((4, 4, 2), dtype=torch.int8, device="cuda"), torch.zeros((4, 4), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError, match="bytes") as ei:
        with torch.cuda.graph(g):
            env.goal_paths(out=out)
    assert ei.value.code == -4
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == 0
    _check(env, what="after the refused capture")
    env.close()


def test_identities_with_expert_and_cost_to_go():
    """For length > 0 the first marked cell is expert_actions()' destination; the marked cells are exactly those whose
    cost_to_go() is the centre's minus 1 .. minus length; length <= the centre's cost, equal iff the sub-goal is the
    target; uncapped, a sub-goal that is not the target has its successor outside the window."""
    from expert_reference import MOVES
    from pogema_amd import GridConfig, VecPogema
    moves = np.array(MOVES)
    for size, r in ((16, 3), (70, 2)):
        env = VecPogema(GridConfig(size=size, num_agents=13, obs_radius=r, density=0.3, seed=8, on_target="finish",
                                   max_episode_steps=64), batch=6)
        env.reset(seed=8)
        rng = np.random.default_rng(8)
        for _ in range(3):
            planes, subgoal, length = (t.cpu().numpy() for t in env.goal_paths(format="uint8"))
            one = env.goal_paths(steps=1, format="uint8")[0].cpu().numpy()
            actions, dist = (t.cpu().numpy() for t in env.expert_actions())
            ctg = env.cost_to_go().cpu().numpy()
            st = env.get_state()
            xy, tgt = st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy()
            on = length > 0
            assert on.any() and np.array_equal(on, dist > 0)
            first = np.zeros_like(one)
            bi, ai = np.nonzero(on)
            first[bi, ai, r + moves[actions[bi, ai], 0], r + moves[actions[bi, ai], 1]] = 1
            assert np.array_equal(one, first)
            centre = ctg[:, :, r, r]
            assert (length[on] <= centre[on]).all()
            hit = ((xy + subgoal) == tgt).all(-1) & on
            assert np.array_equal(hit, (length == centre) & on)
            bits = env.goal_directions(format="bits").cpu().numpy()
            for b, i in zip(bi, ai):
                marked = np.sort(ctg[b, i][planes[b, i] == 1])[::-1]
                assert np.array_equal(marked, centre[b, i] - np.arange(1, length[b, i] + 1)), (b, i)
                if not hit[b, i]:                # the descent from the sub-goal leaves the window
                    m = int(bits[b, i, r + subgoal[b, i, 0], r + subgoal[b, i, 1]])
                    nxt = subgoal[b, i] + moves[(m & -m).bit_length()]
                    assert m and np.abs(nxt).max() == r + 1
            env.step(mixed_actions(env, rng, p_expert=0.9))
        env.close()


def test_following_the_expert_reaches_the_subgoal():
    """One agent per env: stepping expert_actions() `length` times lands on p0 + subgoal."""
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=16, num_agents=1, obs_radius=3, density=0.3, seed=17, on_target="nothing",
                               max_episode_steps=10**6), batch=24)
    env.reset(seed=17)
    _, subgoal, length = (t.cpu().numpy() for t in env.goal_paths())
    p0 = env.get_state()["agents_xy"].cpu().numpy()
    assert length.max() >= 3
    seen = {0: p0}
    for t in range(1, int(length.max()) + 1):
        env.step(env.expert_actions()[0])
        seen[t] = env.get_state()["agents_xy"].cpu().numpy()
    for b in range(env.batch):
        assert np.array_equal(seen[int(length[b, 0])][b, 0], p0[b, 0] + subgoal[b, 0]), b
    env.close()


def test_state_untouched():
    """get_state() and the next step()'s outputs are identical with and without a preceding goal_paths()."""
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
            a.goal_paths(steps=(None, 2)[t % 2], format=FORMATS[t % 3], planes=t != 3)
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
    """goal_paths() captured once after an eager call, on one stream; replays after further steps (and after new targets,
    which make fields stale) equal the eager result on the same state."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A = 6, 6
    gc = GridConfig(size=size, num_agents=A, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                    on_target="nothing", max_episode_steps=10**6)
    env = VecPogema(gc, batch=B)
    env.reset(seed=4)
    outs = tuple(torch.zeros_like(t) for t in env.goal_paths(format="rows"))  # eager: allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.goal_paths(format="rows", out=outs)
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
        for o, e in zip(outs, env.goal_paths(format="rows")):
            assert torch.equal(o, e), f"step {t}"
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == built + B * A
    _check(env, what="after replays")
    env.close()
