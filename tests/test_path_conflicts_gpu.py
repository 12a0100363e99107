"""GPU: path conflicts (VecPogema.path_conflicts / pgx_path_conflicts, docs/SPEC.md S26) equal the CPU reference
(tests/path_conflicts_reference.py, the all-pairs statement of the section) bit for bit on get_state() -- the hand-built
cases in both layouts with every subset of kinds and every `arrived`, forecasts and plans of random instances in every
on_target mode, every lane layout of the kernel with a partly filled last workgroup, K = 1 .. 256, keys that all fall
into one slot of the kernel's table, the widest keys -- and keep the contract of a query: `out=` buffers at odd addresses
with nothing written around them, NULL outputs, the engine state left alone, a first call inside a graph capture."""
import itertools

import numpy as np
import pytest

from agent_counts import LAYOUT_ROWS, pibt_geometry, radii_accepted
from path_conflicts_cases import ALL, CASES, FORECAST_INPUTS, PLAN_INPUT, expected, paths_of
from path_conflicts_reference import KINDS, path_conflicts_reference
from util import generate_instances, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu

NAMES = ("first_step", "partner", "kind", "count")
SUBSETS = tuple(s for n in (1, 2, 3) for s in itertools.combinations(ALL, n))
MODES = (("priority", "finish"), ("block_both", "restart"), ("soft", "nothing"))


def _vanish(env, arrived):
    return arrived == "vanish" if arrived is not None else env.grid_config.on_target == "finish"


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.dtype} {g.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what} {name}: {len(bad)} mismatches, first {bad[0].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"


def _check(env, paths, what="", kinds=(ALL,), arrived=("stay", "vanish", None)):
    """path_conflicts(paths) == the reference on get_state(), bit for bit, for every entry of `kinds` and `arrived`.
    Returns the reference's arrays of the last combination."""
    st = env.get_state()
    host = paths.cpu().numpy()
    state = [st[k].cpu().numpy() for k in ("agents_xy", "targets_xy", "is_active")]
    want = None
    for ks in kinds:
        for arr in arrived:
            want = path_conflicts_reference(host, *state, env.height, env.width, ks, _vanish(env, arr))
            _same(env.path_conflicts(paths, kinds=ks, arrived=arr), want, f"{what} [{'+'.join(ks)}, {arr}]")
    return want


def _env(gc_kw, batch, instance=None, **kw):
    """A VecPogema; `instance`: (obstacles, agents, targets) installed with reset_from_state, else reset(seed)."""
    from pogema_amd import GridConfig, VecPogema
    if instance is not None:
        gc = GridConfig(map=instance[0][0].tolist(), num_agents=instance[1].shape[1], **gc_kw)
        env = VecPogema(gc, batch=batch, **kw)
        env.reset_from_state(*instance)
    else:
        env = VecPogema(GridConfig(**gc_kw), batch=batch, **kw)
        env.reset(seed=gc_kw.get("seed", 0))
    return env


def _walks(rng, start, H, W, K, p_out=0.0):
    """Random walks from `start` int [B, A, 2] in the plan layout, int32 [K, B, A, 2]; `p_out`: cells set to (-1, -1)."""
    moves = np.array([(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)])
    pos, steps = np.asarray(start).astype(np.int64), []
    for _ in range(K):
        pos = np.clip(pos + moves[rng.integers(0, 5, pos.shape[:2])], 0, [H - 1, W - 1])
        steps.append(np.where(rng.random(pos.shape[:2] + (1,)) < p_out, -1, pos))
    return np.stack(steps).astype(np.int32)


def _to_cells(plan):
    return np.ascontiguousarray(plan.transpose(1, 2, 0, 3)).astype(np.int16)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_shared_cases(case):
    """The hand-built cases, installed through GridConfig(map, agents_xy, targets_xy) at batch 2: both layouts with every
    subset of kinds and every `arrived` against the reference, and the case's checks against the arrays it writes out."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(map="\n".join(case["map"]), agents_xy=case.get("start_xy", case["agents_xy"]),
                    targets_xy=case["targets_xy"], obs_radius=1,
                    on_target="finish" if "actions" in case else "nothing", max_episode_steps=64)
    env = VecPogema(gc, batch=2)
    env.reset(seed=0)
    if "actions" in case:
        env.step(torch.as_tensor([case["actions"]] * 2, device=env.device))
    st = env.get_state()
    assert st["is_active"][0].cpu().numpy().astype(bool).tolist() == case["is_active"]
    active = np.array(case["is_active"])
    assert st["agents_xy"][1].cpu().numpy()[active].tolist() == np.array(case["agents_xy"])[active].tolist()
    for layout in ("cells", "plan"):
        paths = torch.as_tensor(paths_of(case, layout, batch=2), device=env.device)
        _check(env, paths, what=f"{case['name']} {layout}", kinds=SUBSETS)
        for chk in case["checks"]:
            got = env.path_conflicts(paths, kinds=chk["kinds"], arrived=chk["arrived"])
            for b in range(2):
                _same([g[b] for g in got], expected(chk), f"{case['name']} {layout} {chk['kinds']} {chk['arrived']} env {b}")
    env.close()


@pytest.mark.parametrize("inp", FORECAST_INPUTS, ids=[f"{i['size']}x{i['size']}" for i in FORECAST_INPUTS])
@pytest.mark.parametrize("collision,on_target", MODES)
def test_forecast_form(inp, collision, on_target):
    """paths=None: the conflicts of agent_forecasts(steps)' cells, for steps 1, 2, 3 and 8, on the instances
    tests/test_path_conflicts.py proves non-vacuous and after four steps, when agents are hidden or have new targets."""
    torch = lazy_torch()
    instance = generate_instances(inp["batch"], inp["size"], inp["size"], inp["agents"], inp["density"], inp["seed"])
    env = _env(dict(obs_radius=2, collision_system=collision, on_target=on_target, max_episode_steps=64, seed=inp["seed"]),
               inp["batch"], instance)
    rng = np.random.default_rng(inp["seed"])
    for phase in ("reset", "stepped"):
        _, cells8 = env.agent_forecasts(8, planes=False)
        for steps in (1, 2, 3, 8):
            want = _check(env, cells8[:, :, :steps].contiguous(), what=f"{phase} steps {steps}")
            assert steps < 3 or (want[3] > 0).any()
            st = env.get_state()
            state = [st[k].cpu().numpy() for k in ("agents_xy", "targets_xy", "is_active")]
            for ks, arr in ((("vertex", "edge"), None), (ALL, "stay")):
                want = path_conflicts_reference(cells8[:, :, :steps].cpu().numpy(), *state, env.height, env.width, ks,
                                                _vanish(env, arr))
                _same(env.path_conflicts(steps=steps, kinds=ks, arrived=arr), want, f"{phase} paths=None steps {steps} {arr}")
        if phase == "reset":
            for _ in range(4):
                env.step(mixed_actions(env, rng, p_expert=0.8))
            if on_target == "finish":
                assert not bool(env.get_state()["is_active"].all()), "nobody is hidden: step longer"
    defaults = env.path_conflicts()
    _same(defaults, [t.cpu().numpy() for t in env.path_conflicts(steps=3, kinds=("vertex", "edge"), arrived=None)], "defaults")
    env.close()


SMALL_LAYOUTS = ((1, 8, 70), (2, 8, 70), (63, 24, 6), (64, 24, 6), (65, 24, 5), (256, 40, 2))


@pytest.mark.parametrize("agents,size,batch", SMALL_LAYOUTS + LAYOUT_ROWS + ((1024, 64, 2),),
                         ids=lambda v: str(v))
def test_lane_layouts(agents, size, batch):
    """Every shape of the kernel's workgroup: 64 envs of one or two agents, envs that straddle waves, one env per
    workgroup, 3 / 2 / 1 envs of 1024 lanes -- with a batch that leaves the last workgroup partly filled wherever a
    workgroup holds more than one env.  K = 3 from forecasts, all kinds."""
    T, epb, log2n, grid, last = pibt_geometry(agents, batch)
    assert T == (256 if agents <= 256 else 1024) and grid >= 2 and (epb == 1 or last < epb)
    r = radii_accepted(agents, size, batch)[0]
    env = _env(dict(size=size, num_agents=agents, obs_radius=r, density=0.1, seed=agents, on_target="nothing",
                    collision_system="soft", max_episode_steps=64), batch)
    env.step(mixed_actions(env, np.random.default_rng(agents), p_expert=0.8))
    _, cells = env.agent_forecasts(3, planes=False)
    want = _check(env, cells, what=f"A={agents}", arrived=("vanish", None))
    assert agents < 63 or (want[3] > 0).any()
    assert agents < 256 or ((want[3][0] > 0).any() and (want[3][-1] > 0).any()), "the first and the last env hold conflicts"
    env.close()


def test_many_workgroups():
    """200 envs of 13 agents: 11 workgroups of 19 envs, the last one holds 10."""
    assert pibt_geometry(13, 200)[1:] == (19, 5, 11, 10)
    env = _env(dict(size=8, num_agents=13, obs_radius=2, density=0.1, seed=2, max_episode_steps=64), 200)
    env.step(mixed_actions(env, np.random.default_rng(2), p_expert=0.7))
    _, cells = env.agent_forecasts(3, planes=False)
    want = _check(env, cells, what="200 x 13")
    assert (want[3][-1] > 0).any() or (want[3][-2] > 0).any()
    env.close()


@pytest.mark.parametrize("agents,K", [(64, 1), (64, 2), (64, 9), (5, 256)])
def test_steps_and_set_parity(agents, K):
    """Plan-layout random walks with a few cells outside the map.  64 agents fill an open 8 x 8 map, the smallest the
    engine accepts for them (it refuses more agents than cells): conflicts of every kind at every step, K odd and even;
    5 agents on an open 3 x 3 map walk the longest K."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    side = 8 if agents == 64 else 3
    rng = np.random.default_rng(K)
    B = 3
    cells = np.array([[n // side, n % side] for n in range(side * side)])
    agents_xy = np.stack([rng.permutation(cells)[:agents] for _ in range(B)])
    targets_xy = np.stack([rng.permutation(cells)[:agents] for _ in range(B)])
    gc = GridConfig(map="\n".join(["." * side] * side), num_agents=agents, obs_radius=1, on_target="nothing", max_episode_steps=64)
    env = VecPogema(gc, batch=B)
    env.reset_from_state(np.zeros((B, side, side), dtype=np.uint8), agents_xy, targets_xy)
    plan = _walks(rng, agents_xy, side, side, K, p_out=0.03)
    want = _check(env, torch.as_tensor(plan, device=env.device), what=f"plan K={K}", kinds=(ALL, ("edge",), ("vertex", "follow")))
    _check(env, torch.as_tensor(_to_cells(plan), device=env.device), what=f"cells K={K}")
    st = env.get_state()
    state = [st[k].cpu().numpy() for k in ("agents_xy", "targets_xy", "is_active")]
    for name in KINDS:
        per_kind = path_conflicts_reference(plan, *state, side, side, (name,), False)
        assert (per_kind[3] > 0).any(), name
    assert (want[3] > 0).any()
    env.close()


def kernel_slot(key, log2n):
    """The slot pgx_path_conflicts.hip's table probes first for a cell key: the kernel's hash, restated."""
    return ((key * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - log2n)


@pytest.mark.parametrize("conflict", [False, True])
def test_one_bucket(conflict):
    """20 agents whose current cells and whose cells of both steps are 60 distinct cells of a 64 x 64 map that all start
    probing at one slot of the 64-slot table: the probe runs past 19 foreign keys.  Without a conflict nothing is
    reported; with one (a shared cell at step 1, a swap at step 2, a follow at step 2) exactly that."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    A, side = 20, 64
    log2n = pibt_geometry(A, 2)[2]
    assert log2n == 6
    keys = [k for k in range(side * side) if kernel_slot(k, log2n) == 5]
    assert len(keys) >= 3 * A
    cell = lambda k: [k // side, k % side]
    now, one, two = ([cell(k) for k in keys[s * A:(s + 1) * A]] for s in range(3))
    if conflict:
        one[1] = one[0]                          # agents 0 and 1 share a cell at step 1
        two[2], two[3] = one[3], one[2]          # agents 2 and 3 change places
        two[4] = one[5]                          # agent 4 follows agent 5
    gc = GridConfig(map="\n".join(["." * side] * side), agents_xy=now, targets_xy=now[1:] + now[:1], obs_radius=1,
                    on_target="nothing", max_episode_steps=64)
    env = VecPogema(gc, batch=2)
    env.reset(seed=0)
    plan = np.repeat(np.array([one, two], dtype=np.int32)[:, None], 2, 1)
    want = _check(env, torch.as_tensor(plan, device=env.device), what="one bucket plan", kinds=SUBSETS)
    _check(env, torch.as_tensor(_to_cells(plan), device=env.device), what="one bucket cells")
    if conflict:
        assert want[0][0, :6].tolist() == [1, 1, 2, 2, 2, -1] and want[2][0, :6].tolist() == [1, 1, 2, 2, 4, 0]
        assert want[3].sum() == 2 * 5
    else:
        assert not want[3].any()
    env.close()


def test_widest_keys():
    """One env of 1024 x 1024: the corner cells' keys use all 20 bits.  No distance field is built."""
    torch = lazy_torch()
    env = _env(dict(size=1024, num_agents=3, obs_radius=1, density=0.0, seed=3, on_target="nothing", max_episode_steps=64), 1)
    corners = np.array([(1023, 1023), (1023, 0), (0, 1023)])
    rng = np.random.default_rng(3)
    plan = corners[rng.integers(0, 3, (12, 1, 3))].astype(np.int32)
    plan[0, 0] = corners[[0, 0, 1]]              # a vertex at (1023, 1023)
    plan[1, 0] = corners[[1, 2, 0]]
    plan[2, 0] = corners[[2, 1, 0]]              # (1023, 0) <-> (0, 1023): an edge
    want = _check(env, torch.as_tensor(plan, device=env.device), what="1024 x 1024 plan", kinds=SUBSETS)
    _check(env, torch.as_tensor(_to_cells(plan), device=env.device), what="1024 x 1024 cells")
    assert want[0][0].tolist() == [1, 1, 2] and want[3][0].min() >= 2
    assert env.cost_to_go_builds == 0
    env.close()


@pytest.mark.parametrize("on_target", ["finish", "nothing"])
def test_a_plan_has_no_vertex_and_no_edge_conflict(on_target):
    """pibt_plan()'s promise, checked on the device: distinct cells and no swaps over 32 steps, judged the way the plan
    was made (arrived=None); its follow moves are found."""
    inp = PLAN_INPUT
    instance = generate_instances(inp["batch"], inp["size"], inp["size"], inp["agents"], inp["density"], inp["seed"])
    env = _env(dict(obs_radius=3, collision_system="soft", on_target=on_target, max_episode_steps=64, seed=inp["seed"]),
               inp["batch"], instance, auto_reset=False)
    path_xy = env.pibt_plan(inp["steps"])[1]
    _check(env, path_xy, what=f"plan {on_target}", kinds=(ALL, ("vertex", "edge")))
    first, partner, kind, count = env.path_conflicts(path_xy)
    assert int(count.sum()) == 0 and bool((first == -1).all()) and bool((partner == -1).all()) and not bool(kind.any())
    assert int(env.path_conflicts(path_xy, kinds=("follow",))[3].sum()) >= 1
    env.close()


def test_block_both_leaves_the_plan_no_earlier_than_its_first_follow():
    """Under block_both the engine reverts follow moves: the first step at which stepping the plan's actions leaves
    path_xy in an env is never before the env's smallest first_step of kind follow."""
    torch = lazy_torch()
    inp = PLAN_INPUT
    K = inp["steps"]
    instance = generate_instances(inp["batch"], inp["size"], inp["size"], inp["agents"], inp["density"], inp["seed"])
    env = _env(dict(obs_radius=3, collision_system="block_both", on_target="finish", max_episode_steps=64, seed=inp["seed"]),
               inp["batch"], instance, auto_reset=False)
    actions, path_xy = env.pibt_plan(K)[:2]
    first = env.path_conflicts(path_xy, kinds=("follow",))[0]
    big = K + 1
    first_follow = torch.where(first > 0, first, torch.full_like(first, big)).min(1).values.cpu().numpy()
    left = np.full(inp["batch"], big)
    alive = np.ones(inp["batch"], dtype=bool)
    for h in range(K):
        out = env.step(actions[h])
        off = (env.get_state()["agents_xy"] != path_xy[h]).any(-1).any(-1).cpu().numpy()
        left = np.where(alive & off & (left == big), h + 1, left)
        alive &= ~out[4]["episode_done"].cpu().numpy().astype(bool)
    print("first follow per env", first_follow.tolist(), "left the plan at", left.tolist())
    assert (left < big).any(), "no env left its plan: the check is vacuous"
    assert (first_follow <= left).all()
    env.close()


def test_out_buffers_and_offset_views():
    """`out=` buffers, `kind` at an odd address, cells-layout `paths` as a view 2 bytes past a 16-byte boundary: the same
    result, nothing written around them."""
    torch = lazy_torch()
    env = _env(dict(size=12, num_agents=16, obs_radius=2, density=0.3, seed=26, on_target="nothing", max_episode_steps=64), 5)
    _, cells = env.agent_forecasts(8, planes=False)
    want = env.path_conflicts(cells, kinds=ALL)
    assert int(want[3].sum()) > 0
    fill = 77
    bufs = [torch.full((t.numel() + 8,), fill, dtype=t.dtype, device=env.device) for t in want]
    views = [b[1:1 + t.numel()].view(t.shape) for b, t in zip(bufs, want)]
    assert views[2].data_ptr() % 2 == 1
    pbuf = torch.full((cells.numel() + 8,), fill, dtype=torch.int16, device=env.device)
    pview = pbuf[1:1 + cells.numel()].view(cells.shape)
    pview.copy_(cells)
    assert pview.data_ptr() % 16 == 2
    got = env.path_conflicts(pview, kinds=ALL, out=tuple(views))
    for g, v, t, b in zip(got, views, want, bufs):
        assert g is v and torch.equal(v, t)
        assert bool((b[:1] == fill).all()) and bool((b[1 + t.numel():] == fill).all())
    assert torch.equal(pview, cells) and bool((pbuf[:1] == fill).all()) and bool((pbuf[1 + cells.numel():] == fill).all())
    env.close()


def test_null_outputs_list_view_and_refusals():
    torch = lazy_torch()
    from pogema_amd import CONFLICT_KINDS, GridConfig, VecPogema, _lib, pogema_v0
    from pogema_amd._lib import PgxError
    B, A, K = 4, 16, 4
    env = VecPogema(GridConfig(size=12, num_agents=A, obs_radius=2, density=0.3, seed=26, max_episode_steps=64), batch=B)
    paths = torch.zeros((B, A, K, 2), dtype=torch.int16, device=env.device)
    with pytest.raises(PgxError) as ei:
        env.path_conflicts(paths)
    assert ei.value.code == -4  # before a reset, like step()
    env.reset(seed=26)
    _, paths = env.agent_forecasts(K, planes=False)
    want = env.path_conflicts(paths, kinds=ALL, arrived="stay")
    assert int(want[3].sum()) > 0
    # every combination of NULL outputs through the C entry
    for mask in range(1, 16):
        outs = [torch.full_like(t, 99) for t in want]
        ptrs = [o.data_ptr() if mask >> n & 1 else None for n, o in enumerate(outs)]
        _lib.check(env._lib.pgx_path_conflicts(env._handle, paths.data_ptr(), _lib.CONFLICT_PATHS_CELLS, K, 7 | 8, *ptrs,
                                               env._stream()))
        for n, (o, t) in enumerate(zip(outs, want)):
            assert torch.equal(o, t) if mask >> n & 1 else bool((o == 99).all()), (mask, n)
    # the Python refusals
    plan = paths.permute(2, 0, 1, 3).contiguous().to(torch.int32)
    assert all(torch.equal(a, b) for a, b in zip(env.path_conflicts(plan, kinds=ALL, arrived="stay"), want))
    for bad in (paths.cpu().numpy(), paths.tolist(), paths.to(torch.int64), paths.float(), plan.to(torch.uint8)):
        with pytest.raises(TypeError, match="paths must be"):
            env.path_conflicts(bad)
    for bad in (paths[:, :, :, :1], paths[:, :15], paths[:3], paths.permute(2, 0, 1, 3), plan.permute(1, 2, 0, 3),
                plan[:, :, :, :1], paths.cpu(), plan.cpu(), paths[:, :, :0],
                torch.zeros((B, A, 257, 2), dtype=torch.int16, device=env.device),
                torch.zeros((B, 2 * A, K, 2), dtype=torch.int16, device=env.device)[:, ::2]):
        with pytest.raises(ValueError, match=r"paths must be a contiguous int(16|32) tensor of shape"):
            env.path_conflicts(bad)
    for bad in ((), "vertex", ("vertex", "vertex"), ("swap",)):
        with pytest.raises(ValueError, match="'vertex', 'edge', 'follow'"):
            env.path_conflicts(paths, kinds=bad)
    with pytest.raises(ValueError, match="'stay' or 'vanish'"):
        env.path_conflicts(paths, arrived="finish")
    for bad in (0, 9, True, 2.0):
        with pytest.raises(ValueError, match=r"1\.\.8"):
            env.path_conflicts(steps=bad)
    env.path_conflicts(paths, steps=99)        # ignored when paths is given
    with pytest.raises(ValueError, match="out must be"):
        env.path_conflicts(paths, out=want[:3])
    with pytest.raises(ValueError, match=r"out\[kind\] is None"):
        env.path_conflicts(paths, out=(want[0], want[1], None, want[3]))
    for n, name in enumerate(NAMES):
        for bad in (want[n].to(torch.int16), want[n][:, :8], want[n].cpu()):
            outs = list(want)
            outs[n] = bad
            with pytest.raises(ValueError, match=rf"out\[{name}\]"):
                env.path_conflicts(paths, out=tuple(outs))
    env.close()

    one = pogema_v0(GridConfig(size=12, num_agents=A, obs_radius=2, density=0.3, seed=26))
    one.reset(seed=26)
    views = one.path_conflicts(steps=8, kinds=ALL, arrived="stay")
    full = [t[0].cpu().numpy() for t in one._vec.path_conflicts(steps=8, kinds=ALL, arrived="stay")]
    assert isinstance(views, list) and len(views) == A and any(v[3] for v in views)
    for i, (first, partner, kinds, count) in enumerate(views):
        assert all(type(v) is int for v in (first, partner, count)) and type(kinds) is tuple
        assert (first, partner, count) == (int(full[0][i]), int(full[1][i]), int(full[3][i]))
        assert sum(CONFLICT_KINDS[k] for k in kinds) == int(full[2][i]) and (kinds == ()) == (first == -1)
    one.close()


def test_state_and_next_step_are_untouched():
    torch = lazy_torch()
    kw = dict(size=12, num_agents=16, obs_radius=2, density=0.3, seed=26, collision_system="priority", max_episode_steps=64)
    asked, plain = _env(kw, 6), _env(kw, 6)
    rng = np.random.default_rng(1)
    for t in range(3):
        _, cells = asked.agent_forecasts(8, planes=False)
        plain.agent_forecasts(8, planes=False)
        asked.path_conflicts(cells, kinds=ALL)
        asked.path_conflicts(cells.permute(2, 0, 1, 3).contiguous().to(torch.int32), arrived="stay")
        sa, sp = asked.get_state(occupancy=True), plain.get_state(occupancy=True)
        assert all(torch.equal(sa[k], sp[k]) for k in sa), t
        actions = torch.as_tensor(rng.integers(0, 5, size=(6, 16)), device=asked.device)
        oa, op = asked.step(actions), plain.step(actions)
        assert all(torch.equal(a, p) for a, p in zip(oa[:4], op[:4])), t
    asked.close()
    plain.close()


def test_first_call_inside_a_capture():
    """With caller paths the very first call of an engine may be captured: its replays after further steps equal the
    eager call.  With paths=None the first call inside a capture is agent_forecasts()', which is refused."""
    torch = lazy_torch()
    from pogema_amd._lib import PgxError
    kw = dict(size=12, num_agents=16, obs_radius=2, density=0.3, seed=26, max_episode_steps=64)
    env = _env(kw, 5)
    st = env.get_state()
    plan = torch.as_tensor(_walks(np.random.default_rng(5), st["agents_xy"].cpu().numpy(), 12, 12, 6), device=env.device)
    outs = tuple(torch.zeros((5, 16), dtype=d, device=env.device) for d in (torch.int32, torch.int32, torch.uint8, torch.int32))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.path_conflicts(plan, kinds=ALL, out=outs)
    assert env.cost_to_go_builds == 0
    rng = np.random.default_rng(6)
    for t in range(3):
        g.replay()
        want = _check(env, plan, what=f"eager after {t} steps", arrived=(None,))
        _same(outs, want, f"replay after {t} steps")
        assert (want[3] > 0).any()
        env.step(torch.as_tensor(rng.integers(0, 5, size=(5, 16)), device=env.device))
    env.close()

    env = _env(kw, 5)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError, match="bytes") as ei:
        with torch.cuda.graph(g):
            env.path_conflicts(out=outs)
    assert ei.value.code == -4
    torch.cuda.synchronize()
    _, cells = env.agent_forecasts(3, planes=False)
    _same(env.path_conflicts(), _check(env, cells, kinds=(("vertex", "edge"),), arrived=(None,)), "after the refused capture")
    env.close()
