"""GPU: neighbour lists (VecPogema.visible_agents / pgx_visible_agents, docs/SPEC.md S12) equal the CPU reference
(tests/visible_agents_reference.py) applied to get_state(), bit for bit on index, offset and count: every lane layout,
after resets and after steps of every collision system and on_target mode, truncated lists, and against plane 1 of the
engine's own observation.  The call leaves the engine state alone and can be captured in a HIP graph."""
import numpy as np
import pytest

from agent_counts import LAYOUT_ROWS, radii_accepted
from visible_agents_reference import visible_agents_reference
from util import lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu


def _reference(env, k):
    st = env.get_state()
    return visible_agents_reference(st["agents_xy"].cpu().numpy(), st["is_active"].cpu().numpy(), env.obs_radius, k)


def _check(env, k, what="", full=None):
    """visible_agents(k) == the reference on get_state(); returns the reference's (index, offset, count).  `full`: the
    reference for a k' >= k on the same state, whose first k entries are the reference for k (one sorted list, cut)."""
    got = [t.cpu().numpy() for t in env.visible_agents(k=k)]
    ref = _reference(env, k) if full is None else (full[0][:, :, :k], full[1][:, :, :k], full[2])
    assert got[0].dtype == np.int32 and got[1].dtype == np.int8 and got[2].dtype == np.int32
    for name, g, w in zip(("index", "offset", "count"), got, ref):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what} k={k}: {len(bad)} mismatches in {name}, first at {bad[0].tolist()}: "
                               f"{g[tuple(bad[0])]} vs {w[tuple(bad[0])]}")
    return ref


KS = (1, 5, 8, 13, 16, 17, 32)

# (agents, map side, batch): one row per lane layout -- several envs per wave, one wave, several waves, several workgroups
# per env -- with batches that leave the last workgroup partly filled.  Every row runs those of obs_radius 1, 5 and 15 the
# engine admits: it refuses 512 agents and more with a 31 x 31 window (README.md "Limits": the step kernel's LDS budget).
# The rows between 256 and 1024 agents are tests/agent_counts.py's: 3, 2 and 1 envs per 1024-lane workgroup of the planners
# and the outcomes, a last workgroup that is partly filled, ragged last chunks of the neighbour lists (1, 86 and 255 rows).
LAYOUTS = [(1, 6, 300), (2, 6, 131), (3, 7, 90), (8, 10, 70), (16, 12, 37), (33, 14, 9), (64, 16, 7), (65, 18, 5),
           (200, 28, 3), *LAYOUT_ROWS, (1024, 64, 2)]


@pytest.mark.parametrize("agents,size,batch", LAYOUTS)
def test_every_lane_layout_matches_reference(agents, size, batch):
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(agents)
    radii = radii_accepted(agents, size, batch)
    assert radii == (1, 5, 15) or (agents >= 512 and radii == (1, 5))
    for r in radii:
        gc = GridConfig(size=size, num_agents=agents, obs_radius=r, density=0.1, seed=agents + r,
                        collision_system="soft", on_target="finish", max_episode_steps=64)
        env = VecPogema(gc, batch=batch)
        env.reset(seed=agents + r)
        full = _reference(env, max(KS))
        for k in KS:
            _check(env, k, what=f"A={agents} r={r} reset", full=full)
        for _ in range(4):
            env.step(mixed_actions(env, rng, p_expert=0.8))
        full = _reference(env, max(KS))
        for k in KS:
            _check(env, k, what=f"A={agents} r={r} after 4 steps", full=full)
        env.close()


@pytest.mark.parametrize("name,rows,cols", [("wide", 5, 40), ("tall", 37, 6), ("odd", 13, 21)])
def test_non_square_maps(name, rows, cols):
    from pogema_amd import GridConfig, VecPogema
    grid = "\n".join("".join("#" if (x * 7 + y * 3) % 11 == 0 else "." for y in range(cols)) for x in range(rows))
    rng = np.random.default_rng(rows)
    for r in (1, 5, 15):
        env = VecPogema(GridConfig(map=grid, num_agents=12, obs_radius=r, seed=3, collision_system="priority",
                                   max_episode_steps=64), batch=11)
        env.reset(seed=3)
        for t in range(5):
            if t % 2 == 0:
                for k in KS:
                    _check(env, k, what=f"{name} r={r} step {t}")
            env.step(mixed_actions(env, rng, p_expert=0.8))
        env.close()


def test_1024_map():
    """The large-map layout of the step kernel underneath; agents are far apart, so a second env packs them close."""
    from pogema_amd import GridConfig, VecPogema
    rng = np.random.default_rng(1024)
    env = VecPogema(GridConfig(size=1024, num_agents=40, obs_radius=15, density=0.3, seed=5, max_episode_steps=64), batch=2)
    env.reset(seed=5)
    for k in (1, 13, 32):
        _check(env, k, what="1024 reset")
    for _ in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.8))
    for k in (1, 13, 32):
        _check(env, k, what="1024 after 3 steps")
    env.close()
    # the same map size with the agents placed next to each other at the far corner (coordinates above 1000)
    torch = lazy_torch()
    obst = np.zeros((1, 1024, 1024), dtype=np.uint8)
    cells = np.array([(1023 - i // 6, 1023 - i % 6) for i in range(30)], dtype=np.int32)[None]
    targets = np.array([(i // 6, i % 6) for i in range(30)], dtype=np.int32)[None]
    env = VecPogema(GridConfig(size=1024, num_agents=30, obs_radius=4, density=0.0, seed=5, max_episode_steps=64), batch=1)
    env.reset_from_state(obst, cells, targets)
    for k in (5, 32):
        ref = _check(env, k, what="1024 corner")
    assert ref[2].max() > 5
    env.step(torch.zeros((1, 30), dtype=torch.int64, device=env.device))
    _check(env, 32, what="1024 corner after a step")
    env.close()


@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
@pytest.mark.parametrize("collision", ["priority", "block_both", "soft"])
def test_modes_after_steps(collision, on_target):
    """Hidden (finished), restarted and auto-reset agents all occur."""
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=12, num_agents=10, obs_radius=3, density=0.25, seed=7, collision_system=collision,
                    on_target=on_target, max_episode_steps=40)
    env = VecPogema(gc, batch=24, auto_reset=True)
    env.reset(seed=7)
    rng = np.random.default_rng(11)
    inactive_seen = False
    seen = 0
    for t in range(45):
        if t % 3 == 0:
            for k in (1, 5, 13):
                ref = _check(env, k, what=f"{collision}/{on_target} step {t}")
            seen = max(seen, int(ref[2].max()))
            inactive_seen |= bool((~env.get_state()["is_active"]).any())
        env.step(mixed_actions(env, rng, p_expert=0.85))
    if on_target == "finish":
        assert inactive_seen, "no finished (hidden) agent was ever checked"
    assert seen > 0
    env.close()


def test_crowded_map_truncates_the_lists():
    from pogema_amd import GridConfig, VecPogema
    K = 8
    gc = GridConfig(size=12, num_agents=64, obs_radius=5, density=0.0, seed=2, collision_system="soft",
                    max_episode_steps=64)
    env = VecPogema(gc, batch=6)
    env.reset(seed=2)
    ref = _reference(env, K)
    assert ref[2].max() > K, "the case does not force truncation"
    _check(env, K, what="crowded")
    rng = np.random.default_rng(2)
    for _ in range(3):
        env.step(mixed_actions(env, rng, p_expert=0.8))
    ref = _check(env, K, what="crowded after 3 steps")
    assert ref[2].max() > K
    env.close()


@pytest.mark.parametrize("collision,soft_occupancy", [("priority", None), ("block_both", None), ("soft", "exact")])
@pytest.mark.parametrize("size,agents,r", [(16, 8, 5), (32, 16, 5), (64, 64, 5)])
def test_lists_rebuild_plane_one_of_the_observation(collision, soft_occupancy, size, agents, r):
    """Ones scattered at (r + dx, r + dy) for an active agent's list, plus its own centre, are plane 1 of observe()."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, Semantics, VecPogema
    K = 32
    gc = GridConfig(size=size, num_agents=agents, obs_radius=r, density=0.3, seed=13, collision_system=collision,
                    on_target="finish", max_episode_steps=128)
    kw = {} if soft_occupancy is None else {"semantics": Semantics(soft_occupancy=soft_occupancy)}
    env = VecPogema(gc, batch=16, **kw)
    env.reset(seed=13)
    rng = np.random.default_rng(13)
    W = 2 * r + 1
    for t in range(10):
        index, offset, count = env.visible_agents(k=K)
        assert int(count.max()) <= K
        plane = env.observe()[:, :, 1]
        active = env.get_state()["is_active"]
        built = torch.zeros((16, agents, W * W), dtype=torch.float32, device=env.device)
        cell = (offset[..., 0].long() + r) * W + offset[..., 1].long() + r
        built.scatter_(2, cell, (index >= 0).to(torch.float32))   # empty entries write 0 at the centre ...
        built[:, :, r * W + r] = 1.0                                # ... which is the agent itself
        built = built.view(16, agents, W, W)
        assert active.any()
        assert torch.equal(built[active], plane[active].to(torch.float32)), f"{collision} step {t}"
        env.step(mixed_actions(env, rng, p_expert=0.8))
    env.close()


def test_out_tensors_and_refused_arguments():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A, K = 6, 9, 5
    env = VecPogema(GridConfig(size=10, num_agents=A, obs_radius=3, density=0.1, seed=21), batch=B)
    env.reset(seed=21)
    index, offset, count = env.visible_agents(k=K)
    assert index.dtype == torch.int32 and tuple(index.shape) == (B, A, K)
    assert offset.dtype == torch.int8 and tuple(offset.shape) == (B, A, K, 2)
    assert count.dtype == torch.int32 and tuple(count.shape) == (B, A)
    d_index, _, _ = env.visible_agents()
    assert tuple(d_index.shape) == (B, A, 13)
    oi = torch.full((B, A, K), 99, dtype=torch.int32, device=env.device)
    oo = torch.full((B, A, K, 2), 99, dtype=torch.int8, device=env.device)
    oc = torch.full((B, A), 99, dtype=torch.int32, device=env.device)
    ri, ro, rc = env.visible_agents(k=K, out=(oi, oo, oc))
    assert ri is oi and ro is oo and rc is oc
    assert torch.equal(oi, index) and torch.equal(oo, offset) and torch.equal(oc, count)
    bad = [
        (torch.empty((B, A, K), dtype=torch.int64, device=env.device), oo, oc),           # dtype
        (oi, torch.empty((B, A, K, 2), dtype=torch.uint8, device=env.device), oc),
        (oi, oo, torch.empty((B, A), dtype=torch.int64, device=env.device)),
        (torch.empty((B, A, K + 1), dtype=torch.int32, device=env.device), oo, oc),       # shape
        (oi, torch.empty((B, A, K), dtype=torch.int8, device=env.device), oc),
        (oi, oo, torch.empty((B, A, 1), dtype=torch.int32, device=env.device)),
        (torch.empty((B, A, 2 * K), dtype=torch.int32, device=env.device)[:, :, ::2], oo, oc),  # contiguity
        (torch.empty((B, A, K), dtype=torch.int32), oo, oc),                              # device
        (oi, oo),
        (oi, None, oc),                                                                   # an entry left out
    ]
    for out in bad:
        with pytest.raises(ValueError):
            env.visible_agents(k=K, out=out)
    for k in (0, 33, -1, 2.0, None):
        with pytest.raises(ValueError):
            env.visible_agents(k=k)
    env.close()


def test_optional_outputs_through_the_c_abi():
    """offset = NULL / count = NULL: the other outputs are as usual and nothing else is written."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema, _lib
    B, A, K = 5, 20, 7
    env = VecPogema(GridConfig(size=9, num_agents=A, obs_radius=4, density=0.0, seed=8), batch=B)
    env.reset(seed=8)
    index, offset, count = env.visible_agents(k=K)
    n = B * A * K
    # guard words around every output: a write outside its range would show
    gi = torch.full((n + 64,), 77, dtype=torch.int32, device=env.device)
    go = torch.full((2 * n + 64,), 77, dtype=torch.int8, device=env.device)
    gc = torch.full((B * A + 64,), 77, dtype=torch.int32, device=env.device)
    call = env._lib.pgx_visible_agents
    for with_offset, with_count in ((False, False), (True, False), (False, True), (True, True)):
        gi.fill_(77), go.fill_(77), gc.fill_(77)
        _lib.check(call(env._handle, K, 0, gi[32:].data_ptr(), go[32:].data_ptr() if with_offset else None,
                        gc[32:].data_ptr() if with_count else None, env._stream()))
        assert torch.equal(gi[32:32 + n].view(B, A, K), index)
        assert bool((gi[:32] == 77).all()) and bool((gi[32 + n:] == 77).all())
        if with_offset:
            assert torch.equal(go[32:32 + 2 * n].view(B, A, K, 2), offset)
            assert bool((go[:32] == 77).all()) and bool((go[32 + 2 * n:] == 77).all())
        else:
            assert bool((go == 77).all())
        if with_count:
            assert torch.equal(gc[32:32 + B * A].view(B, A), count)
            assert bool((gc[:32] == 77).all()) and bool((gc[32 + B * A:] == 77).all())
        else:
            assert bool((gc == 77).all())
    # refused arguments: PGX_E_INVALID, and nothing is launched
    for k, flags, idx in ((0, 0, gi.data_ptr()), (33, 0, gi.data_ptr()), (K, 1, gi.data_ptr()), (K, 0, None)):
        assert call(env._handle, k, flags, idx, None, None, env._stream()) == -1
        assert b"pgx_visible_agents" in env._lib.pgx_last_error()
    env.close()


def test_before_reset_is_refused():
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=8, num_agents=2, obs_radius=2, seed=1), batch=2)
    with pytest.raises(PgxError) as ei:
        env.visible_agents()
    assert ei.value.code == -4  # PGX_E_STATE, as pgx_step before a reset
    env.close()


def test_state_untouched():
    """save_state() blobs before and after the call are equal, and the next step() equals that of a twin env that never
    called it."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=14, num_agents=12, obs_radius=3, density=0.2, seed=31, collision_system="soft",
                    on_target="restart", max_episode_steps=32)
    a = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
    b = VecPogema(gc, batch=8, auto_reset=True, reuse_buffers=False)
    a.reset(seed=31)
    b.reset(seed=31)
    rng = np.random.default_rng(31)
    for t in range(6):
        acts = torch.as_tensor(rng.integers(0, 5, size=(8, 12)), device=a.device)
        before = a.save_state()["engine"].clone()
        a.visible_agents(k=13)
        a.visible_agents(k=32)
        assert torch.equal(a.save_state()["engine"], before), f"step {t}"
        ra, rb = a.step(acts), b.step(acts)
        for x, y in zip(ra[:4], rb[:4]):
            assert torch.equal(x, y), f"step {t}"
        assert torch.equal(ra[4]["is_active"], rb[4]["is_active"])
    a.close()
    b.close()


def test_visible_agents_then_step_in_hip_graph():
    """visible_agents(out=...) -> step() captured once in a HIP graph; 30 replays equal the eager run of a twin and the
    reference.  No call outside the capture is needed beforehand (the warm-up is torch's recipe, not the engine's)."""
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    B, A, K = 32, 12, 13
    gc = GridConfig(size=12, num_agents=A, obs_radius=3, density=0.2, seed=4, collision_system="soft",
                    max_episode_steps=24)
    eager = VecPogema(gc, batch=B, auto_reset=True)
    graphed = VecPogema(gc, batch=B, auto_reset=True)
    eager.reset(seed=4)
    graphed.reset(seed=4)
    rng = np.random.default_rng(4)
    acts = torch.zeros((B, A), dtype=torch.int64, device="cuda")
    out_v = (torch.zeros((B, A, K), dtype=torch.int32, device="cuda"), torch.zeros((B, A, K, 2), dtype=torch.int8, device="cuda"),
             torch.zeros((B, A), dtype=torch.int32, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch's graph recipe asks
        graphed.visible_agents(k=K, out=out_v)
        graphed.step(acts)
    torch.cuda.current_stream().wait_stream(side)
    eager.step(acts)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.visible_agents(k=K, out=out_v)
        out = graphed.step(acts)
    for t in range(30):
        acts.copy_(mixed_actions(eager, rng, p_expert=0.8))
        want = _check(eager, K, what=f"eager step {t}")
        g.replay()
        ref = eager.step(acts)
        for name, x, w in zip(("index", "offset", "count"), out_v, want):
            assert np.array_equal(x.cpu().numpy(), w), f"step {t}: {name}"
        for x, y in zip(out[:4], ref[:4]):
            assert torch.equal(x, y), f"step {t}"
    se, sg = eager.get_state(), graphed.get_state()
    for k in se:
        assert torch.equal(se[k], sg[k])
    eager.close()
    graphed.close()


def test_list_view_of_the_single_env():
    from pogema_amd import GridConfig, pogema_v0
    one = pogema_v0(GridConfig(size=8, num_agents=10, obs_radius=3, density=0.0, seed=21))
    one.reset(seed=21)
    for k in (13, 2):
        lists = one.visible_agents(k=k) if k != 13 else one.visible_agents()
        index, offset, count = (t[0].cpu().numpy() for t in one._vec.visible_agents(k=k))
        assert isinstance(lists, list) and len(lists) == 10
        for i, row in enumerate(lists):
            n = min(int(count[i]), k)
            assert row == [(int(index[i, s]), int(offset[i, s, 0]), int(offset[i, s, 1])) for s in range(n)]
            assert all(isinstance(v, int) for e in row for v in e)
    assert any(len(row) == 2 for row in one.visible_agents(k=2))
    one.close()
