"""GPU: map pools (docs/SPEC.md S10) -- pgx_set_map_pool / pgx_reset_pool / pgx_regenerate_pool / pgx_get_map_index through
VecPogema -- against the generator oracles (oracle/generator_oracle.py with `given_map`, po_generate of the C oracle)
and the step oracle (oracle/pogema_oracle.py), and against the shared-map path a one-map pool must reproduce."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import generator_oracle as G
from oracle.c_oracle import load as load_c_oracle
from oracle.pogema_oracle import PogemaOracle, splitmix64
from util import random_actions

pytestmark = pytest.mark.gpu

TAG_POOL = 0x504F4F4C00000000


def pick(seed, env, epoch, M):
    return ((splitmix64(G.instance_hash(seed, env, epoch, 0) ^ TAG_POOL) >> 32) * M) >> 32


def oracle_instance(pool, seed, env, epoch, A):
    """(k, obstacles, agents_xy, targets_xy) of global env `env` in generation `epoch` (Python generator oracle)."""
    k = pick(seed, env, epoch, len(pool))
    H, W = pool.shape[1:]
    o, a, t = G.generate_instance(seed, env, H, W, A, 0.0, epoch=epoch, given_map=pool[k])
    return k, o, a, t


def c_instance(pool, seed, env, epoch, A):
    """The same through the C oracle's po_generate, one env per call (fast enough for full-size batches)."""
    lib = load_c_oracle()
    lib.po_generate.argtypes = [C.c_int32] * 4 + [C.c_float, C.c_uint64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
    lib.po_generate.restype = C.c_int
    k = pick(seed, env, epoch, len(pool))
    H, W = pool.shape[1:]
    m = np.ascontiguousarray(pool[k], np.uint8)
    a = np.empty((1, A, 2), np.int32)
    t = np.empty((1, A, 2), np.int32)
    ep = np.array([epoch], np.uint32)
    assert lib.po_generate(1, H, W, A, 0.0, seed, env, ep.ctypes.data, 10, 1, m.ctypes.data, a.ctypes.data,
                           t.ctypes.data) == 0
    return k, m, a[0], t[0]


def make_pool(M, H, W, seed):
    """Hand-built maps: Bernoulli maps of mixed densities, horizontal walls with doors, vertical corridors, rooms."""
    rng = np.random.default_rng(seed)
    maps = np.zeros((M, H, W), np.uint8)
    for m in range(M):
        kind = m % 4
        if kind == 0:
            maps[m] = rng.random((H, W)) < rng.choice([0.0, 0.1, 0.2, 0.3])
        elif kind == 1:
            for x in range(2, H, 4):
                maps[m, x, :] = 1
                maps[m, x, rng.integers(0, W, size=max(1, W // 8))] = 0
        elif kind == 2:
            for y in range(1, W, 3):
                maps[m, :, y] = 1
                maps[m, rng.integers(0, H), y] = 0
            maps[m] &= (rng.random((H, W)) > 0.05).astype(np.uint8)
        else:
            maps[m, ::max(2, H // 3), :] = 1
            maps[m, :, ::max(2, W // 3)] = 1
            maps[m] &= (rng.random((H, W)) > 0.3).astype(np.uint8)
    return maps


def device_state(env):
    maps = torch.empty((env.batch, env.height, env.width), dtype=torch.uint8, device=env.device)
    from pogema_amd import _lib
    _lib.check(env._lib.pgx_get_map(env._handle, maps.data_ptr(), env._stream()))
    st = env.get_state()
    return (maps.cpu().numpy(), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
            env.map_index.cpu().numpy())


RESET_CASES = [
    # name, H, W, A, r, on_target, empty_outside, env_index_base
    ("finish", 12, 12, 6, 3, "finish", True, 0),
    ("restart", 12, 12, 6, 3, "restart", True, 13),
    ("nothing_nonsquare", 9, 14, 5, 2, "nothing", True, 5),
    ("outside_random", 10, 16, 4, 4, "finish", False, 3),
]


@pytest.mark.parametrize("case", RESET_CASES, ids=[c[0] for c in RESET_CASES])
def test_reset_matches_oracle_and_rollout(case):
    from pogema_amd import GridConfig, VecPogema
    _, H, W, A, r, on_target, empty_outside, base = case
    B, seed, T = 10, 31, 10
    pool = make_pool(5, H, W, seed=len(case[0]))
    gc = GridConfig(num_agents=A, obs_radius=r, seed=seed, on_target=on_target, empty_outside=empty_outside,
                    density=0.25, max_episode_steps=64, collision_system="soft")
    env = VecPogema(gc, batch=B, env_index_base=base, map_pool=pool)
    assert np.array_equal(env.map_pool.cpu().numpy(), pool) and (env.map_index.cpu().numpy() == -1).all()
    obs, _ = env.reset(seed=seed)
    maps, agents, targets, index = device_state(env)
    refs = []
    for b in range(B):
        k, o, a, t = oracle_instance(pool, seed, base + b, 0, A)
        assert index[b] == k and np.array_equal(maps[b], o), f"env {b}: map"
        assert np.array_equal(agents[b], a) and np.array_equal(targets[b], t), f"env {b}: placement"
        refs.append(PogemaOracle(o, a, t, obs_radius=r, collision_system="soft", on_target=on_target, max_episode_steps=64,
                                 auto_reset=False, seed=seed, env_index=base + b, empty_outside=empty_outside,
                                 outside_density=0.25))
    assert len(set(index.tolist())) > 1, "the pool should spread over several maps"
    assert np.array_equal(obs.cpu().numpy(), np.stack([np.stack(e._obs()) for e in refs]))
    go, ga, gt = env.generate(seed)  # the host generator draws the same instances
    assert np.array_equal(go, maps) and np.array_equal(ga, agents) and np.array_equal(gt, targets)
    actions = random_actions(T, B, A, 3)
    for t in range(T):
        obs, rew, term, trunc, _ = env.step(torch.from_numpy(actions[t]).cuda())
        st = env.get_state()
        for b in range(B):
            robs, rrew, rterm, rtrunc, _ = refs[b].step(actions[t, b])
            rs = refs[b].get_state()
            assert np.array_equal(obs[b].cpu().numpy(), np.stack(robs)), (t, b)
            assert rew[b].tolist() == rrew and term[b].tolist() == rterm and trunc[b].tolist() == rtrunc, (t, b)
            assert np.array_equal(st["agents_xy"][b].cpu().numpy(), rs["agents_xy"])
            assert np.array_equal(st["targets_xy"][b].cpu().numpy(), rs["targets_xy"]), (t, b)
    env.close()


@pytest.mark.parametrize("observation_type", ["POMAPF", "MAPF"])
def test_reset_with_dict_observations(observation_type):
    from pogema_amd import GridConfig, VecPogema
    pool = make_pool(3, 8, 11, seed=2)
    env = VecPogema(GridConfig(num_agents=3, obs_radius=2, seed=4, observation_type=observation_type), batch=6,
                    map_pool=pool)
    obs, _ = env.reset(seed=4)
    index = env.map_index.cpu().numpy()
    assert (obs["xy"] == 0).all()
    if observation_type == "MAPF":
        assert np.array_equal(obs["global_obstacles"].cpu().numpy(), pool[index].astype(np.float32))
    env.close()


def test_one_map_pool_equals_shared_map():
    """A pool of one map draws, bit for bit, the instances of GridConfig(map=pool[0]): after reset, after reset_where and
    over regenerate steps."""
    from pogema_amd import GridConfig, VecPogema
    B, A, seed, T = 9, 5, 8, 4
    one = make_pool(1, 11, 11, seed=9)
    common = dict(num_agents=A, obs_radius=3, seed=seed, max_episode_steps=T, on_target="restart")
    pooled = VecPogema(GridConfig(**common), batch=B, env_index_base=2, map_pool=one, auto_reset="regenerate")
    shared = VecPogema(GridConfig(map=one[0].tolist(), **common), batch=B, env_index_base=2, auto_reset="regenerate")

    def same(what, o1, o2):
        assert torch.equal(o1, o2), what
        s1, s2 = device_state(pooled), device_state(shared)
        for x, y in zip(s1[:3], s2[:3]):
            assert np.array_equal(x, y), what
        assert (s1[3] == 0).all() and (s2[3] == -1).all(), what
        for k, v in pooled.get_state().items():
            assert torch.equal(v, shared.get_state()[k]), (what, k)

    same("reset", pooled.reset(seed=seed)[0], shared.reset(seed=seed)[0])
    mask = torch.zeros(B, dtype=torch.bool, device="cuda")
    mask[::3] = True
    same("reset_where", pooled.reset_where(mask, seed=seed + 1), shared.reset_where(mask, seed=seed + 1))
    actions = random_actions(3 * T + 1, B, A, 6)
    for t in range(actions.shape[0]):
        a = torch.from_numpy(actions[t]).cuda()
        o1, r1, *_ = pooled.step(a)
        o2, r2, *_ = shared.step(a)
        assert torch.equal(r1, r2)
        same(f"step {t}", o1, o2)
    assert pooled.regenerate_failures() == 0 == shared.regenerate_failures()
    pooled.close()
    shared.close()


def test_reset_where_follows_oracle():
    from pogema_amd import GridConfig, VecPogema
    B, A, seed, base = 12, 4, 17, 40
    pool = make_pool(6, 10, 13, seed=5)
    env = VecPogema(GridConfig(num_agents=A, obs_radius=2, seed=seed), batch=B, env_index_base=base, map_pool=pool)
    env.reset(seed=seed)
    before = device_state(env)
    epochs = np.zeros(B, np.int64)
    rng = np.random.default_rng(1)
    for rnd in range(3):
        mask = rng.random(B) < 0.5
        env.reset_where(torch.from_numpy(mask), seed=seed)
        epochs += mask
        maps, agents, targets, index = device_state(env)
        for b in range(B):
            if not mask[b]:
                assert all(np.array_equal(x[b], y[b]) for x, y in zip((maps, agents, targets, index), before)), (rnd, b)
                continue
            k, o, a, t = oracle_instance(pool, seed, base + b, int(epochs[b]), A)
            assert index[b] == k and np.array_equal(maps[b], o), (rnd, b)
            assert np.array_equal(agents[b], a) and np.array_equal(targets[b], t), (rnd, b)
        assert np.array_equal(env._initial[0].cpu().numpy(), maps)
        before = (maps, agents, targets, index)
    env.close()


@pytest.mark.parametrize("on_target,empty_outside", [("finish", True), ("restart", True), ("finish", False)])
def test_regenerate_follows_oracle(on_target, empty_outside):
    """auto_reset='regenerate' with a pool: a finished env continues on pool map pick(seed, env, epoch) with the oracle's
    placement, checked step by step against per-env oracles rebuilt at every episode end (no host sync in step())."""
    from pogema_amd import GridConfig, VecPogema
    B, A, r, seed, base, T = 12, 4, 2, 21, 7, 5
    pool = make_pool(6, 10, 10, seed=3)
    gc = GridConfig(num_agents=A, obs_radius=r, density=0.25, seed=seed, on_target=on_target, max_episode_steps=T,
                    collision_system="priority", empty_outside=empty_outside)
    env = VecPogema(gc, batch=B, env_index_base=base, auto_reset="regenerate", map_pool=pool)
    obs, _ = env.reset(seed=seed)

    def fresh(b, epoch):
        k, o, a, t = oracle_instance(pool, seed, base + b, epoch, A)
        return k, PogemaOracle(o, a, t, obs_radius=r, collision_system="priority", on_target=on_target,
                               max_episode_steps=T, auto_reset=False, seed=seed, env_index=base + b,
                               empty_outside=empty_outside, outside_density=0.25, epoch=epoch)

    epochs = [0] * B
    refs = [fresh(b, 0) for b in range(B)]
    assert np.array_equal(obs.cpu().numpy(), np.stack([np.stack(e._obs()) for _, e in refs]))
    rng = np.random.default_rng(5)
    for t in range(3 * T + 2):
        acts = rng.integers(0, 5, size=(B, A))
        obs, rew, term, trunc, info = env.step(torch.from_numpy(acts).cuda())
        st = env.get_state()
        index = env.map_index.cpu().numpy()
        for b in range(B):
            robs, rrew, rterm, rtrunc, _ = refs[b][1].step(acts[b])
            assert rew[b].tolist() == rrew and term[b].tolist() == rterm and trunc[b].tolist() == rtrunc, (t, b)
            done = all(rterm) or all(rtrunc)
            assert bool(info["episode_done"][b]) == done
            if done:
                epochs[b] += 1
                refs[b] = fresh(b, epochs[b])
                robs = refs[b][1]._obs()
            rs = refs[b][1].get_state()
            assert index[b] == refs[b][0], (t, b)
            assert np.array_equal(obs[b].cpu().numpy(), np.stack(robs)), (t, b)
            assert np.array_equal(st["agents_xy"][b].cpu().numpy(), rs["agents_xy"])
            assert np.array_equal(st["targets_xy"][b].cpu().numpy(), rs["targets_xy"])
            assert int(st["elapsed"][b]) == rs["elapsed"]
    assert max(epochs) >= 3 and env.regenerate_failures() == 0
    env.close()


def test_full_size_pool_matches_c_oracle():
    """configs[2] (8192 envs x 64x64, 64 agents) on a pool of 64 hand-built maps: every env equals po_generate."""
    from pogema_amd import GridConfig, VecPogema
    B, S, A, seed = 8192, 64, 64, 123
    pool = make_pool(64, S, S, seed=11)
    env = VecPogema(GridConfig(num_agents=A, obs_radius=5, seed=seed), batch=B, map_pool=pool)
    env.reset(seed=seed)
    maps, agents, targets, index = device_state(env)
    assert len(set(index.tolist())) == 64
    for b in range(B):
        k, o, a, t = c_instance(pool, seed, b, 0, A)
        assert index[b] == k and np.array_equal(maps[b], o), b
        assert np.array_equal(agents[b], a) and np.array_equal(targets[b], t), b
    env.close()


@pytest.mark.parametrize("H,W,on_target", [(256, 256, "restart"), (600, 20, "finish")])
def test_large_map_pool_matches_c_oracle(H, W, on_target):
    """Maps beyond the LDS forest: the pool's components are labelled with the L2-resident union-find."""
    from pogema_amd import GridConfig, VecPogema
    B, A, seed, base = 12, 64, 5, 1000
    pool = make_pool(4, H, W, seed=H)
    env = VecPogema(GridConfig(num_agents=A, obs_radius=3, seed=seed, on_target=on_target), batch=B,
                    env_index_base=base, map_pool=pool)
    env.reset(seed=seed)
    maps, agents, targets, index = device_state(env)
    for b in range(B):
        k, o, a, t = c_instance(pool, seed, base + b, 0, A)
        assert index[b] == k and np.array_equal(maps[b], o), b
        assert np.array_equal(agents[b], a) and np.array_equal(targets[b], t), b
    env.step(torch.zeros((B, A), dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    env.close()


def test_install_refuses_maps_below_capacity():
    from pogema_amd import GridConfig, VecPogema
    pool = np.zeros((3, 6, 6), np.uint8)
    pool[1] = 1
    pool[1, 0, :3] = 0   # one component of 3 cells: 1 pair
    pool[1, 5, 5] = 0    # and a single cell: 0 pairs
    with pytest.raises(ValueError, match=r"map 1 of the pool holds 1 start/target pairs"):
        VecPogema(GridConfig(num_agents=2, obs_radius=2), batch=4, map_pool=pool)
    env = VecPogema(GridConfig(num_agents=2, obs_radius=2, seed=1), batch=4, map_pool=pool[[0, 2]])
    assert env.pool_capacity.tolist() == [18, 18]
    env.reset(seed=1)
    with pytest.raises(ValueError, match=r"map 0 of the pool holds 1"):
        env.set_map_pool(pool[[1, 0]])
    assert env.map_pool is None  # a refused pool is not installed; the current instances stay
    with pytest.raises(ValueError, match="this engine's are 6x6"):
        env.set_map_pool(np.zeros((2, 6, 7), np.uint8))
    env.set_map_pool(pool[[2]])
    env.reset(seed=1)
    assert (env.map_index.cpu().numpy() == 0).all()
    env.close()


def test_same_shape_reinstall_reaches_a_captured_graph():
    """A HIP graph of step() + regenerate, replayed after a same-size re-install, draws from the new pool -- exactly as
    the same calls made eagerly."""
    from pogema_amd import GridConfig, VecPogema
    B, A, T, seed = 16, 3, 2, 9
    first = make_pool(4, 9, 9, seed=1)
    second = make_pool(4, 9, 9, seed=2)
    second[:, 0, 0] = 1  # a mark no map of the first pool has
    first[:, 0, 0] = 0
    gc = GridConfig(num_agents=A, obs_radius=2, seed=seed, max_episode_steps=T)
    graphed = VecPogema(gc, batch=B, auto_reset="regenerate", map_pool=first)
    eager = VecPogema(gc, batch=B, auto_reset="regenerate", map_pool=first)
    graphed.reset(seed=seed)
    eager.reset(seed=seed)
    static_actions = torch.zeros((B, A), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed.step(static_actions)
    torch.cuda.current_stream().wait_stream(side)
    eager.step(static_actions)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = graphed.step(static_actions)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for t in range(4 * T):
        if t == T:
            graphed.set_map_pool(second)
            eager.set_map_pool(second)
        acts = torch.randint(0, 5, (B, A), generator=gen, device="cuda")
        static_actions.copy_(acts)
        g.replay()
        ref = eager.step(acts)
        for a, b in zip(out[:4], ref[:4]):
            assert torch.equal(a, b), f"step {t}"
    maps, agents, targets, index = device_state(graphed)
    emaps, eagents, etargets, eindex = device_state(eager)
    assert np.array_equal(maps, emaps) and np.array_equal(agents, eagents) and np.array_equal(index, eindex)
    assert (index >= 0).all() and all(np.array_equal(maps[b], second[index[b]]) for b in range(B))
    assert graphed.regenerate_failures() == 0
    graphed.close()
    eager.close()


def test_snapshot_carries_map_index():
    from pogema_amd import GridConfig, VecPogema
    B, A, seed = 8, 3, 2
    pool = make_pool(5, 10, 10, seed=8)
    gc = GridConfig(size=10, num_agents=A, obs_radius=2, seed=seed, max_episode_steps=3, on_target="restart")
    plain = VecPogema(gc, batch=B)
    plain.reset(seed=seed)
    env = VecPogema(gc, batch=B, map_pool=pool, auto_reset="regenerate")
    never = VecPogema(gc, batch=B)
    assert int(plain._lib.pgx_snapshot_bytes(plain._handle)) == int(never._lib.pgx_snapshot_bytes(never._handle))
    assert int(env._lib.pgx_snapshot_bytes(env._handle)) == int(plain._lib.pgx_snapshot_bytes(plain._handle)) + 32
    env.reset(seed=seed)
    for _ in range(4):
        env.step(torch.zeros((B, A), dtype=torch.int64, device="cuda"))
    snap = env.save_state()
    saved = device_state(env)
    for _ in range(4):
        env.step(torch.ones((B, A), dtype=torch.int64, device="cuda"))
    assert not all(np.array_equal(x, y) for x, y in zip(device_state(env), saved))
    env.load_state(snap)
    for x, y in zip(device_state(env), saved):
        assert np.array_equal(x, y)
    # a snapshot taken without a pool loads into a handle with one: its envs then run no pool map
    env.load_state(plain.save_state())
    maps, agents, _, index = device_state(env)
    pmaps, pagents, _, pindex = device_state(plain)
    assert (index == -1).all() and (pindex == -1).all()
    assert np.array_equal(maps, pmaps) and np.array_equal(agents, pagents)
    # and a pool snapshot does not load into a handle without a pool
    with pytest.raises(Exception, match="snapshot"):
        never.load_state(snap)
    for e in (plain, env, never):
        e.close()


def test_non_pool_installs_clear_map_index():
    from pogema_amd import GridConfig, VecPogema
    B, A = 6, 2
    pool = make_pool(3, 8, 8, seed=4)
    env = VecPogema(GridConfig(num_agents=A, obs_radius=2, seed=1, density=0.2), batch=B, map_pool=pool)
    env.reset(seed=1)
    assert (env.map_index.cpu().numpy() >= 0).all()
    o, a, t = env.generate(3)
    env.reset_from_state(o, a, t)
    assert (env.map_index.cpu().numpy() == -1).all()
    env.close()


def test_pipelined_matches_one_engine():
    from pogema_amd import GridConfig, PipelinedVecPogema, VecPogema
    B, A, seed = 8, 4, 6
    pool = make_pool(5, 12, 10, seed=6)
    gc = GridConfig(num_agents=A, obs_radius=3, seed=seed, max_episode_steps=4)
    one = VecPogema(gc, batch=B, env_index_base=3, map_pool=pool, auto_reset="regenerate")
    pipe = PipelinedVecPogema(gc, batch=B, parts=2, env_index_base=3, map_pool=pool, auto_reset="regenerate")
    o1, _ = one.reset(seed=seed)
    parts = pipe.reset(seed=seed)
    pipe.synchronize()
    assert torch.equal(o1, torch.cat([p[0] for p in parts]))
    actions = random_actions(10, B, A, 2)
    for t in range(actions.shape[0]):
        a = torch.from_numpy(actions[t]).cuda()
        o1, r1, *_ = one.step(a)
        res = pipe.step(a)
        pipe.synchronize()
        assert torch.equal(o1, torch.cat([r[0] for r in res])) and torch.equal(r1, torch.cat([r[1] for r in res])), t
    for k, v in one.get_state().items():
        assert torch.equal(v, pipe.get_state()[k]), k
    assert torch.equal(one.map_index, torch.cat([e.map_index for e in pipe.engines]))
    one.close()
    pipe.close()


def test_expert_on_pool_maps():
    from expert_reference import expert_reference
    from pogema_amd import GridConfig, VecPogema
    B, A = 10, 6
    pool = make_pool(6, 20, 17, seed=12)
    env = VecPogema(GridConfig(num_agents=A, obs_radius=3, seed=3), batch=B, map_pool=pool)
    env.reset(seed=3)
    maps, agents, targets, _ = device_state(env)
    active = env.get_state()["is_active"].cpu().numpy()
    for flag in (False, True):
        acts, dist = env.expert_actions(agents_as_obstacles=flag)
        ra, rd = expert_reference(maps, agents, targets, active, agents_as_obstacles=flag)
        assert np.array_equal(dist.cpu().numpy(), rd) and np.array_equal(acts.cpu().numpy(), ra), flag
    env.close()
