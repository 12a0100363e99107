"""GPU: token observations (VecPogema.agent_tokens / pgx_agent_tokens, docs/SPEC.md S21) equal, byte for byte, the
torch composition of the four queries S21 is written in and the CPU reference (tests/agent_tokens_reference.py) on
get_state() and the installed maps -- both field-build layouts, 2- and 4-byte fields, every radius class, one to several
workgroups per env, every list size, rows at every alignment; the clip, the history, inactive and unreachable agents;
the shared field cache follows S11's contract, the engine state is left alone, a graph replay equals the eager call;
`out` at any alignment; the list view."""
import numpy as np
import pytest

from agent_tokens_reference import BLOCKED, GREEDY0, PAD, agent_tokens_reference, token_length
from test_goal_directions_gpu import MODES
from util import generate_instances, installed_maps, lazy_torch, mixed_actions

pytestmark = pytest.mark.gpu


def _reference(env, slots, history=None, length=None):
    st = env.get_state()
    h = None if history is None else history.cpu().numpy()
    return agent_tokens_reference(installed_maps(env), st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy(),
                                  st["is_active"].cpu().numpy(), env.obs_radius, slots=slots, history=h, length=length)


def _random_history(env, rng, full_range=False):
    torch = lazy_torch()
    lo, hi = (-128, 128) if full_range else (-1, 6)
    h = rng.integers(lo, hi, size=(env.batch, env.num_agents, 5)).astype(np.int8)
    return torch.as_tensor(h, device=env.device)


def _assert_equal(got, want, what):
    torch = lazy_torch()
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} mismatches, first {bad[0].tolist()}: "
                           f"{got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


def _check(env, slots, what, history=None, length=None):
    """agent_tokens() == the CPU reference, byte for byte; returns the reference."""
    want = _reference(env, slots, history, length)
    got = env.agent_tokens(slots=slots, history=history, length=length)
    assert tuple(got.shape) == (env.batch, env.num_agents, token_length(env.obs_radius, slots) if length is None else length)
    _assert_equal(got, want, what)
    return want


def _compose(env, slots, history=None, length=None):
    """S21 in torch, from the four queries on the same engine."""
    torch = lazy_torch()
    B, A, W, r = env.batch, env.num_agents, env.window, env.obs_radius
    dev = env.device
    ctg = env.cost_to_go().long()
    own = ctg[:, :, r, r]
    st = env.get_state()
    active = st["is_active"].bool()
    xy, tg = st["agents_xy"].long(), st["targets_xy"].long()
    m = env.goal_directions("bits")[:, :, r, r].long()
    win = ctg.reshape(B, A, W * W)
    blocked = (win == -1) | (own == -1).unsqueeze(-1)
    wtok = torch.where(blocked, torch.full_like(win, 41), (win - own.unsqueeze(-1)).clamp(-20, 20) + 20)
    j = torch.arange(A, device=dev).view(1, A, 1).expand(B, A, 1)
    off = torch.zeros((B, A, 1, 2), dtype=torch.long, device=dev)
    if slots > 1:
        index, offset, _ = env.visible_agents(k=slots - 1)
        j = torch.cat((j, index.long()), 2)
        off = torch.cat((off, offset.long()), 2)
    present = j >= 0
    jj = j.clamp(min=0)
    b = torch.arange(B, device=dev).view(B, 1, 1)
    goal = (tg[b, jj] - xy.unsqueeze(2)).clamp(-20, 20) + 20
    if history is None:
        ht = torch.full((B, A, 5), 42, dtype=torch.long, device=dev)
    else:
        h = history.long()
        ht = torch.where((h >= 0) & (h <= 4), 43 + h, torch.full_like(h, 42))
    slot = torch.cat((off + 20, goal, ht[b, jj], (48 + m[b, jj]).unsqueeze(-1)), -1)
    slot = torch.where(present.unsqueeze(-1), slot, torch.full_like(slot, 64))
    l0 = W * W + 10 * slots
    length = l0 if length is None else length
    tail = torch.full((B, A, length - l0), 64, dtype=torch.long, device=dev)
    row = torch.cat((wtok, slot.reshape(B, A, 10 * slots), tail), 2)
    return torch.where(active.unsqueeze(-1), row, torch.full_like(row, 64)).to(torch.uint8)


# ---- 1: the composition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,agents,radius,slots,length", [(16, 6, 5, 13, 256), (20, 13, 2, 4, None), (70, 9, 3, 1, None)])
def test_equals_the_composition_of_the_queries(size, agents, radius, slots, length):
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=size, num_agents=agents, obs_radius=radius, density=0.3, seed=size, on_target="restart",
                    max_episode_steps=64)
    env = VecPogema(gc, batch=5)
    env.reset(seed=size)
    rng = np.random.default_rng(size)
    for t in range(4):
        history = None if t == 0 else _random_history(env, rng)
        got = env.agent_tokens(slots=slots, history=history, length=length)
        _assert_equal(got, _compose(env, slots, history, length), f"size {size} step {t}")
        env.step(mixed_actions(env, rng, p_expert=0.7))
    env.close()


# ---- 2: the CPU reference over the shapes ----------------------------------------------------------------------------
def _reset_and_steps(gc, batch, seed, slots, length, what, steps=3):
    from pogema_amd import VecPogema
    env = VecPogema(gc, batch=batch)
    env.reset(seed=seed)
    rng = np.random.default_rng(seed)
    _check(env, slots, f"{what} reset", history=_random_history(env, rng), length=length)
    for _ in range(steps):
        env.step(mixed_actions(env, rng, p_expert=0.7))
    _check(env, slots, f"{what} after {steps} steps", history=_random_history(env, rng), length=length)
    env.close()


# sides 64 and 65 switch between the two field-build layouts; batch 3 leaves a tail in every launch; L0 = 49 + 10 * slots is
# odd, so the rows start at every alignment
@pytest.mark.parametrize("size", [2, 8, 33, 64, 65])
def test_square_maps_match_reference(size):
    from pogema_amd import GridConfig
    for k, agents in enumerate((1, 6, 13)):
        collision, on_target = MODES[(k + size) % 3]
        if size == 2:
            agents = 1                       # four cells: most of the window is outside the map
        gc = GridConfig(size=size, num_agents=agents, obs_radius=3, density=0.0 if size == 2 else 0.3, seed=size,
                        collision_system=collision, on_target=on_target, max_episode_steps=256)
        _reset_and_steps(gc, 3, size + k, (13, 5, 2)[k], (None, 256, None)[k], f"size {size} A={agents} {collision}/{on_target}")


def test_wide_cell_map():
    """257 x 256 has more than 65536 cells: 4-byte fields."""
    from pogema_amd import GridConfig
    rng = np.random.default_rng(257)
    grid = (rng.random((257, 256)) < 0.25).astype(int).tolist()
    gc = GridConfig(map=grid, num_agents=3, obs_radius=2, seed=6, collision_system="soft", on_target="nothing",
                    max_episode_steps=64)
    _reset_and_steps(gc, 2, 6, 3, None, "257 x 256", steps=2)


@pytest.mark.parametrize("radius", [1, 2, 5, 15])
def test_obs_radius(radius):
    from pogema_amd import GridConfig
    for k, agents in enumerate((1, 6, 13)):
        collision, on_target = MODES[(k + radius) % 3]
        gc = GridConfig(size=20, num_agents=agents, obs_radius=radius, density=0.3, seed=radius,
                        collision_system=collision, on_target=on_target, max_episode_steps=64)
        l0 = token_length(radius, 13)
        _reset_and_steps(gc, 3, radius + k, 13, (None, l0 + 3, 256 if l0 <= 256 else 2048)[k], f"radius {radius} A={agents}")


@pytest.mark.parametrize("agents,size,radius", [(70, 24, 3), (300, 40, 2)])
def test_several_waves_and_several_workgroups_per_env(agents, size, radius):
    from pogema_amd import GridConfig
    for k, (slots, length) in enumerate(((13, None), (32, 512))):
        collision, on_target = MODES[k]
        gc = GridConfig(size=size, num_agents=agents, obs_radius=radius, density=0.2, seed=agents, collision_system=collision,
                        on_target=on_target, max_episode_steps=64)
        _reset_and_steps(gc, 3, agents + k, slots, length, f"A={agents} slots={slots}", steps=2)


# 40 agents on 12 x 12 at radius 5: up to 39 visible, so every list size overflows and every slot is filled somewhere
@pytest.mark.parametrize("slots", [1, 2, 9, 10, 13, 17, 18, 32])
def test_slots_and_lengths(slots):
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=12, num_agents=40, obs_radius=5, density=0.1, seed=slots, collision_system="soft",
                    on_target="restart", max_episode_steps=64)
    env = VecPogema(gc, batch=3)
    env.reset(seed=slots)
    rng = np.random.default_rng(slots)
    env.step(mixed_actions(env, rng, p_expert=0.7))
    history = _random_history(env, rng)
    l0 = token_length(5, slots)
    assert l0 == 121 + 10 * slots
    for length in (None, 256, l0 + 3, 2048):
        if length is not None and length < l0:
            continue
        ref = _check(env, slots, f"slots {slots} length {length}", history=history, length=length)
    assert (ref[:, :, l0 - 10:l0] != PAD).any(), "the last slot is filled nowhere: the list size is not exercised"
    env.close()


# ---- 3: the clip -------------------------------------------------------------------------------------------------------
def test_the_clip_is_exercised():
    """64 x 64 at radius 15 and density 0.1: window cells 30 steps from the centre, targets more than 20 cells away.  The
    instance is drawn on the host (seed 3), so the reference alone shows that both ends of both clips occur."""
    from pogema_amd import GridConfig, VecPogema
    B, A, r, slots = 2, 8, 15, 4
    obstacles, agents, targets = generate_instances(B, 64, 64, A, 0.1, 3)
    ref = agent_tokens_reference(obstacles, agents, targets, np.ones((B, A), bool), r, slots=slots)
    ww = 31 * 31
    win = ref[:, :, :ww]
    goals = np.concatenate([ref[:, :, ww + 10 * s + 2:ww + 10 * s + 4] for s in range(slots)], -1)
    assert (win == 0).any() and (win == 40).any(), "the window part never reaches the clip"
    assert (goals == 0).any() and (goals == 40).any(), "the goal entries never reach the clip"
    env = VecPogema(GridConfig(size=64, num_agents=A, obs_radius=r, density=0.1, seed=3), batch=B)
    env.reset_from_state(obstacles, agents, targets)
    _assert_equal(env.agent_tokens(slots=slots), ref, "clip")
    env.close()


# ---- 4: the history ------------------------------------------------------------------------------------------------------
def test_history():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=12, num_agents=9, obs_radius=4, density=0.2, seed=5), batch=4)
    env.reset(seed=5)
    rng = np.random.default_rng(5)
    none = env.agent_tokens(slots=6)
    minus = torch.full((4, 9, 5), -1, dtype=torch.int8, device=env.device)
    assert torch.equal(none, env.agent_tokens(slots=6, history=minus))
    full = _random_history(env, rng, full_range=True)
    full[0, 0] = torch.tensor([-128, -1, 0, 4, 5], dtype=torch.int8)
    full[0, 1, 0] = 127
    want = _check(env, 6, "history -128..127", history=full)
    assert not np.array_equal(want, none.cpu().numpy())
    # a view with strides: every second agent row of a tensor twice as long
    wide = _random_history(env, rng, full_range=True).repeat(1, 2, 1)
    view = wide[:, ::2]
    assert not view.is_contiguous() and tuple(view.shape) == (4, 9, 5)
    assert torch.equal(env.agent_tokens(slots=6, history=view), env.agent_tokens(slots=6, history=view.contiguous()))
    _check(env, 6, "strided history", history=view)
    env.close()


# ---- 5: inactive and unreachable agents ------------------------------------------------------------------------------------
def test_hidden_agents_are_pad_and_absent():
    from pogema_amd import GridConfig, VecPogema
    gc = GridConfig(size=10, num_agents=8, obs_radius=4, density=0.15, seed=7, collision_system="soft", on_target="finish",
                    max_episode_steps=64)
    env = VecPogema(gc, batch=6)
    env.reset(seed=7)
    rng = np.random.default_rng(7)
    for _ in range(8):
        env.step(mixed_actions(env, rng, p_expert=0.9))
    active = env.get_state()["is_active"].cpu().numpy().astype(bool)
    assert (~active).any() and active.any(), "no agent finished: nothing hidden to check"
    slots = 8
    got = _check(env, slots, "after finishes", history=_random_history(env, rng))
    assert (got[~active] == PAD).all()
    index, _, _ = env.visible_agents(k=slots - 1)
    index = index.cpu().numpy()
    listed = np.zeros_like(active)
    for b in range(6):
        listed[b, index[b][index[b] >= 0]] = True
    assert not (listed & ~active).any()
    env.close()


def test_target_in_another_component():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    grid = np.zeros((9, 9), int)
    grid[:, 4] = 1                           # two rooms
    env = VecPogema(GridConfig(map=grid.tolist(), num_agents=4, obs_radius=2, seed=2), batch=3)
    env.reset(seed=2)
    st = env.get_state()
    xy, tgt = st["agents_xy"].cpu().numpy(), st["targets_xy"].cpu().numpy().copy()
    b, i = 1, 2
    tgt[b, i] = (8, 8) if xy[b, i, 1] < 4 else (0, 0)
    env.set_targets(torch.as_tensor(tgt))
    assert np.array_equal(env.get_state()["targets_xy"].cpu().numpy(), tgt), "set_targets did not take the target"
    got = _check(env, 3, "unreachable target")
    assert (got[b, i, :25] == BLOCKED).all() and got[b, i, 25 + 9] == GREEDY0
    want_goal = np.clip(tgt[b, i] - xy[b, i], -20, 20) + 20
    assert got[b, i, 27:29].tolist() == want_goal.tolist()
    assert (got[b, (i + 1) % 4, :25] != BLOCKED).any()
    env.close()


# ---- 6: the cache contract, the state, graph capture -----------------------------------------------------------------------
def _snapshot(env):
    """The engine's snapshot in a zero-filled blob (save_state() leaves the padding between its segments as torch.empty
    gave it)."""
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
    for t in range(3):
        env.step(torch.as_tensor(rng.integers(0, 5, size=(6, 11)), device=env.device))
        before, blob = env.get_state(occupancy=True), _snapshot(env)
        env.agent_tokens(slots=(13, 1, 32)[t], history=_random_history(env, rng) if t else None)
        after = env.get_state(occupancy=True)
        for k in before:
            assert torch.equal(before[k], after[k]), f"step {t}: {k}"
        assert torch.equal(blob, _snapshot(env)), f"step {t}: the snapshot changed"
    env.close()


def test_builds_move_as_goal_directions_would():
    from pogema_amd import GridConfig, VecPogema
    B, A = 5, 8
    gc = GridConfig(size=10, num_agents=A, obs_radius=3, density=0.2, seed=4, collision_system="soft", on_target="restart",
                    max_episode_steps=10**6)
    a, b = VecPogema(gc, batch=B), VecPogema(gc, batch=B)
    a.reset(seed=4)
    b.reset(seed=4)
    assert a.cost_to_go_builds == 0
    a.agent_tokens()
    b.goal_directions()
    assert a.cost_to_go_builds == b.cost_to_go_builds == B * A
    a.agent_tokens(slots=3, length=300)
    assert a.cost_to_go_builds == B * A, "a second call on an unchanged state built fields"
    total = 0
    for t in range(6):
        before = a.get_state()["targets_xy"].cpu().numpy()
        actions, _ = a.expert_actions()
        a.step(actions)
        b.step(actions)
        st = a.get_state()
        changed = int(((st["targets_xy"].cpu().numpy() != before).any(-1) & st["is_active"].cpu().numpy().astype(bool)).sum())
        built = a.cost_to_go_builds
        a.agent_tokens()
        b.goal_directions()
        assert a.cost_to_go_builds - built == changed, f"step {t}"
        assert a.cost_to_go_builds == b.cost_to_go_builds, f"step {t}"
        total += changed
    assert total > 0, "no agent drew a new target: the rebuild is not exercised"
    a.close()
    b.close()


def test_first_call_inside_capture_is_refused_then_replays():
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd._lib import PgxError
    gc = GridConfig(size=16, num_agents=6, obs_radius=3, density=0.3, seed=4, collision_system="soft",
                    on_target="restart", max_episode_steps=10**6)
    env = VecPogema(gc, batch=6)
    env.reset(seed=4)
    history = torch.full((6, 6, 5), -1, dtype=torch.int8, device=env.device)
    out = torch.zeros((6, 6, 256), dtype=torch.uint8, device=env.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(PgxError, match="bytes") as ei:   # the first user of the cache allocates it: not inside a capture
        with torch.cuda.graph(g):
            env.agent_tokens(history=history, length=256, out=out)
    assert ei.value.code == -4
    torch.cuda.synchronize()
    assert env.cost_to_go_builds == 0
    eager = env.agent_tokens(history=history, length=256)   # eager: allocates the cache, builds every field
    assert env.cost_to_go_builds == 36
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.agent_tokens(history=history, length=256, out=out)
    g.replay()
    assert torch.equal(out, eager)
    rng = np.random.default_rng(4)
    for t in range(4):
        actions = mixed_actions(env, rng, p_expert=0.8)
        env.step(actions)
        history.copy_(torch.cat((actions.to(torch.int8).unsqueeze(-1), history[:, :, :-1]), -1))
        out.zero_()
        g.replay()
        assert torch.equal(out, env.agent_tokens(history=history, length=256)), f"replay after step {t}"
    _check(env, 13, "after replays", history=history, length=256)
    env.close()


def test_regenerated_pool_maps_and_copies_replay():
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
    out = torch.zeros((12, 4, 64), dtype=torch.uint8, device=env.device)
    env.agent_tokens(slots=3, length=64)             # eager: allocates the cache
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.agent_tokens(slots=3, length=64, out=out)
    for _ in range(7):                       # two episode ends per env
        env.step(torch.as_tensor(rng.integers(0, 5, size=(12, 4)), device=env.device))
    assert (env.map_index.cpu().numpy() != first).any(), "no env drew another map: the first reset's maps would pass"
    want = _check(env, 3, "after regeneration", length=64)
    out.zero_()
    g.replay()
    _assert_equal(out, want, "replay after regeneration")
    env.step(torch.as_tensor(rng.integers(1, 5, size=(12, 4)), device=env.device))
    before = env.agent_tokens(slots=3, length=64)
    src, dst = [0, 1, 2], [5, 6, 7]
    assert not torch.equal(before[src], before[dst])
    env.copy_envs(src, dst)
    want = _check(env, 3, "after copy_envs", length=64)
    assert np.array_equal(want[dst], before[src].cpu().numpy())
    out.zero_()
    g.replay()
    _assert_equal(out, want, "replay after copy_envs")
    env.close()


# ---- 7: out= ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots,length", [(13, None), (13, 256), (2, 72)])
def test_out_at_any_alignment(slots, length):
    torch = lazy_torch()
    from pogema_amd import GridConfig, VecPogema
    env = VecPogema(GridConfig(size=16, num_agents=6, obs_radius=3, density=0.3, seed=5), batch=5)
    env.reset(seed=5)
    want = env.agent_tokens(slots=slots, length=length)
    assert want.data_ptr() % 16 == 0
    own = torch.full_like(want, 7)
    assert env.agent_tokens(slots=slots, length=length, out=own) is own and torch.equal(own, want)
    n, fill = want.numel(), 7
    for shift in (1, 2, 3, 4, 15):
        buf = torch.full((n + 32,), fill, dtype=torch.uint8, device=env.device)
        assert buf.data_ptr() % 16 == 0
        view = buf[shift:shift + n].view(want.shape)
        assert view.data_ptr() % 16 == shift
        assert env.agent_tokens(slots=slots, length=length, out=view) is view
        assert torch.equal(view, want), f"shift {shift}"
        assert bool((buf[:shift] == fill).all()) and bool((buf[shift + n:] == fill).all()), f"shift {shift}: bytes around out"
    for bad in (torch.empty(want.shape, dtype=torch.int8, device=env.device),
                torch.empty(want.shape[:-1] + (want.shape[-1] + 1,), dtype=torch.uint8, device=env.device),
                torch.empty(want.shape, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out"):
            env.agent_tokens(slots=slots, length=length, out=bad)
    env.close()


def test_errors_name_the_argument():
    from pogema_amd import GridConfig, VecPogema, _lib
    from pogema_amd._lib import PgxError
    env = VecPogema(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21), batch=2)
    with pytest.raises(PgxError) as ei:
        env.agent_tokens()
    assert ei.value.code == -4               # before a reset, like step()
    env.reset(seed=21)
    torch = lazy_torch()
    out = torch.zeros((2, 5, 256), dtype=torch.uint8, device=env.device)
    lib, h, s = env._lib, env._handle, env._stream()
    for args, needle in (((0, 256, 0, None, out.data_ptr(), s), "slots"), ((33, 2048, 0, None, out.data_ptr(), s), "slots"),
                         ((13, 178, 0, None, out.data_ptr(), s), "length"), ((13, 2049, 0, None, out.data_ptr(), s), "length"),
                         ((13, 256, 1, None, out.data_ptr(), s), "flags"), ((13, 256, 0, None, None, s), "tokens")):
        assert lib.pgx_agent_tokens(h, *args) == -1
        msg = lib.pgx_last_error().decode()
        assert "pgx_agent_tokens" in msg and needle in msg, msg
    assert not bool(out.any())
    env.close()


# ---- 8: the list view ------------------------------------------------------------------------------------------------------
def test_list_view():
    from pogema_amd import GridConfig, pogema_v0
    one = pogema_v0(GridConfig(size=16, num_agents=5, obs_radius=3, density=0.3, seed=21, on_target="nothing"))
    one.reset(seed=21)
    one.step([1, 2, 3, 4, 0])
    rows = one.agent_tokens()
    assert isinstance(rows, np.ndarray) and rows.dtype == np.uint8 and rows.shape == (5, 49 + 130)
    assert np.array_equal(rows, one._vec.agent_tokens()[0].cpu().numpy())
    hist = [[1, -1, -1, -1, -1], [2, -1, -1, -1, -1], [3, -1, -1, -1, -1], [4, -1, -1, -1, -1], [0, -1, -1, -1, -1]]
    rows = one.agent_tokens(slots=4, history=hist, length=96)
    assert rows.shape == (5, 96) and rows[:, 49 + 4].tolist() == [44, 45, 46, 47, 43]
    assert (rows[:, 49 + 40:] == PAD).all()
    one.close()
