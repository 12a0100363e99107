"""GPU: pgx_step_held -- a recycled output set that still holds the engine's previous write is not sent its target-plane
zeros again -- gives bit for bit what pgx_step gives.

Every case drives an engine with the feature on and a twin built with `held_zeros=False` through the same operations and
compares the five outputs of every step with torch.equal; the two smallest shapes also run against the C oracle as
tests/util.py does.  Shapes: the smallest that reach each form of the kernel (single wave, helper waves, the three-wave
form of large launches, real multi-wave environments, an unaligned environment base)."""
import os
import subprocess
import sys

import pytest

from util import assert_rollouts_equal, c_oracle_rollout, engine_rollout, generate_instances, random_actions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (batch, map side, agents, obs_radius, on_target, max_episode_steps)
SHAPES = {
    "single_wave_g8": (32, 16, 8, 5, "finish", 7),
    "helper_waves": (48, 32, 64, 5, "restart", 64),
    "three_waves": (2048, 32, 64, 5, "nothing", 64),
    "multi_wave_a100": (6, 32, 100, 7, "restart", 9),
    "unaligned_w7": (5, 12, 3, 3, "finish", 6),
}


def _pair(name, **kw):
    import torch
    from pogema_amd import GridConfig, VecPogema
    batch, size, agents, r, on_target, limit = SHAPES[name]
    envs = []
    for held in (True, False):
        gc = GridConfig(size=size, num_agents=agents, obs_radius=r, density=0.2, seed=11, on_target=on_target,
                        max_episode_steps=limit, collision_system="soft")
        if name == "three_waves":  # 190 MB tensors: no zone walk for a test (seconds per engine)
            kw = dict(kw, placement_budget_gib=0)
        env = VecPogema(gc, batch=batch, auto_reset=True, held_zeros=held, **kw)
        env.reset(seed=5)
        envs.append(env)
    on, off = envs
    assert on.held_zeros["enabled"] and not off.held_zeros["enabled"]
    on.warm_buffers()
    for members, _, _ in on._recycler._sets:  # whatever the masters hold before their first use must not matter
        members[0].fill_(float("nan"))
    gen = torch.Generator(device="cpu").manual_seed(3)
    return on, off, lambda: torch.randint(0, 5, (batch, agents), generator=gen).to("cuda")


def _same(a, b, what):
    import torch
    for k, name in enumerate(("obs", "rewards", "terminated", "truncated")):
        if a[k] is None and b[k] is None:
            continue
        assert torch.equal(a[k], b[k]), f"{what}: {name} differs from the plain step"
    for key in ("is_active", "episode_done", "metrics"):
        assert torch.equal(a[4][key], b[4][key]), f"{what}: {key} differs from the plain step"


def _step_both(on, off, act, what, **kw):
    a, b = on.step(act, **kw), off.step(act, **kw)
    _same(a, b, what)
    return a


@pytest.mark.parametrize("name", list(SHAPES))
def test_held_steps_equal_plain_steps_over_rotating_sets(name):
    """3 (or 2) output sets x at least 4 rotations of random actions; auto-reset (`restore`) fires on the short limits."""
    on, off, actions = _pair(name)
    sets = len(on._recycler)
    steps = sets * 4 + 1
    for t in range(steps):
        _step_both(on, off, actions(), f"{name} step {t}")
    info = on.held_zeros
    assert info["steps"] == steps and info["refreshes"] == sets, info  # only the first write of each set rewrote everything
    assert off.held_zeros["steps"] == 0
    on.close()
    off.close()


@pytest.mark.parametrize("name", ["single_wave_g8", "helper_waves", "multi_wave_a100", "unaligned_w7"])
def test_whatever_touches_a_set_or_the_state_in_between(name):
    import torch
    on, off, actions = _pair(name)
    rec = on._recycler
    sets = len(rec)
    for t in range(sets + 1):
        _step_both(on, off, actions(), f"{name} warm {t}")
    # a caller writes into a returned observation before dropping it: that set's next write is a refresh
    out = _step_both(on, off, actions(), f"{name} before mul_")
    out[0].mul_(2)
    del out
    before = on.held_zeros["refreshes"]
    for t in range(sets):
        _step_both(on, off, actions(), f"{name} after mul_ {t}")
    assert on.held_zeros["refreshes"] == before + 1
    # steps without observations in between leave the sets as they are
    for t in range(2):
        _step_both(on, off, actions(), f"{name} no-obs {t}", compute_obs=False)
    before = on.held_zeros["refreshes"]
    _step_both(on, off, actions(), f"{name} after no-obs")
    assert on.held_zeros["refreshes"] == before
    # every set held by the caller: the step falls back to fresh tensors (the plain kernel) ...
    kept = [_step_both(on, off, actions(), f"{name} keep {k}") for k in range(sets)]
    misses, taken = rec.misses, on.held_zeros["steps"]
    _step_both(on, off, actions(), f"{name} all sets held")
    assert rec.misses == misses + 1 and on.held_zeros["steps"] == taken
    del kept
    # ... observe() takes a set the plain way: untrusted afterwards
    assert torch.equal(on.observe(), off.observe())
    before = on.held_zeros["refreshes"]
    for t in range(sets):
        _step_both(on, off, actions(), f"{name} after observe {t}")
    assert on.held_zeros["refreshes"] == before + 1
    # state changes need nothing: the record describes the buffer, not the state
    mask = torch.zeros(on.batch, dtype=torch.bool, device="cuda")
    mask[::2] = True
    assert torch.equal(on.reset_where(mask, seed=21), off.reset_where(mask, seed=21))
    for t in range(sets):
        _step_both(on, off, actions(), f"{name} after reset_where {t}")
    targets = on.get_state()["targets_xy"].roll(1, dims=1)  # every agent gets its neighbour's target: free cells of its own map
    on.set_targets(targets)
    off.set_targets(targets)
    snap_on, snap_off = on.save_state(), off.save_state()
    for t in range(sets):
        _step_both(on, off, actions(), f"{name} after set_targets {t}")
    on.load_state(snap_on)
    off.load_state(snap_off)
    for t in range(sets + 1):
        _step_both(on, off, actions(), f"{name} after load_state {t}")
    # a rollout in between (it may borrow sets for its ring: taken the plain way)
    acts = torch.stack([actions() for _ in range(3)])
    ra, rb = on.rollout(acts, obs_slots=2), off.rollout(acts, obs_slots=2)
    assert torch.equal(ra["obs"], rb["obs"]) and torch.equal(ra["rewards"], rb["rewards"])
    del ra, rb
    for t in range(sets + 1):
        _step_both(on, off, actions(), f"{name} after rollout {t}")
    on.close()
    off.close()


def test_rollout_ring_borrowed_from_the_sets_makes_them_untrusted():
    """The three-wave shape: its 190 MB observation tensors are large enough for rollout() to borrow its ring from the
    recycler's sets (torch never sees the rollout kernel's writes: plain take() must have forgotten the records)."""
    import torch
    on, off, actions = _pair("three_waves")
    sets = len(on._recycler)
    for t in range(sets + 1):
        _step_both(on, off, actions(), f"warm {t}")
    acts = torch.stack([actions() for _ in range(2)])
    ra, rb = on.rollout(acts, obs_slots=2), off.rollout(acts, obs_slots=2)
    borrowed = ra["obs"].data_ptr() in set(on._recycler.obs_pointers())
    assert torch.equal(ra["obs"], rb["obs"])
    del ra, rb
    before = on.held_zeros["refreshes"]
    for t in range(sets):
        _step_both(on, off, actions(), f"after rollout {t}")
    assert borrowed, "two idle sets and obs_slots=2: the ring must come from the recycler's sets"
    assert on.held_zeros["refreshes"] == before + 2
    on.close()
    off.close()


@pytest.mark.parametrize("name", ["unaligned_w7", "single_wave_g8"])
@pytest.mark.parametrize("on_target", ["finish", "restart", "nothing"])
def test_against_the_c_oracle(name, on_target, monkeypatch):
    """The only reference that shares no code with the engine.  These shapes lie below the size from which step() takes the
    held kernel by itself, so PGX_HELD_ZEROS=1 (read at create) forces it; what the engine reports when engine_rollout
    closes it proves that the 13 steps were held launches and that most of them left zeros out."""
    from pogema_amd import VecPogema
    batch, size, agents, r, _, limit = SHAPES[name]
    obstacles, starts, targets = generate_instances(batch, size, size, agents, 0.2, 77)
    actions = random_actions(13, batch, agents, 5)
    kw = dict(obs_radius=r, collision_system="soft", on_target=on_target, max_episode_steps=limit, auto_reset=True)
    ref = c_oracle_rollout(obstacles, starts, targets, actions, **kw)
    reports, close = [], VecPogema.close

    def reporting_close(self, *a, **k):
        reports.append(self.held_zeros)
        return close(self, *a, **k)

    monkeypatch.setenv("PGX_HELD_ZEROS", "1")
    monkeypatch.setattr(VecPogema, "close", reporting_close)
    got = engine_rollout(obstacles, starts, targets, actions, **kw)
    assert_rollouts_equal(ref, got, f"{name}/{on_target}")
    assert reports and reports[0]["enabled"], reports  # (close() runs again when the engine is collected: the first report counts)
    assert reports[0]["steps"] == 13 and reports[0]["refreshes"] <= 3, reports  # one full write per output set, at the most


def test_step_takes_the_held_kernel_by_itself_only_for_large_observation_tensors(monkeypatch):
    """held_zeros=None, PGX_HELD_ZEROS unset: on from VecPogema.HELD_MIN_BYTES of observations (docs/EXPERIMENTS.md: 95 MB
    neutral, 190 MB faster, smaller launches slower)."""
    from pogema_amd import GridConfig, VecPogema
    monkeypatch.delenv("PGX_HELD_ZEROS", raising=False)
    assert VecPogema.HELD_MIN_BYTES == 128 << 20
    for batch, want in ((1024, False), (2048, True)):  # 95 MB and 190 MB of float32 observations
        env = VecPogema(GridConfig(size=32, num_agents=64, obs_radius=5, seed=1), batch=batch, placement_budget_gib=0)
        assert env.held_zeros["enabled"] == want, (batch, env.held_zeros)
        env.close()
    env = VecPogema(GridConfig(size=32, num_agents=64, obs_radius=5, seed=1), batch=2048, placement_budget_gib=0, held_zeros=False)
    assert not env.held_zeros["enabled"]
    env.close()


def test_environment_variable_switches_it_off():
    code = ("from pogema_amd import GridConfig, VecPogema\nimport torch\n"
            "env = VecPogema(GridConfig(size=16, num_agents=8, obs_radius=5, seed=1), batch=8)\nenv.reset(seed=1)\n"
            "for _ in range(4): env.step(torch.zeros((8, 8), dtype=torch.int64, device='cuda'))\n"
            "print('HELD', env.held_zeros)\n")
    outs = {}
    for val in ("0", "1"):
        p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PGX_HELD_ZEROS=val, PYTHONPATH=ROOT),
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[val] = next(ln for ln in p.stdout.splitlines() if ln.startswith("HELD"))
    assert "'enabled': False" in outs["0"] and "'steps': 0" in outs["0"], outs
    assert "'enabled': True" in outs["1"] and "'steps': 4" in outs["1"], outs
