"""CPU: the stateful fuzz proves itself without a GPU (tests/stateful_model.py; the GPU run is tests/test_stateful_gpu.py).

* A host stand-in engine -- the part of VecPogema's surface that run() uses, on a second Model plus the reference
  functions, CPU torch tensors, the product's own RecyclingOutputs over CPU buffers and a held-zeros write that, like
  pgx_step_held, leaves out what a trusted set already holds -- passes run() for every committed (profile, seed).
* Seeded faults: the stand-in with one of twelve defects must make run() fail on a committed case, at an operation of the
  kind the defect belongs to.  All twelve are modelled.  Two of them only through the bookkeeping, because the stand-in
  computes every query from the state and keeps no fields it could serve stale: fault 1 (cache rows copied without their
  tags) and fault 5 (a map change that load_state hides from the cache) show as a wrong `cost_to_go_builds` delta, not as
  a wrong field.
* The committed sequences reach what they are meant to reach (counted from the op lists and the model's own run).
* The model is not the only witness: its steps equal the plain-C oracle's.
* draw_ops is deterministic and its ops are plain JSON.
"""
import copy
import json
import time

import numpy as np
import pytest
import torch

import stateful_model as S
from stateful_model import CACHE_QUERIES, PROFILES, QUERIES, Model, StatefulMismatch, committed_seeds, draw_ops, \
    profile_config, query_kind, run

CASES = [(p, s) for p in PROFILES for s in committed_seeds(p)]
_OPS = {}


def ops_of(profile, seed):
    if (profile, seed) not in _OPS:
        _OPS[(profile, seed)] = draw_ops(profile, seed)
    return _OPS[(profile, seed)]


# ---- the stand-in -------------------------------------------------------------------------------------------------------
class FaultyModel(Model):
    """The stand-in's own Model, with the state-side defects."""

    def __init__(self, cfg, fault=None):
        super().__init__(cfg)
        self.fault = fault

    def _copy_cache_row(self, s, d):
        if self.fault == 1:       # the fields and the map bits travel, the tags stay
            self.built_map[d] = self.built_map[s]
            return
        super()._copy_cache_row(s, d)

    def _copy_one(self, s, d):
        super()._copy_one(s, d)
        if self.fault == 2:       # the copy takes its source's global env index along
            self.env[d].env_index = self.env[s].env_index
        if self.fault == 3:       # ... its source's generation
            self.epoch[d] = self.epoch[s]

    def _restore(self, snap):
        elapsed = [e._elapsed_steps for e in self.env]
        super()._restore(snap)
        if self.fault == 4:       # `elapsed` is not restored
            for e, n in zip(self.env, elapsed):
                e._elapsed_steps = n
        if self.fault == 5:       # the cache is told the new maps without dropping the fields built on the old ones
            maps = self.maps()
            self.built_map = [None if self.built_map[b] is None else maps[b].tobytes() for b in range(self.B)]

    def _advance(self, b):
        if self.fault == 9 and self.epoch[b] > 0:   # an env regenerated before keeps its generation
            return
        super()._advance(b)

    def _counts(self, st, b, i):
        return True if self.fault == 10 else super()._counts(st, b, i)

    def set_targets(self, targets, mask=None):
        super().set_targets(targets, None if self.fault == 11 else mask)

    def rollout(self, actions):
        if self.fault != 12:
            return super().rollout(actions)
        # auto-reset inside the rollout restores the state the rollout started from, not the instance's initial state
        true_init = [e._init_args for e in self.env]
        for e in self.env:
            st = e.get_state()
            e._init_args = (e._init_args[0], [tuple(map(int, p)) for p in st["agents_xy"]],
                            [tuple(map(int, p)) for p in st["targets_xy"]])
        out = super().rollout(actions)
        for e, init in zip(self.env, true_init):
            e._init_args = init
        return out


def _recycler_class(fault):
    from pogema_amd.buffers import RecyclingOutputs

    class Recycler(RecyclingOutputs):
        if fault == 6:            # a set stays trusted although observe() took it the plain way and wrote it
            def take(self, with_obs=True):
                i = self._take_index()
                return None if i is None else self._hand_out(i, with_obs)
        if fault == 7:            # ... although torch saw the caller's write: the version counter is not looked at
            @staticmethod
            def _version(t):
                return 0
        if fault == 8:            # a set is handed out while the caller still references it
            def _is_idle(self, i):
                return True
    return Recycler


class StandIn:
    """The part of VecPogema's surface that run() uses, on the host."""

    def __init__(self, cfg, fault=None):
        self.cfg, self.fault = cfg, fault
        self.m = FaultyModel(cfg, fault)
        self.device = torch.device("cpu")
        self.B, self.A, self.w = cfg["B"], cfg["A"], 2 * cfg["r"] + 1
        self.obs_shape = (self.B, self.A, 3, self.w, self.w)
        self._recycler = None
        self._held_on = bool(cfg["held"]) and cfg["auto_reset"] != "regenerate"
        self._held_steps = self._held_refreshes = 0
        self._held_at = {}        # set index -> where the last held write left each agent's target-plane 1
        self.episode_done = torch.zeros(self.B, dtype=torch.bool)
        self.metrics = torch.zeros((self.B, 6), dtype=torch.float32)

    # -- buffers -----------------------------------------------------------------------------------------------------
    def _fresh(self, with_obs=True):
        B, A = self.B, self.A
        return (torch.empty(self.obs_shape, dtype=torch.float32) if with_obs else None, torch.empty((B, A), dtype=torch.float32),
                torch.empty((B, A), dtype=torch.bool), torch.empty((B, A), dtype=torch.bool), torch.empty((B, A), dtype=torch.bool))

    def _build_recycler(self):
        bufs = [torch.full(self.obs_shape, float("nan")) for _ in range(3)]
        return _recycler_class(self.fault)(bufs, self.B, self.A)

    @property
    def held_zeros(self):
        return {"enabled": self._held_on, "steps": self._held_steps, "refreshes": self._held_refreshes}

    def _write(self, outs, res, compute_obs):
        """Like the engine's kernels, behind torch's back: no version counter moves."""
        obs, rew, term, trunc, act = outs
        if compute_obs:
            obs.data.copy_(torch.from_numpy(res["obs"]))
        for t, k in ((rew, "rewards"), (term, "terminated"), (trunc, "truncated"), (act, "is_active")):
            t.data.copy_(torch.from_numpy(res[k]))

    def _held_write(self, obs, index, trusted, new):
        """pgx_step_held's write: planes 0 and 1 whole; of the target plane only the old 1 cleared and the new one set
        when the set is trusted to hold the previous held write, else everything."""
        flat = new[:, :, 2].reshape(self.B, self.A, -1).argmax(-1)
        with torch.no_grad():
            o = obs.data            # (the engine's kernel writes behind torch's back too: no version bump)
            o[:, :, :2] = torch.from_numpy(new[:, :, :2])
            plane = o[:, :, 2].reshape(self.B, self.A, -1).clone()   # what the buffer holds now
            if trusted:
                plane.scatter_(2, torch.from_numpy(self._held_at[index])[..., None], 0.0)
            else:
                plane.zero_()
            plane.scatter_(2, torch.from_numpy(flat)[..., None], 1.0)
            o[:, :, 2] = plane.view(self.B, self.A, self.w, self.w)
        self._held_at[index] = flat

    # -- mutators ----------------------------------------------------------------------------------------------------
    def reset(self, seed=None):
        self.m.reset(seed)
        if self._recycler is None:
            self._recycler = self._build_recycler()
        return self.observe(), {"is_active": torch.ones((self.B, self.A), dtype=torch.bool)}

    def reset_where(self, mask):
        self.m.reset_where([bool(v) for v in mask.tolist()])
        return self.observe()

    def observe(self, out=None):
        if out is None:
            taken = self._recycler.take()
            out = taken[0] if taken is not None else torch.empty(self.obs_shape, dtype=torch.float32)
            del taken
        out.data.copy_(torch.from_numpy(self.m.observe()))
        return out

    def step(self, actions, compute_obs=True, out=None):
        res = self.m.step(actions.numpy().astype(np.int64))
        self.episode_done.copy_(torch.from_numpy(res["episode_done"]))
        done = res["episode_done"]
        self.metrics[torch.from_numpy(done)] = torch.from_numpy(res["metrics"][done])
        infos = {"episode_done": self.episode_done, "metrics": self.metrics}
        if out is not None:
            outs = out
        elif self._held_on:
            held = self._recycler.take_for_step(compute_obs)
            if held is not None and compute_obs:
                outs, _, trusted, index = held
                self._held_write(outs[0], index, trusted, res["obs"])
                self._write(outs, res, False)
                self._recycler.vouch(index)
                self._held_steps += 1
                self._held_refreshes += 0 if trusted else 1
                infos["is_active"] = outs[4]
                return outs[0], outs[1], outs[2], outs[3], infos
            outs = held[0] if held is not None else self._fresh(compute_obs)
        else:
            outs = self._recycler.take(compute_obs) or self._fresh(compute_obs)
        self._write(outs, res, compute_obs)
        infos["is_active"] = outs[4]
        return (outs[0] if compute_obs else None), outs[1], outs[2], outs[3], infos

    def rollout(self, actions):
        res = self.m.rollout(actions.numpy().astype(np.int64))
        return {k: torch.from_numpy(v) for k, v in res.items()}

    def set_targets(self, targets, mask=None):
        self.m.set_targets(np.asarray(targets), None if mask is None else np.asarray(mask))

    def copy_envs(self, src, dst, *, cache=True):
        from pogema_amd.vec_env import copy_pairs
        copy_pairs(src, dst, self.B)          # the engine's own check of the pairs: the fuzz sends only legal ones
        self.m.copy_envs(src, dst, cache)

    def save_state(self):
        return self.m.save_state()

    def load_state(self, k):
        self.m.load_state(k)

    # -- state -------------------------------------------------------------------------------------------------------
    def get_state(self, occupancy=False):
        return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in self.m.state().items()}

    def installed_maps(self):
        return self.m.maps()

    @property
    def map_index(self):
        return torch.tensor(self.m.map_index, dtype=torch.int32)

    @property
    def cost_to_go_builds(self):
        return self.m.builds

    # -- queries -----------------------------------------------------------------------------------------------------
    def _query(self, op, dtypes=()):
        res, _ = self.m.query(op)
        out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in res]
        for k, d in enumerate(dtypes):
            if d is not None and out[k] is not None:
                out[k] = out[k].to(d)
        return tuple(out)

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def expert_actions(self, agents_as_obstacles=False, dtype=torch.int64):
        return self._query({"op": "expert_actions", "agents_as_obstacles": agents_as_obstacles}, (dtype,))

    def cost_to_go(self):
        return self._query({"op": "cost_to_go"})[0]

    def visible_agents(self, k=13):
        return self._query({"op": "visible_agents", "k": k}, (torch.int32, torch.int8, torch.int32))

    def pibt_actions(self, priority=None, dtype=torch.int64, *, swap=False):
        return self._query({"op": "pibt_actions", "priority": self._np(priority), "swap": swap}, (dtype,))

    def pibt_plan(self, horizon, priority=None, growing=True, dtype=torch.int64):
        return self._query({"op": "pibt_plan", "horizon": horizon, "priority": self._np(priority), "growing": growing}, (dtype,))

    def shield_actions(self, scores, priority=None, tie_break=None):
        return self._query({"op": "shield_actions", "scores": scores.numpy(), "priority": self._np(priority),
                            "tie_break": tie_break}, (torch.int64, torch.int32, torch.uint8))

    def goal_directions(self, format="float32"):
        return self._query({"op": "goal_directions", "format": format}, (torch.float32 if format == "float32" else torch.uint8,))[0]

    def goal_paths(self, steps=None, format="float32", planes=True):
        return self._query({"op": "goal_paths", "steps": steps, "format": format, "planes": planes},
                           (torch.float32 if format == "float32" else None,))

    def agent_forecasts(self, steps=3, format="float32", planes=True):
        return self._query({"op": "agent_forecasts", "steps": steps, "format": format, "planes": planes},
                           (torch.float32 if format == "float32" else None,))

    def move_outcomes(self, actions):
        return self._query({"op": "move_outcomes", "actions": actions.numpy()}, (torch.int32, torch.uint8, torch.int32, torch.int32))

    def policy_input(self, channels, dtype=torch.float32):
        return self._query({"op": "policy_input", "channels": list(channels)}, (dtype,))[0]

    def global_state(self, channels, dtype=torch.float32):
        return self._query({"op": "global_state", "channels": list(channels)}, (dtype,))[0]

    def agent_tokens(self, slots=13, history=None, length=None):
        return self._query({"op": "agent_tokens", "slots": slots, "history": self._np(history), "length": length})[0]


def _run_stand_in(profile, seed, fault=None):
    cfg = profile_config(profile, seed)
    run(StandIn(cfg, fault), Model(cfg), ops_of(profile, seed), label=f"stand-in {profile} seed {seed} fault {fault}")


# ---- 1: the driver passes on a correct engine ---------------------------------------------------------------------------
STAND_IN_SECONDS = {}


@pytest.mark.parametrize("profile,seed", CASES)
def test_stand_in_passes(profile, seed):
    t0 = time.perf_counter()
    _run_stand_in(profile, seed)
    STAND_IN_SECONDS[(profile, seed)] = time.perf_counter() - t0
    print(f"stand-in {profile} seed {seed}: {len(ops_of(profile, seed))} ops, {STAND_IN_SECONDS[(profile, seed)]:.2f} s")


# ---- 2: it has teeth ----------------------------------------------------------------------------------------------------
CACHE_READERS = ("cost_to_go", "pibt_actions", "pibt_plan", "shield_actions", "goal_directions", "goal_paths",
                 "agent_forecasts", "policy_input", "agent_tokens")
# fault: (what it is, the profiles that can show it, the kinds of operation at which run() may notice it)
FAULTS = {
    1: ("copy_envs(cache=True) copies the fields but not the tags", PROFILES, CACHE_READERS),
    2: ("a copy takes its source's global env index: the lifelong stream is keyed on the source", ("lifelong", "pool"),
        ("step", "rollout")),
    3: ("a copy takes its source's epoch", ("maps", "pool"), ("step", "reset_where")),
    4: ("load_state does not restore `elapsed`", PROFILES, ("load_state",)),
    5: ("load_state leaves the cache tags of envs whose map the snapshot changes", ("maps", "pool"), CACHE_READERS),
    6: ("a held set is trusted after observe() wrote it", ("lifelong", "wide"), ("step",)),
    7: ("a held set is trusted after the caller's in-place write", ("lifelong", "wide"), ("step",)),
    8: ("the recycler hands out a set the caller still references", PROFILES, ("step", "observe", "reset", "reset_where")),
    9: ("reset_where does not advance the epoch of an env that was regenerated before", ("maps", "pool"), ("reset_where",)),
    10: ("cost_to_go_builds counts inactive agents", ("maps", "wide"), CACHE_READERS),
    11: ("set_targets(mask=...) updates unmasked agents", PROFILES, ("set_targets",)),
    12: ("rollout restores on auto-reset from the state at its start", ("lifelong", "wide"), ("rollout",)),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_seeded_fault_is_caught(fault):
    what, profiles, kinds = FAULTS[fault]
    seen = []
    for profile in profiles:
        for seed in committed_seeds(profile):
            try:
                _run_stand_in(profile, seed, fault)
            except StatefulMismatch as exc:
                seen.append((profile, seed, exc.index, exc.op["op"], exc.what[:120]))
                if exc.op["op"] in kinds:
                    print(f"fault {fault} ({what}): caught in {profile} seed {seed} at op {exc.index} ({exc.op['op']}): {exc.what[:200]}")
                    return
    raise AssertionError(f"fault {fault} ({what}) is not caught at an operation of kind {kinds} by any committed case; "
                         f"failures seen: {seen}")


# ---- 3: what the committed sequences reach ------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", PROFILES)
def test_committed_sequences_cover_the_state_surface(profile):
    mutators, queries, pairs = {}, {}, set()
    ends = redraws = 0
    over_copy = over_regen = False
    admitted = S.admitted_mutators(profile_config(profile, 0))
    for seed in committed_seeds(profile):
        ops = ops_of(profile, seed)
        for k, op in enumerate(ops):
            kind = query_kind(op)
            if kind in S.MUTATORS:
                mutators[kind] = mutators.get(kind, 0) + 1
                if k + 1 < len(ops) and query_kind(ops[k + 1]) in CACHE_QUERIES:
                    pairs.add((kind, query_kind(ops[k + 1])))
            else:
                queries[kind] = queries.get(kind, 0) + 1
        model = Model(profile_config(profile, seed))
        for op in ops:
            S.apply_to_model(model, op)
        ends += sum(1 for e in model.events if e[0] == "end")
        redraws += model.redraws
        saved_at = {e[1]: k for k, e in enumerate(model.events) if e[0] == "save"}
        for k, e in enumerate(model.events):
            if e[0] == "load":
                between = [x[0] for x in model.events[saved_at[e[1]]:k]]
                over_copy |= "copy" in between
                over_regen |= "regen" in between
    for m in admitted:
        assert mutators.get(m, 0) >= 5, (profile, m, mutators)
    assert "rollout" in admitted or "rollout" not in mutators
    for q in QUERIES:
        assert queries.get(q, 0) >= 5, (profile, q, queries)
    missing = [(m, q) for m in admitted for q in CACHE_QUERIES if (m, q) not in pairs]
    assert not missing, (profile, missing)
    assert over_copy, f"{profile}: no load_state reaches back over a copy_envs"
    assert over_regen, f"{profile}: no load_state reaches back over a regeneration"
    assert ends >= 3, (profile, ends)
    if profile == "lifelong":
        assert redraws >= 10, redraws


# ---- 4: the model against the plain-C oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["lifelong", "wide"])
def test_model_steps_equal_the_c_oracle(profile):
    """The steps and rollouts of a committed sequence (the part the C oracle has: steps with auto-reset, from the first
    reset's instances) through the model and through oracle/pogema_oracle.c: observations, rewards and flags."""
    from oracle.c_oracle import COracle
    seed = committed_seeds(profile)[0]
    cfg = profile_config(profile, seed)
    ops = ops_of(profile, seed)
    model = Model(cfg)
    obs0 = S.apply_to_model(model, ops[0])
    st = model.state()
    sem = {k: v for k, v in cfg["semantics"].items()}
    ref = COracle(cfg["B"], cfg["H"], cfg["W"], cfg["A"], cfg["r"], cfg["collision"], cfg["on_target"], cfg["max_steps"], True,
                  cfg["gc_seed"], cfg["base"], empty_outside=cfg["empty_outside"], outside_density=cfg["density"], **sem)
    assert np.array_equal(ref.reset(model.maps(), st["agents_xy"], st["targets_xy"]), obs0)
    steps = ends = 0
    for op in ops[1:]:
        if op["op"] not in ("step", "rollout"):
            continue
        for actions in (np.asarray(op["actions"])[None] if op["op"] == "step" else np.asarray(op["actions"])):
            want = model.step(actions)
            obs, rew, term, trunc, act = ref.step(actions)
            what = f"{profile} seed {seed} step {steps}"
            assert np.array_equal(obs, want["obs"]), what
            assert np.allclose(rew, want["rewards"], rtol=0, atol=1e-6), what
            assert np.array_equal(term, want["terminated"]) and np.array_equal(trunc, want["truncated"]), what
            assert np.array_equal(act, want["is_active"]), what
            assert np.array_equal(ref.episode_done.astype(bool), want["episode_done"]), what
            done = want["episode_done"]
            assert np.array_equal(ref.metrics[done], want["metrics"][done]), what
            cs = ref.get_state()
            ms = model.state()
            for k in ("agents_xy", "targets_xy", "elapsed", "is_active"):
                assert np.array_equal(cs[k], ms[k]), (what, k)
            steps += 1
            ends += int(done.sum())
    ref.close()
    assert steps >= 40 and ends >= 3, (steps, ends)


# ---- 5: determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", PROFILES)
def test_draw_ops_is_deterministic_and_plain_json(profile):
    seed = committed_seeds(profile)[0]
    first = json.dumps(ops_of(profile, seed))
    assert json.dumps(draw_ops(profile, seed)) == first
    assert json.loads(first) == ops_of(profile, seed)
    assert json.dumps(json.loads(first)) == first
    assert json.dumps(draw_ops(profile, seed + 1)) != first
    assert ops_of(profile, seed)[0]["op"] == "reset"


def test_truncation_and_seed_shift(monkeypatch):
    seed = committed_seeds("maps")[0]
    full = ops_of("maps", seed)
    monkeypatch.setenv("PGX_STATEFUL_OPS", "7")
    assert draw_ops("maps", seed) == full[:7]
    monkeypatch.delenv("PGX_STATEFUL_OPS")
    monkeypatch.setenv("PGX_STATEFUL_SEED", "40")
    assert committed_seeds("maps") == [S.BASE_SEED + 40 + k for k in range(S.SEEDS_PER_PROFILE)]


def test_failure_message_names_everything():
    cfg = profile_config("maps", committed_seeds("maps")[0])
    ops = copy.deepcopy(ops_of("maps", committed_seeds("maps")[0]))
    with pytest.raises(StatefulMismatch) as ei:
        run(StandIn(cfg, 4), Model(cfg), ops, label="maps seed X")
    text = str(ei.value)
    assert "maps seed X" in text and f"op {ei.value.index}" in text and "first at" in text
    replay = json.loads(text.split("replay (the operations so far):\n", 1)[1])
    assert replay == ops[:ei.value.index + 1]
