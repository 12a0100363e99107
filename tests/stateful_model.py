"""Stateful fuzz: a host model of everything a VecPogema carries from one call to the next, a generator of random but
legal operation sequences, and the driver that applies a sequence to an engine and to the model and compares the two
after every operation.  Pure numpy + the Python oracle; torch is imported only inside run() / make_engine().

The model follows docs/SPEC.md: S1..S8 through oracle.pogema_oracle.PogemaOracle (one per env), S6 / S10 through
oracle.generator_oracle, S11's cache contract as bookkeeping (a tag per field, the map the fields of an env were built
on, a build counter), S19 for copy_envs.  Every query is checked against its tests/*_reference.py function evaluated
on the model's state.

What a snapshot carries (read off snapshot_segments() in pogema_amd/csrc/pgx_api.cpp and VecPogema.save_state):
the complete per-env state S19 lists as copied, AND the generation counters (`epoch`, which copy_envs leaves with
the slot), `map_index` where a pool is installed, and the seed of the last reset(seed) (`reset_seed`, kept by the Python
layer).  It carries nothing of the distance-field cache, of the output sets or of their held-zeros records: after
load_state the cache is revalidated from the state (S11), and the buffers are as the caller left them.  S19 itself names
only the copied segments; that save_state() takes the slot's `epoch` too is the one divergence from its list.

Profiles (PROFILES): the shapes of the issue, with one change -- GridConfig draws random maps as squares only
(GridConfig.size), so `maps` runs 10x10 random maps instead of 9x11; rectangular maps are reached by `wide` (20x34).

Replay: PGX_STATEFUL_SEED shifts the seeds of the committed cases, PGX_STATEFUL_OPS=N cuts a sequence to its first N
operations.  A failure names the profile, the seed, the operation's index, the operation, the first differing element and
the JSON of the operations so far.
"""
from __future__ import annotations

import contextlib
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import generator_oracle as G  # noqa: E402
from oracle.pogema_oracle import PogemaOracle, splitmix64  # noqa: E402

import agent_forecasts_reference as forecasts_ref  # noqa: E402
import goal_directions_reference as directions_ref  # noqa: E402
import goal_paths_reference as paths_ref  # noqa: E402
from agent_counts import shared_fields  # noqa: E402
from agent_tokens_reference import agent_tokens_reference, token_length  # noqa: E402
from cost_to_go_reference import cost_to_go_reference  # noqa: E402
from expert_reference import expert_reference  # noqa: E402
from global_state_reference import CHANNELS as GLOBAL_CHANNELS, global_state_reference  # noqa: E402
from move_outcomes_reference import move_outcomes_reference  # noqa: E402
from pibt_plan_reference import pibt_plan_reference  # noqa: E402
from pibt_reference import pibt_reference  # noqa: E402
from pibt_swap_reference import pibt_swap_reference  # noqa: E402
from policy_input_reference import other_goals_reference  # noqa: E402
from shield_inputs import random_scores, special_scores  # noqa: E402
from shield_reference import shield_reference  # noqa: E402
from visible_agents_reference import visible_agents_reference  # noqa: E402

TAG_POOL = 0x504F4F4C00000000  # 'POOL' (docs/SPEC.md S10)
METRIC_NAMES = ("ISR", "CSR", "ep_length", "SoC", "makespan", "avg_throughput")
OBS_CHANNELS = ("obstacles", "agents", "target")
DIR_CHANNELS = ("up", "down", "left", "right")
POLICY_CHANNELS = OBS_CHANNELS + ("other_goals",) + DIR_CHANNELS
ACTION_DTYPES = ("int8", "int32", "int64")
VALUE_DTYPES = ("float32", "float16", "bfloat16", "uint8")

MUTATORS = ("step", "rollout", "set_targets", "reset_where", "reset", "copy_envs", "save_state", "load_state", "observe",
            "touch", "drop")
# the queries that refresh the distance-field cache before they read it (S11) ...
CACHE_QUERIES = ("cost_to_go", "pibt_actions", "pibt_plan", "shield_distance", "goal_directions", "goal_paths",
                 "agent_forecasts", "policy_input_dirs", "agent_tokens")
# ... and those that never touch it
PLAIN_QUERIES = ("expert_actions", "visible_agents", "shield_plain", "move_outcomes", "policy_input_plain", "global_state")
QUERIES = CACHE_QUERIES + PLAIN_QUERIES
HOLD_LIMIT = 3      # the caller keeps the outputs of at most this many earlier calls referenced
P_EXPERT = 0.75     # share of the model's expert moves among a step's actions


class StatefulMismatch(AssertionError):
    """Engine and model disagree.  `index` / `op`: where in the sequence; `what`: which comparison."""

    def __init__(self, what, index, op, label, ops_so_far):
        self.what, self.index, self.op, self.label = what, index, op, label
        super().__init__(f"{label}: op {index} {json.dumps(op)[:400]}: {what}\nreplay (the operations so far):\n"
                         f"{json.dumps(ops_so_far)}")


# ---- profiles -----------------------------------------------------------------------------------------------------------
PROFILES = ("maps", "pool", "lifelong", "wide")
SEEDS_PER_PROFILE = 4
BASE_SEED = 1000
PAIRS_PER_SEQUENCE = 38


def committed_seeds(profile):
    """The seeds of the committed cases of `profile`, shifted by PGX_STATEFUL_SEED."""
    shift = int(os.environ.get("PGX_STATEFUL_SEED", "0"))
    return [BASE_SEED + shift + k for k in range(SEEDS_PER_PROFILE)]


def _random_map(rng, H, W, density):
    return (rng.random((H, W)) < density).astype(np.uint8)


def profile_config(profile, seed):
    """Everything that defines the engine of (profile, seed) as plain data.  The collision system and the Semantics
    switches are drawn per seed."""
    rng = np.random.default_rng([PROFILES.index(profile), seed, 1])
    cfg = dict(profile=profile, seed=int(seed), collision=str(rng.choice(["priority", "block_both", "soft"])),
               semantics=dict(soft_vertex_rule=str(rng.choice(["lowest_index", "all_stay"])),
                              soft_occupancy=str(rng.choice(["index_order", "exact"])),
                              coop_reward=str(rng.choice(["all_solved", "per_agent"])), bad_action="noop",
                              lifelong_rng="build"),
               gc_seed=int(rng.integers(0, 1000)), base=int(rng.integers(0, 40)), reset_seed=int(rng.integers(0, 10 ** 6)),
               pool=None, shared_map=None, empty_outside=True, held=False)
    if profile == "maps":
        cfg.update(B=6, A=4, H=10, W=10, r=2, density=0.3, on_target="finish", max_steps=8, auto_reset="regenerate",
                   empty_outside=bool(rng.integers(0, 2)))
    elif profile == "pool":
        pool = np.stack([_random_map(rng, 12, 12, d) for d in (0.15, 0.25, 0.3)])
        cfg.update(B=5, A=6, H=12, W=12, r=3, density=0.3, on_target="restart", max_steps=11, auto_reset="regenerate",
                   pool=pool.tolist())
    elif profile == "lifelong":
        cfg.update(B=4, A=5, H=10, W=10, r=2, density=0.0, on_target="restart", max_steps=9, auto_reset=True, held=True,
                   shared_map=_random_map(rng, 10, 10, 0.2).tolist())
        if seed % SEEDS_PER_PROFILE == SEEDS_PER_PROFILE - 1:   # one case in four: the numpy stream (S5), generators copied
            cfg["semantics"]["lifelong_rng"] = "numpy"
    elif profile == "wide":
        cfg.update(B=3, A=70, H=20, W=34, r=5, density=0.0, on_target="finish", max_steps=12, auto_reset=True, held=True,
                   shared_map=_random_map(rng, 20, 34, 0.1).tolist())
    else:
        raise ValueError(f"unknown profile {profile!r}")
    if cfg["shared_map"] is not None:  # GridConfig: with an explicit map, `density` is its obstacle fraction
        m = np.asarray(cfg["shared_map"])
        cfg["density"] = float(sum(1 for v in m.reshape(-1) if v != 0) / m.size)
    return cfg


def make_engine(cfg, **extra):
    """The VecPogema of a profile_config(): no zone walk, the held path on wherever the configuration has a held kernel."""
    from pogema_amd import GridConfig, VecPogema
    from pogema_amd.semantics import Semantics
    s = cfg["semantics"]
    sem = Semantics(soft_vertex=s["soft_vertex_rule"], soft_occupancy=s["soft_occupancy"], coop_reward=s["coop_reward"],
                    bad_action=s["bad_action"], lifelong_rng=s["lifelong_rng"])
    kw = dict(num_agents=cfg["A"], obs_radius=cfg["r"], collision_system=cfg["collision"], on_target=cfg["on_target"],
              max_episode_steps=cfg["max_steps"], seed=cfg["gc_seed"], empty_outside=cfg["empty_outside"])
    if cfg["shared_map"] is not None:
        kw["map"] = cfg["shared_map"]
    elif cfg["pool"] is None:
        kw.update(size=cfg["H"], density=cfg["density"])
    else:
        kw["density"] = cfg["density"]
    pool = None if cfg["pool"] is None else np.asarray(cfg["pool"], dtype=np.uint8)
    return VecPogema(GridConfig(**kw), batch=cfg["B"], env_index_base=cfg["base"], auto_reset=cfg["auto_reset"],
                     semantics=sem, placement_budget_gib=0, map_pool=pool, held_zeros=True if cfg["held"] else None, **extra)


def pool_pick(seed, env, epoch, M):
    return ((splitmix64(G.instance_hash(seed, env, epoch, 0) ^ TAG_POOL) >> 32) * M) >> 32


# ---- the model ----------------------------------------------------------------------------------------------------------
class Model:
    """The host model: one PogemaOracle per env plus what belongs to the slot (generation, pool index) and the S11
    bookkeeping of the distance-field cache."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.B, self.A, self.H, self.W, self.r = cfg["B"], cfg["A"], cfg["H"], cfg["W"], cfg["r"]
        self.regenerate = cfg["auto_reset"] == "regenerate"
        self.pool = None if cfg["pool"] is None else np.asarray(cfg["pool"], dtype=np.uint8)
        self.shared = None if cfg["shared_map"] is None else np.asarray(cfg["shared_map"], dtype=np.uint8)
        self.env = [None] * self.B
        self.epoch = [0] * self.B
        self.map_index = [-1] * self.B
        self.reset_seed = None
        self.cache_allocated = False
        self.tag = [[None] * self.A for _ in range(self.B)]   # the target cell each field was built for
        self.built_map = [None] * self.B                       # the map (bytes) the env's fields were built on
        self.builds = 0
        self.snapshots = []
        self.events = []          # ("regen", env) / ("copy",) / ("save", k) / ("load", k) / ("end", env), in order
        self.redraws = 0          # lifelong targets drawn inside step()

    # -- instances ---------------------------------------------------------------------------------------------------
    def _instance(self, b, epoch, retries):
        e, seed = self.cfg["base"] + b, self.reset_seed
        if self.pool is not None:
            k = pool_pick(seed, e, epoch, len(self.pool))
            return (k,) + G.generate_instance(seed, e, self.H, self.W, self.A, 0.0, epoch=epoch, max_retries=retries,
                                              given_map=self.pool[k])
        return (-1,) + G.generate_instance(seed, e, self.H, self.W, self.A, self.cfg["density"], epoch=epoch,
                                           max_retries=retries, given_map=self.shared)

    def _oracle(self, b, obstacles, agents, targets, epoch):
        c = self.cfg
        return PogemaOracle(obstacles, agents, targets, obs_radius=self.r, collision_system=c["collision"],
                            on_target=c["on_target"], max_episode_steps=c["max_steps"], auto_reset=c["auto_reset"] is True,
                            seed=c["gc_seed"], env_index=c["base"] + b, empty_outside=c["empty_outside"],
                            outside_density=c["density"], epoch=epoch, **c["semantics"])

    def _install(self, b, epoch, retries):
        k, o, a, t = self._instance(b, epoch, retries)
        self.env[b] = self._oracle(b, o, a, t, epoch)
        self.epoch[b] = epoch
        self.map_index[b] = k

    # -- mutators ----------------------------------------------------------------------------------------------------
    def reset(self, seed):
        self.reset_seed = int(seed)
        for b in range(self.B):
            self._install(b, 0, 10)
        return self.observe()

    def reset_where(self, mask):
        for b in range(self.B):
            if mask[b]:
                self._advance(b)
                self.events.append(("regen", b))
                self._install(b, self.epoch[b], 10)
        return self.observe()

    def _advance(self, b):
        self.epoch[b] += 1

    def observe(self):
        return np.stack([np.stack(e._obs()) for e in self.env]).astype(np.float32)

    def step(self, actions):
        """One step of every env (S1..S8).  Returns the dict of step()'s outputs as host arrays; `metrics` rows are zero
        where `episode_done` is not set."""
        B, A = self.B, self.A
        out = {"rewards": np.zeros((B, A), np.float32), "terminated": np.zeros((B, A), bool),
               "truncated": np.zeros((B, A), bool), "is_active": np.zeros((B, A), bool),
               "episode_done": np.zeros(B, bool), "metrics": np.zeros((B, 6), np.float32)}
        obs = []
        for b, e in enumerate(self.env):
            o, rew, term, trunc, infos = e.step(actions[b])
            out["rewards"][b], out["terminated"][b], out["truncated"][b] = rew, term, trunc
            out["is_active"][b] = [i["is_active"] for i in infos]
            if self.cfg["on_target"] == "restart":
                self.redraws += int(sum(rew))
            if "metrics" in infos[0]:
                out["episode_done"][b] = True
                out["metrics"][b] = [infos[0]["metrics"][k] for k in METRIC_NAMES]
                self.events.append(("end", b))
                if self.regenerate:
                    o = self._regenerate(b)
            obs.append(np.stack(o))
        out["obs"] = np.stack(obs).astype(np.float32)
        return out

    def _regenerate(self, b):
        """auto_reset='regenerate': the slot's generation advances and the env continues on the instance of that
        generation; when none can be placed in 3 attempts it returns to its stored initial state (S10, Failure)."""
        self.epoch[b] += 1
        self.events.append(("regen", b))
        try:
            self._install(b, self.epoch[b], 3)
        except OverflowError:
            self.env[b].reset()
        return self.env[b]._obs()

    def rollout(self, actions):
        """K steps: exactly K model steps (S8); the per-step outputs stacked."""
        outs = [self.step(a) for a in actions]
        return {k: np.stack([o[k] for o in outs]) for k in outs[0]}

    def set_targets(self, targets, mask=None):
        for b, e in enumerate(self.env):
            e.set_targets(targets[b], None if mask is None else mask[b])

    def copy_envs(self, src, dst, cache=True):
        """S19: the slot keeps its global env index and its generation; cache rows travel with cache=True once the
        cache is allocated."""
        src = [src] * len(dst) if isinstance(src, int) else list(src)
        self.events.append(("copy",))
        for s, d in zip(src, dst):
            if s == d:
                continue
            self._copy_one(s, d)
            if cache and self.cache_allocated:
                self._copy_cache_row(s, d)

    def _copy_one(self, s, d):
        e = copy.deepcopy(self.env[s])
        e.env_index = self.cfg["base"] + d
        e._outside = (e.seed, e.env_index, self.epoch[d], e._outside[3])
        self.env[d] = e
        self.map_index[d] = self.map_index[s]

    def _copy_cache_row(self, s, d):
        self.tag[d] = list(self.tag[s])
        self.built_map[d] = self.built_map[s]

    def save_state(self):
        self.snapshots.append(copy.deepcopy((self.env, self.epoch, self.map_index, self.reset_seed)))
        self.events.append(("save", len(self.snapshots) - 1))
        return len(self.snapshots) - 1

    def load_state(self, k):
        self.events.append(("load", k))
        self._restore(copy.deepcopy(self.snapshots[k]))

    def _restore(self, snap):
        self.env, self.epoch, self.map_index, self.reset_seed = snap

    # -- state -------------------------------------------------------------------------------------------------------
    def maps(self):
        return np.stack([np.asarray(e._init_args[0], dtype=np.uint8) for e in self.env])

    def state(self):
        sts = [e.get_state() for e in self.env]
        st = {k: np.stack([s[k] for s in sts]) for k in ("agents_xy", "targets_xy", "is_active", "occupancy")}
        st["is_active"] = st["is_active"].astype(bool)
        st["elapsed"] = np.array([s["elapsed"] for s in sts], dtype=np.int32)
        return st

    def active_byte(self, st):
        """The engine's `active` byte: 0 hidden, 1 active, 3 active but missing from the occupancy array (a `soft` ghost)."""
        xy = st["agents_xy"].astype(np.int64) + self.r
        on_cell = st["occupancy"][np.arange(self.B)[:, None], xy[..., 0], xy[..., 1]] != 0
        return np.where(st["is_active"], np.where(on_cell, 1, 3), 0)

    def expert_moves(self):
        """The shortest-path expert's action for every agent (tests/expert_reference.py; with many agents the lowest
        direction plane at the window centre, which S14 defines as the same action)."""
        st, maps = self.state(), self.maps()
        if self.A <= 16:
            return expert_reference(maps, st["agents_xy"], st["targets_xy"], st["is_active"])[0]
        bits = directions_ref.goal_directions_reference(maps, st["agents_xy"], st["targets_xy"], st["is_active"], self.r)
        centre = bits[:, :, self.r, self.r].astype(np.int64)
        low = np.zeros_like(centre)
        for a in (4, 3, 2, 1):
            low = np.where((centre >> (a - 1)) & 1, a, low)
        return low

    # -- S11: the cache contract -----------------------------------------------------------------------------------
    def refresh(self):
        """What a cache-reading query does first: returns the number of fields it must build."""
        self.cache_allocated = True
        st, maps = self.state(), self.maps()
        built = 0
        for b in range(self.B):
            key = maps[b].tobytes()
            if self.built_map[b] != key:           # a map change invalidates every agent of the env
                self.built_map[b] = key
                self.tag[b] = [None] * self.A
            for i in range(self.A):
                if self._counts(st, b, i):
                    t = (int(st["targets_xy"][b, i, 0]), int(st["targets_xy"][b, i, 1]))
                    if self.tag[b][i] != t:
                        self.tag[b][i] = t
                        built += 1
        self.builds += built
        return built

    def _counts(self, st, b, i):
        return bool(st["is_active"][b, i])

    # -- queries -----------------------------------------------------------------------------------------------------
    def query(self, op):
        """The reference result of query `op` on the current state, as a tuple of host arrays in the order the engine
        returns them (None where the engine returns None), and the number of fields the call must build."""
        st, maps = self.state(), self.maps()
        built = self.refresh() if reads_cache(op) else 0
        # (many agents: the planners' references take their one field per target and call from a shared, vectorised memo)
        with shared_fields(maps, st["targets_xy"]) if self.A > 16 else contextlib.nullcontext():
            return self._evaluate(op, st, maps), built

    def _evaluate(self, op, st, maps):
        pos, tgt, act, r, B, A = st["agents_xy"], st["targets_xy"], st["is_active"], self.r, self.B, self.A
        name = op["op"]
        if name == "expert_actions":
            res = expert_reference(maps, pos, tgt, act, op["agents_as_obstacles"])
        elif name == "cost_to_go":
            res = (cost_to_go_reference(maps, pos, tgt, act, r),)
        elif name == "visible_agents":
            res = visible_agents_reference(pos, act, r, op["k"])
        elif name == "pibt_actions":
            ref = pibt_swap_reference if op["swap"] else pibt_reference
            res = ref(maps, pos, tgt, act, priorities(op["priority"], B, A))[:2]
        elif name == "pibt_plan":
            res = pibt_plan_reference(maps, pos, tgt, act, op["horizon"], priorities(op["priority"], B, A),
                                      on_target=self.cfg["on_target"], growing=op["growing"])[:4]
        elif name == "shield_actions":
            res = shield_reference(maps, pos, tgt, act, scores(op, B, A), priorities(op["priority"], B, A),
                                   op["tie_break"])[:3]
        elif name == "goal_directions":
            bits = directions_ref.goal_directions_reference(maps, pos, tgt, act, r)
            res = (bits if op["format"] == "bits" else directions_ref.planes(bits),)
        elif name == "goal_paths":
            planes, subgoal, length = paths_ref.goal_paths_reference(maps, pos, tgt, act, r, op["steps"])
            planes = paths_ref.rows(planes) if op["format"] == "rows" else planes
            res = (planes if op["planes"] else None, subgoal, length)
        elif name == "agent_forecasts":
            planes, cells = forecasts_ref.agent_forecasts_reference(maps, pos, tgt, act, r, op["steps"])
            planes = forecasts_ref.rows(planes) if op["format"] == "rows" else planes
            res = (planes if op["planes"] else None, cells)
        elif name == "move_outcomes":
            res = move_outcomes_reference(maps, pos, act, np.asarray(op["actions"]), self.cfg["collision"],
                                          self.cfg["semantics"]["soft_vertex_rule"])
        elif name == "policy_input":
            obs = self.observe()
            planes = {n: obs[:, :, c] for c, n in enumerate(OBS_CHANNELS)}
            if "other_goals" in op["channels"]:
                planes["other_goals"] = other_goals_reference(pos, tgt, act, r)
            if any(c in DIR_CHANNELS for c in op["channels"]):
                d = directions_ref.planes(directions_ref.goal_directions_reference(maps, pos, tgt, act, r))
                planes.update({n: d[:, :, c] for c, n in enumerate(DIR_CHANNELS)})
            res = (np.stack([np.asarray(planes[c]).astype(np.float32) for c in op["channels"]], axis=2),)
        elif name == "global_state":
            ref = global_state_reference(maps, pos, tgt, self.active_byte(st))
            res = (ref[:, [GLOBAL_CHANNELS.index(c) for c in op["channels"]]],)
        elif name == "agent_tokens":
            res = (agent_tokens_reference(maps, pos, tgt, act, r, slots=op["slots"], history=history(op, B, A),
                                          length=op["length"]),)
        else:
            raise ValueError(f"unknown query {name!r}")
        return tuple(res)


def reads_cache(op):
    name = op["op"]
    if name == "shield_actions":
        return op["tie_break"] == "distance"
    if name == "policy_input":
        return any(c in DIR_CHANNELS for c in op["channels"])
    return name in CACHE_QUERIES


def query_kind(op):
    """The name of `op` in QUERIES / MUTATORS (shield_actions and policy_input come in a cache-reading and a plain form)."""
    name = op["op"]
    if name == "shield_actions":
        return "shield_distance" if reads_cache(op) else "shield_plain"
    if name == "policy_input":
        return "policy_input_dirs" if reads_cache(op) else "policy_input_plain"
    return name


def priorities(seed, B, A):
    """The priorities of a planner call: None, int32 [B, A] drawn from `seed`, or the array itself."""
    if isinstance(seed, np.ndarray):
        return seed.astype(np.int32)
    return None if seed is None else np.random.default_rng(seed).integers(-3, 4, size=(B, A)).astype(np.int32)


def scores(op, B, A):
    """The action scores of a shield_actions op: tests/shield_inputs.py's value sets, drawn from the op's seed."""
    if isinstance(op["scores"], np.ndarray):
        return op["scores"]
    make = special_scores if op["scores"] == "special" else random_scores
    return make(np.random.default_rng(op["scores_seed"]), B, A)


def history(op, B, A):
    if op["history"] is None or isinstance(op["history"], np.ndarray):
        return op["history"]
    return np.random.default_rng(op["history"]).integers(-1, 6, size=(B, A, 5)).astype(np.int8)


# ---- the generator ------------------------------------------------------------------------------------------------------
def admitted_mutators(cfg):
    """rollout() is refused under auto_reset='regenerate'; everything else is admitted by every profile."""
    return tuple(m for m in MUTATORS if not (m == "rollout" and cfg["auto_reset"] == "regenerate"))


def _schedule(cfg, seed, rng, pairs):
    """The (mutator, query) pairs of one sequence.  Every (mutator, cache-reading query) pair belongs to exactly one of
    SEEDS_PER_PROFILE chunks, and a sequence takes chunk `seed % SEEDS_PER_PROFILE`: consecutive seeds cover the whole
    cross product whatever PGX_STATEFUL_SEED is.  The rest are plain queries behind mostly steps."""
    muts = admitted_mutators(cfg)
    chunk = seed % SEEDS_PER_PROFILE
    out = [(m, q) for mi, m in enumerate(muts) for qi, q in enumerate(CACHE_QUERIES)
           if (mi + qi) % SEEDS_PER_PROFILE == chunk]
    movers = ("step", "step", "step", "rollout") if "rollout" in muts else ("step",)
    for q in PLAIN_QUERIES * 2:
        out.append((str(rng.choice(movers)) if rng.random() < 0.6 else str(rng.choice(muts)), q))
    while len(out) < pairs:
        out.append((str(rng.choice(movers)), str(rng.choice(QUERIES))))
    order = rng.permutation(len(out))
    out = [out[k] for k in order]
    # a snapshot must exist before the first load_state: the first save_state pair goes in front of it
    names = [m for m, _ in out]
    if "load_state" in names:
        first_load = names.index("load_state")
        if "save_state" in names:
            first_save = names.index("save_state")
            if first_save > first_load:
                out[first_load], out[first_save] = out[first_save], out[first_load]
        else:
            out.insert(first_load, ("save_state", str(rng.choice(QUERIES))))
    return out


class _Drawer:
    """Draws the arguments of the operations; consults the model only for legality and for the expert's moves."""

    def __init__(self, cfg, seed, rng):
        self.cfg, self.rng, self.model = cfg, rng, Model(cfg)
        self.B, self.A = cfg["B"], cfg["A"]
        self.ops = []
        self.held_obs = []   # one entry per set of outputs the caller keeps: does it hold an observation?

    def emit(self, op):
        self.ops.append(op)
        apply_to_model(self.model, op)

    def _actions(self):
        rng = self.rng
        expert = self.model.expert_moves()
        rnd = rng.integers(0, 5, size=(self.B, self.A))
        return np.where(rng.random((self.B, self.A)) < P_EXPERT, expert, rnd).astype(np.int64)

    def _keep(self, has_obs, force=False):
        keep = force or bool(self.rng.random() < 0.35)
        if keep:
            self.held_obs = (self.held_obs + [has_obs])[-HOLD_LIMIT:]
        return keep

    def step(self, plain=False):
        rng = self.rng
        op = {"op": "step", "actions": self._actions().tolist(), "dtype": str(rng.choice(ACTION_DTYPES)),
              "compute_obs": bool(plain or rng.random() < 0.8), "out": bool(not plain and rng.random() < 0.2)}
        op["keep"] = self._keep(op["compute_obs"], force=plain)
        self.emit(op)

    def mutator(self, name):
        rng, B, A, m = self.rng, self.B, self.A, self.model
        if name == "step":
            return self.step()
        if name == "rollout":
            K = int(rng.integers(1, 6))
            probe, acts = copy.deepcopy(m), []
            saved, self.model = self.model, probe     # the K action sets follow the model through the K steps
            for _ in range(K):
                acts.append(self._actions())
                probe.step(acts[-1])
            self.model = saved
            return self.emit({"op": "rollout", "actions": np.stack(acts).tolist(), "dtype": str(rng.choice(ACTION_DTYPES))})
        if name == "set_targets":
            mask = (rng.random((B, A)) < 0.5).tolist() if rng.random() < 0.5 else None
            return self.emit({"op": "set_targets", "targets": self._targets(favourite=rng.random() < 0.3), "mask": mask})
        if name == "reset_where":
            return self.emit({"op": "reset_where", "mask": (rng.random(B) < 0.4).tolist()})
        if name == "reset":
            return self.emit({"op": "reset", "seed": int(rng.integers(0, 10 ** 6))})
        if name == "copy_envs":
            return self.emit(self._copy())
        if name == "save_state":
            return self.emit({"op": "save_state"})
        if name == "load_state":
            k = int(rng.integers(0, len(m.snapshots)))
            if rng.random() < 0.6:
                # the same target cells before and after a load that may change maps: fields built on the other map must go
                self.emit({"op": "set_targets", "targets": self._targets(favourite=True), "mask": None})
                self.emit({"op": "cost_to_go"})
                self.emit({"op": "load_state", "snapshot": k})
                self.emit({"op": "set_targets", "targets": self._targets(favourite=True), "mask": None})
                self.emit({"op": "cost_to_go"})
                k = int(rng.integers(0, len(m.snapshots)))
            return self.emit({"op": "load_state", "snapshot": k})
        if name == "observe":
            op = {"op": "observe", "out": bool(rng.random() < 0.3)}
            op["keep"] = self._keep(True)
            return self.emit(op)
        if name == "touch":
            if not any(self.held_obs):
                self.step(plain=True)   # something to write into: a kept step with an observation
            which = [k for k, has in enumerate(self.held_obs) if has]
            return self.emit({"op": "touch", "which": int(rng.choice(which)), "how": str(rng.choice(["mul_", "zero_"]))})
        if name == "drop":
            self.held_obs = []
            return self.emit({"op": "drop"})
        raise ValueError(name)

    def _targets(self, favourite):
        """Free cells of each env's current map: random ones, or (favourite) for agent i the first free cell of a fixed
        list read from entry i on -- the same cell again whenever the map allows it."""
        rng, B, A, H, W = self.rng, self.B, self.A, self.cfg["H"], self.cfg["W"]
        maps = self.model.maps()
        fixed = [(1, 1), (H - 2, W - 2), (1, W - 2), (H - 2, 1), (H // 2, W // 2), (2, W // 2), (H // 2, 2), (0, 0)]
        targets = np.zeros((B, A, 2), dtype=np.int64)
        for b in range(B):
            free = np.argwhere(maps[b] == 0)
            targets[b] = free[rng.integers(0, len(free), size=A)]
            if favourite:
                for i in range(A):
                    for k in range(3):
                        c = fixed[(i + k) % len(fixed)]
                        if maps[b][c] == 0:
                            targets[b, i] = c
                            break
        return targets.tolist()

    def _copy(self):
        """copy_envs in one of its accepted forms: no destination twice, no destination that is also a source."""
        rng, B = self.rng, self.B
        form = str(rng.choice(["broadcast", "fanout", "self_pair", "empty", "pairs"]))
        envs = [int(v) for v in rng.permutation(B)]
        if form == "empty":
            src, dst = [], []
        elif form == "broadcast":
            src, dst = envs[0], envs[1:1 + int(rng.integers(1, B))]
        elif form == "fanout":
            dst = envs[1:1 + int(rng.integers(2, B))]
            src = [envs[0]] * len(dst)
        else:
            n = int(rng.integers(1, (B - 1 if form == "self_pair" else B) // 2 + 1))
            src, dst = envs[:n], envs[n:2 * n]
            if form == "self_pair":   # a src == dst pair among the others, of an env no other pair names
                k = int(rng.integers(0, n + 1))
                src, dst = src[:k] + [envs[-1]] + src[k:], dst[:k] + [envs[-1]] + dst[k:]
        return {"op": "copy_envs", "src": src, "dst": dst, "cache": bool(rng.random() < 0.6)}

    def query(self, kind):
        rng, B, A, r = self.rng, self.B, self.A, self.cfg["r"]
        seed = lambda: int(rng.integers(0, 2 ** 31))                       # noqa: E731
        prio = lambda: seed() if rng.random() < 0.6 else None              # noqa: E731
        fmt = lambda third: str(rng.choice(["float32", "uint8", third]))  # noqa: E731
        if kind == "expert_actions":
            op = {"agents_as_obstacles": bool(rng.integers(0, 2)), "dtype": str(rng.choice(ACTION_DTYPES))}
        elif kind == "cost_to_go":
            op = {}
        elif kind == "visible_agents":
            op = {"k": int(rng.integers(1, 33))}
        elif kind == "pibt_actions":
            op = {"priority": prio(), "swap": bool(rng.integers(0, 2)), "dtype": str(rng.choice(ACTION_DTYPES))}
        elif kind == "pibt_plan":
            op = {"horizon": int(rng.integers(1, 7)), "priority": prio(), "growing": bool(rng.integers(0, 2)),
                  "dtype": str(rng.choice(ACTION_DTYPES))}
        elif kind in ("shield_distance", "shield_plain"):
            op = {"op": "shield_actions", "scores": str(rng.choice(["random", "special"])), "scores_seed": seed(),
                  "priority": prio(), "tie_break": "distance" if kind == "shield_distance" else None}
        elif kind == "goal_directions":
            op = {"format": fmt("bits")}
        elif kind == "goal_paths":
            op = {"steps": None if rng.random() < 0.4 else int(rng.integers(1, 13)), "format": fmt("rows"),
                  "planes": bool(rng.random() < 0.75)}
        elif kind == "agent_forecasts":
            op = {"steps": int(rng.integers(1, 9)), "format": fmt("rows"), "planes": bool(rng.random() < 0.75)}
        elif kind == "move_outcomes":
            op = {"actions": rng.integers(0, 5, size=(B, A)).tolist(), "dtype": str(rng.choice(ACTION_DTYPES))}
        elif kind in ("policy_input_dirs", "policy_input_plain"):
            names = POLICY_CHANNELS if kind == "policy_input_dirs" else OBS_CHANNELS + ("other_goals",)
            n = int(rng.integers(1, len(names) + 1))
            ch = [str(c) for c in rng.permutation(names)[:n]]
            if kind == "policy_input_dirs" and not any(c in DIR_CHANNELS for c in ch):
                ch[int(rng.integers(0, n))] = str(rng.choice(DIR_CHANNELS))
            op = {"op": "policy_input", "channels": ch, "dtype": str(rng.choice(VALUE_DTYPES))}
        elif kind == "global_state":
            n = int(rng.integers(1, len(GLOBAL_CHANNELS) + 1))
            op = {"channels": [str(c) for c in rng.permutation(GLOBAL_CHANNELS)[:n]], "dtype": str(rng.choice(VALUE_DTYPES))}
        elif kind == "agent_tokens":
            slots = int(rng.integers(1, 33))
            op = {"slots": slots, "history": seed() if rng.random() < 0.5 else None,
                  "length": None if rng.random() < 0.5 else token_length(r, slots) + int(rng.integers(0, 20))}
        else:
            raise ValueError(kind)
        self.emit(dict({"op": kind}, **op))


def draw_ops(profile, seed, n=None):
    """The operation sequence of (profile, seed): a list of plain-data ops (JSON-able), drawn from
    np.random.default_rng(seed).  Op 0 is the reset(seed) that installs the first instances; then `n` (mutator, query)
    pairs (default PAIRS_PER_SEQUENCE), each preceded by up to two steps so that agents arrive, finish, restart and
    episodes end.  PGX_STATEFUL_OPS=N cuts the list to its first N ops."""
    cfg = profile_config(profile, seed)
    rng = np.random.default_rng([PROFILES.index(profile), seed])
    d = _Drawer(cfg, seed, rng)
    d.emit({"op": "reset", "seed": cfg["reset_seed"]})
    for mut, q in _schedule(cfg, seed, rng, PAIRS_PER_SEQUENCE if n is None else n):
        for _ in range(int(rng.integers(0, 3))):
            d.step()
        d.mutator(mut)
        d.query(q)
    cut = os.environ.get("PGX_STATEFUL_OPS")
    return d.ops[:int(cut)] if cut else d.ops


def apply_to_model(model, op):
    """Apply one op to the model alone; returns what the model says the op returns (None for the caller's buffer
    handling, which is no business of the model's)."""
    name = op["op"]
    if name == "reset":
        return model.reset(op["seed"])
    if name == "step":
        return model.step(np.asarray(op["actions"]))
    if name == "rollout":
        return model.rollout(np.asarray(op["actions"]))
    if name == "set_targets":
        return model.set_targets(np.asarray(op["targets"]), op["mask"])
    if name == "reset_where":
        return model.reset_where(op["mask"])
    if name == "copy_envs":
        return model.copy_envs(op["src"], op["dst"], op["cache"])
    if name == "save_state":
        return model.save_state()
    if name == "load_state":
        return model.load_state(op["snapshot"])
    if name == "observe":
        return model.observe()
    if name in ("touch", "drop"):
        return None
    return model.query(op)


# ---- the driver ---------------------------------------------------------------------------------------------------------
class RecyclerModel:
    """What the caller can know of the recycled output sets (README, "Output buffers: held zeros"; buffers.py): `n` sets
    handed out in turn, a set only when nothing references it; a held step refreshes -- rewrites everything -- exactly
    when the set is new to it (never written by a held step, or handed out the plain way since) or torch saw a write."""

    def __init__(self, n):
        self.n, self.next = n, 0
        self.vouched = [False] * n
        self.steps = self.refreshes = 0

    def take(self, busy):
        for k in range(self.n):
            i = (self.next + k) % self.n
            if i not in busy:
                self.next = (i + 1) % self.n
                return i
        return None

    def plain(self, busy, with_obs=True):
        i = self.take(busy)
        if i is not None and with_obs:
            self.vouched[i] = False
        return i

    def held_step(self, busy, with_obs):
        i = self.take(busy)
        if i is not None and with_obs:
            self.steps += 1
            self.refreshes += 0 if self.vouched[i] else 1
            self.vouched[i] = True
        return i

    def wrote(self, i):
        if i is not None:
            self.vouched[i] = False


def _first_diff(want, got):
    want, got = np.asarray(want), np.asarray(got)
    if want.shape != got.shape:
        return f"shape {got.shape}, expected {want.shape}"
    ne = want != got
    if want.dtype.kind == "f":
        ne &= ~(np.isnan(want) & np.isnan(got.astype(want.dtype)))
    bad = np.argwhere(ne)
    if bad.size == 0:
        return None
    at = tuple(int(v) for v in bad[0])
    return f"{len(bad)} elements differ, first at {at}: engine {got[at]}, model {want[at]}"


def run(engine, model, ops, check=True, label="stateful"):
    """Apply `ops` to `engine` (a VecPogema, or anything with its surface) and to `model`, comparing after every op:
    after a mutator get_state(occupancy=True), whatever the op returned, the installed maps and `map_index`; after a
    query its result against the reference on the model's state, bit for bit, and the delta of `cost_to_go_builds`
    against S11's count.  Outputs the caller keeps referenced are re-read after every op, and the held-zeros counters
    follow RecyclerModel.  `check=False` applies the ops without comparing.  Raises StatefulMismatch."""
    import torch
    dev = engine.device
    B, A, r = model.B, model.A, model.r
    tdt = {n: getattr(torch, n) for n in ACTION_DTYPES + VALUE_DTYPES + ("int16", "bool")}
    snapshots = []   # what engine.save_state() returned, in order
    holds = []       # {"tensors": [...], "expect": [...], "set": index or None}
    recycler = [None]
    index = [0, None]

    def fail(what):
        raise StatefulMismatch(what, index[0], index[1], label, ops[:index[0] + 1])

    def host(t):
        t = t.detach()
        if t.dtype in (torch.bfloat16, torch.float16):
            t = t.float()
        return np.array(t.cpu().numpy(), copy=True)

    def same(name, want, got, tol=None):
        if not check:
            return
        got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
        want = np.asarray(want)
        if tol is not None:
            if got.shape != want.shape or not np.allclose(got, want, rtol=tol, atol=tol):
                fail(f"{name}: {_first_diff(want.astype(np.float32), got)} (tolerance {tol})")
            return
        d = _first_diff(want.astype(got.dtype) if want.dtype != got.dtype and want.dtype.kind in "iub" else want, got)
        if d:
            fail(f"{name}: {d}")

    def dev_t(a, dtype):
        return torch.as_tensor(np.asarray(a), device=dev).to(tdt[dtype])

    def busy():
        return {h["set"] for h in holds if h["set"] is not None}

    def sim():
        if recycler[0] is None and getattr(engine, "_recycler", None):
            recycler[0] = RecyclerModel(len(engine._recycler))
        return recycler[0]

    def hold(tensors, expect, set_index, keep):
        if keep:
            holds.append({"tensors": list(tensors), "expect": [None if e is None else np.array(e, copy=True) for e in expect],
                          "set": set_index})
            del holds[:-HOLD_LIMIT]

    def check_state():
        if not check:
            return
        st = engine.get_state(occupancy=True)
        want = model.state()
        for k in ("agents_xy", "targets_xy", "elapsed", "is_active", "occupancy"):
            same(f"get_state()[{k}]", want[k], st[k])
        same("installed maps", model.maps(), installed_maps(engine))
        if model.pool is not None:
            same("map_index", np.asarray(model.map_index, dtype=np.int32), engine.map_index)

    def check_holds():
        """The recycler must not hand out a set the caller still references: what is kept still holds what it held."""
        if not check:
            return
        for k, h in enumerate(holds):
            for name, t, e in zip(("obs", "rewards", "terminated", "truncated", "is_active"), h["tensors"], h["expect"]):
                if t is not None:
                    same(f"kept outputs {k} ({name}) changed behind the caller's back", e, t, tol=1e-6 if name == "rewards" else None)

    def check_held_counters():
        s = recycler[0]
        if check and s is not None and engine.held_zeros["enabled"]:
            info = engine.held_zeros
            if (info["steps"], info["refreshes"]) != (s.steps, s.refreshes):
                fail(f"held_zeros: engine steps {info['steps']} refreshes {info['refreshes']}, the rule gives steps "
                     f"{s.steps} refreshes {s.refreshes}")

    def compare_step(want, got, what):
        obs, rew, term, trunc, infos = got
        if obs is not None:
            same(f"{what} obs", want["obs"], obs)
        same(f"{what} rewards", want["rewards"], rew, tol=1e-6)
        same(f"{what} terminated", want["terminated"], term)
        same(f"{what} truncated", want["truncated"], trunc)
        same(f"{what} is_active", want["is_active"], infos["is_active"])
        same(f"{what} episode_done", want["episode_done"], infos["episode_done"])
        done = want["episode_done"]
        same(f"{what} metrics of finished envs", want["metrics"][done], host(infos["metrics"])[done])

    def do_step(op):
        want = model.step(np.asarray(op["actions"]))
        actions = dev_t(op["actions"], op["dtype"])
        out, set_index, s = None, None, sim()
        if op["out"]:
            out = (torch.empty((B, A, 3, 2 * r + 1, 2 * r + 1), dtype=torch.float32, device=dev) if op["compute_obs"] else None,
                   torch.empty((B, A), dtype=torch.float32, device=dev)) + tuple(
                       torch.empty((B, A), dtype=torch.bool, device=dev) for _ in range(3))
        elif s is not None:
            set_index = (s.held_step if engine.held_zeros["enabled"] else s.plain)(busy(), op["compute_obs"])
        got = engine.step(actions, compute_obs=op["compute_obs"], out=out)
        compare_step(want, got, "step():")
        tensors = (got[0], got[1], got[2], got[3], got[4]["is_active"])
        hold(tensors, (want["obs"] if op["compute_obs"] else None, want["rewards"], want["terminated"], want["truncated"],
                       want["is_active"]), set_index, op["keep"])

    def do_rollout(op):
        want = model.rollout(np.asarray(op["actions"]))
        got = engine.rollout(dev_t(op["actions"], op["dtype"]))
        for k in ("obs", "terminated", "truncated", "is_active", "episode_done"):
            same(f"rollout() {k}", want[k], got[k])
        same("rollout() rewards", want["rewards"], got["rewards"], tol=1e-6)
        done = want["episode_done"]
        same("rollout() metrics of finished envs", want["metrics"][done], host(got["metrics"])[done])

    def do_observe(op):
        want = model.observe()
        out, set_index, s = None, None, sim()
        if op["out"]:
            out = torch.empty((B, A, 3, 2 * r + 1, 2 * r + 1), dtype=torch.float32, device=dev)
        elif s is not None:
            set_index = s.plain(busy())
        got = engine.observe(out=out)
        same("observe()", want, got)
        hold((got, None, None, None, None), (want, None, None, None, None), set_index, op["keep"])

    def do_reset(op):
        want = model.reset(op["seed"]) if op["op"] == "reset" else model.reset_where(op["mask"])
        first = sim() is None
        if not first:
            sim().plain(busy())
        if op["op"] == "reset":
            obs, infos = engine.reset(seed=op["seed"])
            same("reset() is_active", np.ones((B, A), bool), infos["is_active"])
        else:
            obs = engine.reset_where(dev_t(op["mask"], "bool"))
        same(f"{op['op']}() obs", want, obs)
        del obs
        if first and sim() is not None:   # the recycler is built by the first reset's own observe()
            sim().plain(set())

    def do_touch(op):
        with_obs = [h for h in holds if h["tensors"][0] is not None]
        h = with_obs[op["which"] % len(with_obs)]
        if op["how"] == "mul_":
            h["tensors"][0].mul_(2)
            h["expect"][0] = h["expect"][0] * 2
        else:
            h["tensors"][0].zero_()
            h["expect"][0] = np.zeros_like(h["expect"][0])
        if recycler[0] is not None:
            recycler[0].wrote(h["set"])

    def do_query(op):
        before = engine.cost_to_go_builds if check else 0
        want, built = model.query(op)
        name = op["op"]
        p = None if op.get("priority") is None else dev_t(priorities(op["priority"], B, A), "int32")
        if name == "expert_actions":
            got = engine.expert_actions(op["agents_as_obstacles"], dtype=tdt[op["dtype"]])
        elif name == "cost_to_go":
            got = (engine.cost_to_go(),)
        elif name == "visible_agents":
            got = engine.visible_agents(op["k"])
        elif name == "pibt_actions":
            got = engine.pibt_actions(priority=p, dtype=tdt[op["dtype"]], swap=op["swap"])
        elif name == "pibt_plan":
            got = engine.pibt_plan(op["horizon"], priority=p, growing=op["growing"], dtype=tdt[op["dtype"]])
        elif name == "shield_actions":
            got = engine.shield_actions(torch.as_tensor(scores(op, B, A), device=dev), priority=p, tie_break=op["tie_break"])
        elif name == "goal_directions":
            got = (engine.goal_directions(op["format"]),)
        elif name == "goal_paths":
            got = engine.goal_paths(op["steps"], op["format"], op["planes"])
        elif name == "agent_forecasts":
            got = engine.agent_forecasts(op["steps"], op["format"], op["planes"])
        elif name == "move_outcomes":
            got = engine.move_outcomes(dev_t(op["actions"], op["dtype"]))
        elif name == "policy_input":
            got = (engine.policy_input(tuple(op["channels"]), dtype=tdt[op["dtype"]]),)
        elif name == "global_state":
            got = (engine.global_state(tuple(op["channels"]), dtype=tdt[op["dtype"]]),)
        else:
            h = history(op, B, A)
            got = (engine.agent_tokens(op["slots"], None if h is None else torch.as_tensor(h, device=dev), op["length"]),)
        if len(got) != len(want):
            fail(f"{name}() returned {len(got)} results, expected {len(want)}")
        for k, (w, g) in enumerate(zip(want, got)):
            if w is None or g is None:
                if check and not (w is None and g is None):
                    fail(f"{name}() result {k}: engine {'None' if g is None else 'a tensor'}, expected the opposite")
                continue
            g = host(g)
            same(f"{name}() result {k}", np.asarray(w).astype(g.dtype), g)
        if check:
            delta = engine.cost_to_go_builds - before
            if delta != built:
                fail(f"cost_to_go_builds grew by {delta}, S11's contract gives {built}")

    from util import installed_maps as _installed

    def installed_maps(e):
        return e.installed_maps() if hasattr(e, "installed_maps") else _installed(e)

    for k, op in enumerate(ops):
        index[0], index[1] = k, op
        name = op["op"]
        if name == "step":
            do_step(op)
        elif name == "rollout":
            do_rollout(op)
        elif name in ("reset", "reset_where"):
            do_reset(op)
        elif name == "observe":
            do_observe(op)
        elif name == "set_targets":
            model.set_targets(np.asarray(op["targets"]), op["mask"])
            engine.set_targets(np.asarray(op["targets"]), None if op["mask"] is None else np.asarray(op["mask"]))
        elif name == "copy_envs":
            model.copy_envs(op["src"], op["dst"], op["cache"])
            engine.copy_envs(op["src"], op["dst"], cache=op["cache"])
        elif name == "save_state":
            model.save_state()
            snapshots.append(engine.save_state())
        elif name == "load_state":
            model.load_state(op["snapshot"])
            engine.load_state(snapshots[op["snapshot"]])
        elif name == "touch":
            do_touch(op)
        elif name == "drop":
            del holds[:]
        else:
            do_query(op)
        if name in MUTATORS:
            check_state()
        check_holds()
        check_held_counters()
    del holds[:]
