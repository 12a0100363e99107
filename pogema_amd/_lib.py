"""ctypes binding of libpogema_amd.so (the C-ABI declared in include/pogema_amd.h).

There is deliberately NO fallback: if the HIP library is missing or cannot be loaded the import of
the engine raises, and every compute call raises `PgxError` when the device is unusable.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PGX_LIB: diagnostic override (A/B of two builds of the SAME engine on one box); never a fallback
LIB_PATH = os.environ.get("PGX_LIB") or os.path.join(_HERE, "libpogema_amd.so")

PGX_ABI_VERSION = 6

COLLISION_SYSTEMS = {"priority": 0, "block_both": 1, "soft": 2}
ON_TARGET = {"finish": 0, "restart": 1, "nothing": 2}
ACTION_DTYPES = {"int8": 0, "int32": 1, "int64": 2}
SOFT_VERTEX_RULES = {"lowest_index": 0, "all_stay": 1}
SOFT_OCCUPANCY = {"index_order": 0, "exact": 1}
COOP_REWARDS = {"all_solved": 0, "per_agent": 1}
BAD_ACTIONS = {"noop": 0, "flag": 1}
LIFELONG_RNGS = {"build": 0, "numpy": 1}
def _obs_dtypes():
    import torch
    return {torch.float32: 0, torch.uint8: 1, torch.bfloat16: 2, torch.float16: 3}


def obs_elem_bytes(dtype) -> int:
    """Bytes per observation cell for a torch dtype the engine writes (float32 4, bfloat16 / float16 2, uint8 1)."""
    import torch
    return {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2, torch.uint8: 1}[dtype]


class _LazyObsDtypes(dict):
    """torch dtype -> PGX_OBS_* code; built on first use so that importing this module stays cheap."""

    def _fill(self):
        if not dict.__len__(self):
            self.update(_obs_dtypes())

    def __contains__(self, k):
        self._fill()
        return dict.__contains__(self, k)

    def __getitem__(self, k):
        self._fill()
        return dict.__getitem__(self, k)


OBS_DTYPES = _LazyObsDtypes()
METRIC_NAMES = ("ISR", "CSR", "ep_length", "SoC", "makespan", "avg_throughput")
# hard limits of the engine (include/pogema_amd.h: PGX_MAX_*); upstream's GridConfig admits size 2..1024, obs_radius 1..128,
# num_agents >= 1 -- README.md "Limits"
MAX_OBS_RADIUS, MAX_AGENTS, MAX_SIDE = 15, 1024, 1024
MAX_NEIGHBOURS = 32  # PGX_MAX_NEIGHBOURS: entries per agent of pgx_visible_agents
DIRECTIONS_FORMATS = {"float32": 0, "uint8": 1, "bits": 2}  # PGX_DIRECTIONS_*: formats of pgx_goal_directions
PATHS_FORMATS = {"float32": 0, "uint8": 1, "rows": 2}  # PGX_PATHS_*: formats of pgx_goal_paths' planes (docs/SPEC.md S22)
MAX_PATH_STEPS = 960  # PGX_MAX_PATH_STEPS: the largest cap of pgx_goal_paths, 31 * 31 - 1
FORECAST_FORMATS = {"float32": 0, "uint8": 1, "rows": 2}  # PGX_FORECAST_*: formats of pgx_agent_forecasts' planes (docs/SPEC.md S24)
MAX_FORECAST_STEPS = 8  # PGX_MAX_FORECAST_STEPS: the most steps of pgx_agent_forecasts
BLOCKING_BLOCKERS = {"all": 0, "on_target": 1}  # flags of pgx_blocking (PGX_BLOCKING_ON_TARGET; docs/SPEC.md S25)
BLOCKING_ON_TARGET = 1  # PGX_BLOCKING_ON_TARGET
MAX_BLOCKING_INFLATION = 64  # PGX_MAX_BLOCKING_INFLATION: the largest inflation of pgx_blocking
# PGX_CONFLICT_VERTEX / _EDGE / _FOLLOW: the kind bits of pgx_path_conflicts, name -> bit (docs/SPEC.md S26)
CONFLICT_KINDS = {"vertex": 1, "edge": 2, "follow": 4}
CONFLICT_ARRIVED = {None: 0, "stay": 8, "vanish": 16}  # PGX_CONFLICT_STAY / _VANISH; None: the engine's on_target decides
CONFLICT_PATHS_PLAN, CONFLICT_PATHS_CELLS = 0, 1  # PGX_CONFLICT_PATHS_*: int32 [K, B, A, 2] / int16 [B, A, K, 2]
MAX_CONFLICT_STEPS = 256  # PGX_MAX_CONFLICT_STEPS: steps of one pgx_path_conflicts, = MAX_PLAN_HORIZON
SHIELD_TIE_BREAKS = {None: 0, "distance": 1}  # flags of pgx_shield_actions (PGX_SHIELD_TIE_DISTANCE)
MAX_PLAN_HORIZON = 256  # PGX_MAX_PLAN_HORIZON: steps of one pgx_pibt_plan
PLAN_FIXED_PRIORITY = 1  # PGX_PLAN_FIXED_PRIORITY: flag of pgx_pibt_plan
MAX_WHCA_HORIZON = 31  # PGX_MAX_WHCA_HORIZON: the window of one pgx_whca_plan (docs/SPEC.md S28)
SWAP_MAX_WALK = 2048  # PGX_SWAP_MAX_WALK: steps of a corridor walk of pgx_pibt_swap_actions (docs/SPEC.md S23)
# PGX_OUTCOME_*: the codes of pgx_move_outcomes, index = code (docs/SPEC.md S17)
OUTCOMES = ("STAY", "MOVED", "OBSTACLE", "SWAP", "OCCUPIED", "FOLLOW", "CONTESTED")
NUM_OUTCOMES = len(OUTCOMES)  # PGX_NUM_OUTCOMES
# PGX_CHANNEL_*: the planes of pgx_policy_input, name -> code (docs/SPEC.md S18); its dtype table is OBS_DTYPES (PGX_OBS_*)
POLICY_CHANNELS = {"obstacles": 0, "agents": 1, "target": 2, "other_goals": 3, "up": 4, "down": 5, "left": 6, "right": 7}
NUM_CHANNELS = len(POLICY_CHANNELS)  # PGX_NUM_CHANNELS
COPY_NO_CACHE = 1  # PGX_COPY_NO_CACHE: flag of pgx_copy_envs (docs/SPEC.md S19)
DEFAULT_POLICY_CHANNELS = ("obstacles", "agents", "target", "up", "down", "left", "right")
# PGX_GLOBAL_*: the planes of pgx_global_state, name -> code (docs/SPEC.md S20); its dtype table is OBS_DTYPES too
GLOBAL_CHANNELS = {"obstacles": 0, "agents": 1, "targets": 2, "agent_ids": 3, "target_ids": 4}
NUM_GLOBAL_CHANNELS = len(GLOBAL_CHANNELS)  # PGX_NUM_GLOBAL_CHANNELS
DEFAULT_GLOBAL_CHANNELS = ("obstacles", "agents", "targets")
GLOBAL_ID_CHANNELS = ("agent_ids", "target_ids")
# the most agents an id channel holds exactly, by PGX_OBS_* code (PGX_GLOBAL_ID_MAX_U8, PGX_GLOBAL_ID_MAX_BF16); the
# other formats hold every count the engine accepts
GLOBAL_ID_MAX = {1: 255, 2: 256}
# PGX_GLOBAL_BAND_CELLS: a workgroup of pgx_global_state holds GLOBAL_BAND_CELLS // W whole rows of a map at a time
GLOBAL_BAND_CELLS = 8192
# PGX_TOKEN_* / PGX_*_TOKEN_*: the vocabulary and the limits of pgx_agent_tokens (docs/SPEC.md S21)
TOKEN_CLIP = 20            # ids 0 .. 2 * TOKEN_CLIP are the integers -TOKEN_CLIP .. TOKEN_CLIP
TOKEN_BLOCKED = 41
TOKEN_ACTION_NONE = 42
TOKEN_ACTION0 = 43         # .. + 4: a recorded action 0..4
TOKEN_GREEDY0 = 48         # .. + 15: the greedy-move mask
TOKEN_PAD = 64
NUM_TOKENS = 65
TOKEN_HISTORY = 5          # recorded actions per agent
TOKEN_SLOT_LEN = 10        # entries per agent slot
MAX_TOKEN_SLOTS = 32
MAX_TOKEN_LENGTH = 2048
TOKENS = {"CLIP": TOKEN_CLIP, "BLOCKED": TOKEN_BLOCKED, "ACTION_NONE": TOKEN_ACTION_NONE, "ACTION0": TOKEN_ACTION0,
          "GREEDY0": TOKEN_GREEDY0, "PAD": TOKEN_PAD, "NUM_TOKENS": NUM_TOKENS, "HISTORY": TOKEN_HISTORY,
          "SLOT_LEN": TOKEN_SLOT_LEN, "MAX_SLOTS": MAX_TOKEN_SLOTS, "MAX_LENGTH": MAX_TOKEN_LENGTH}


# every symbol include/pogema_amd.h declares; tests/test_abi.py checks the library exports them all
EXPORTED_SYMBOLS = (
    "pgx_abi_version", "pgx_last_error", "pgx_create", "pgx_check_config", "pgx_destroy", "pgx_obs_elems", "pgx_agent_elems",
    "pgx_reset_from_state", "pgx_reset_random", "pgx_regenerate", "pgx_regenerate_failures", "pgx_get_map", "pgx_step", "pgx_step_held", "pgx_held_available", "pgx_observe", "pgx_set_metrics_buffers", "pgx_get_state", "pgx_generate", "pgx_place_agents",
    "pgx_snapshot_bytes", "pgx_save_snapshot", "pgx_load_snapshot", "pgx_time_observe", "pgx_bad_action_count",
    "pgx_buffers_create", "pgx_buffers_ptr", "pgx_buffers_get_info", "pgx_buffers_destroy", "pgx_set_targets",
    "pgx_np_streams", "pgx_np_streams_host", "pgx_np_generate", "pgx_np_generate_host", "pgx_rollout", "pgx_buffers_stride", "pgx_buffers_drop", "pgx_xcd_shares", "pgx_xcd_tune", "pgx_buffers_create_at", "pgx_time_observe_pair", "pgx_buffers_va_reserved", "pgx_get_geometry",
    "pgx_expert_actions", "pgx_set_map_pool", "pgx_reset_pool", "pgx_regenerate_pool", "pgx_get_map_index",
    "pgx_cost_to_go", "pgx_cost_to_go_bytes", "pgx_cost_to_go_builds", "pgx_visible_agents", "pgx_pibt_actions",
    "pgx_goal_directions", "pgx_shield_actions", "pgx_pibt_plan", "pgx_move_outcomes",
    "pgx_policy_input", "pgx_copy_envs", "pgx_global_state", "pgx_global_state_check",
    "pgx_agent_tokens", "pgx_agent_tokens_length", "pgx_goal_paths", "pgx_pibt_swap_actions", "pgx_pibt_swap_plan",
    "pgx_agent_forecasts", "pgx_blocking", "pgx_path_conflicts", "pgx_whca_plan", "pgx_repair_plan",
)


class PgxError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"pogema_amd engine error {code}: {message}")
        self.code = code


class PgxBuffersInfo(C.Structure):
    _fields_ = [("bytes", C.c_int64), ("count", C.c_int32), ("spread", C.c_int32), ("candidates", C.c_int32),
                ("reserved0", C.c_int32), ("same_zone_us", C.c_float), ("final_us", C.c_float), ("spacer_gib", C.c_double),
                ("buffer_gbs", C.c_float), ("reserved1", C.c_float)]


class PgxGeometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("lanes_per_env", "waves", "envs_per_wave", "multi_wave", "p16", "stagger",
                                          "store_policy", "state_stores", "grid", "lds_bytes", "for_rollout", "xcd_aware")]


class PgxRolloutIO(C.Structure):
    _fields_ = [("actions", C.c_void_p), ("obs", C.c_void_p), ("rewards", C.c_void_p), ("terminated", C.c_void_p),
                ("truncated", C.c_void_p), ("is_active", C.c_void_p), ("episode_done", C.c_void_p), ("metrics", C.c_void_p),
                ("action_dtype", C.c_int32), ("obs_slots", C.c_int32), ("obs_slot_stride", C.c_int64),
                ("policy_seed", C.c_uint64), ("policy_step0", C.c_int64), ("actions_out", C.c_void_p)]


class PgxConfig(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("num_agents", C.c_int32),
        ("obs_radius", C.c_int32), ("collision_system", C.c_int32), ("on_target", C.c_int32),
        ("max_episode_steps", C.c_int32), ("auto_reset", C.c_int32), ("obs_dtype", C.c_int32),
        ("seed", C.c_uint64), ("env_index_base", C.c_int64),
        ("random_outside", C.c_int32), ("outside_density", C.c_float),
        ("soft_vertex_rule", C.c_int32), ("coop_reward", C.c_int32), ("bad_action", C.c_int32), ("lifelong_rng", C.c_int32),
        ("soft_occupancy", C.c_int32), ("abi_version", C.c_int32),
    ]


_lib = None


def build_hint() -> str:
    return ("build it with `python -c 'import __graft_entry__ as g; g.build()'` from the repo root "
            "(or `make -C pogema_amd/csrc`)")


def load() -> C.CDLL:
    """Load the engine library once; raises ImportError loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: the HIP engine is not built; {build_hint()}")
    # torch ships its own libamdhip64.so.7; load it FIRST so that the dynamic loader resolves our
    # NEEDED libamdhip64.so.7 to the very same runtime (two HIP runtimes in one process cannot both
    # own the GPU: the second reports "no ROCm-capable device").
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float
    lib.pgx_abi_version.restype = C.c_int
    lib.pgx_last_error.restype = C.c_char_p
    lib.pgx_create.argtypes = [C.POINTER(PgxConfig), C.c_int, C.POINTER(vp)]
    lib.pgx_destroy.argtypes = [vp]
    lib.pgx_check_config.argtypes = [C.POINTER(PgxConfig)]
    lib.pgx_obs_elems.argtypes = [vp]
    lib.pgx_obs_elems.restype = i64
    lib.pgx_agent_elems.argtypes = [vp]
    lib.pgx_agent_elems.restype = i64
    lib.pgx_reset_from_state.argtypes = [vp, vp, vp, vp, vp]
    lib.pgx_reset_random.argtypes = [vp, f32, u64, vp, vp, i32, vp]
    lib.pgx_regenerate.argtypes = [vp, vp, f32, u64, vp, i32, vp, vp]
    lib.pgx_regenerate_failures.argtypes = [vp, vp]
    lib.pgx_regenerate_failures.restype = i64
    lib.pgx_get_map.argtypes = [vp, vp, vp]
    lib.pgx_buffers_create.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_double, C.POINTER(vp)]
    lib.pgx_buffers_create.restype = C.c_int
    lib.pgx_buffers_create_at.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_double, C.c_double, C.POINTER(vp)]
    lib.pgx_buffers_create_at.restype = C.c_int
    lib.pgx_buffers_ptr.argtypes = [vp, C.c_int]
    lib.pgx_buffers_ptr.restype = vp
    lib.pgx_buffers_get_info.argtypes = [vp, C.POINTER(PgxBuffersInfo)]
    lib.pgx_buffers_get_info.restype = C.c_int
    lib.pgx_buffers_destroy.argtypes = [vp]
    lib.pgx_buffers_destroy.restype = C.c_int
    lib.pgx_np_streams.argtypes = [vp, i64, i32, u64, C.c_double, i64, vp, vp]
    lib.pgx_np_streams.restype = C.c_int
    lib.pgx_np_streams_host.argtypes = [vp, i64, i32, u64, C.c_double, i64, vp]
    lib.pgx_np_streams_host.restype = C.c_int
    lib.pgx_np_generate.argtypes = [vp, i32, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp]
    lib.pgx_np_generate.restype = C.c_int
    lib.pgx_np_generate_host.argtypes = [vp, i32, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp]
    lib.pgx_np_generate_host.restype = C.c_int
    lib.pgx_xcd_tune.argtypes = [vp, vp, vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), vp]
    lib.pgx_xcd_tune.restype = C.c_int
    lib.pgx_get_geometry.argtypes = [vp, i32, C.POINTER(PgxGeometry)]
    lib.pgx_get_geometry.restype = C.c_int
    lib.pgx_xcd_shares.argtypes = [vp, vp]
    lib.pgx_xcd_shares.restype = C.c_int
    lib.pgx_buffers_drop.argtypes = [vp, i32]
    lib.pgx_buffers_drop.restype = C.c_int
    lib.pgx_buffers_va_reserved.argtypes = []
    lib.pgx_buffers_va_reserved.restype = C.c_int64
    lib.pgx_buffers_stride.argtypes = [vp]
    lib.pgx_buffers_stride.restype = C.c_int64
    lib.pgx_rollout.argtypes = [vp, i32, C.POINTER(PgxRolloutIO), vp]
    lib.pgx_rollout.restype = C.c_int
    lib.pgx_expert_actions.argtypes = [vp, i32, vp, i32, vp, vp]
    lib.pgx_expert_actions.restype = C.c_int
    lib.pgx_cost_to_go.argtypes = [vp, i32, vp, vp]
    lib.pgx_cost_to_go.restype = C.c_int
    lib.pgx_cost_to_go_bytes.argtypes = [C.POINTER(PgxConfig)]
    lib.pgx_cost_to_go_bytes.restype = i64
    lib.pgx_cost_to_go_builds.argtypes = [vp, vp]
    lib.pgx_cost_to_go_builds.restype = i64
    lib.pgx_visible_agents.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.pgx_visible_agents.restype = C.c_int
    lib.pgx_pibt_actions.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    lib.pgx_pibt_actions.restype = C.c_int
    lib.pgx_pibt_swap_actions.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    lib.pgx_pibt_swap_actions.restype = C.c_int
    lib.pgx_pibt_plan.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    lib.pgx_pibt_plan.restype = C.c_int
    lib.pgx_pibt_swap_plan.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    lib.pgx_pibt_swap_plan.restype = C.c_int
    lib.pgx_whca_plan.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    lib.pgx_whca_plan.restype = C.c_int
    lib.pgx_repair_plan.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.pgx_repair_plan.restype = C.c_int
    lib.pgx_goal_directions.argtypes = [vp, i32, vp, i32, vp]
    lib.pgx_goal_directions.restype = C.c_int
    lib.pgx_shield_actions.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, vp, vp]
    lib.pgx_shield_actions.restype = C.c_int
    lib.pgx_move_outcomes.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.pgx_move_outcomes.restype = C.c_int
    lib.pgx_policy_input.argtypes = [vp, C.POINTER(i32), i32, i32, vp, vp]
    lib.pgx_policy_input.restype = C.c_int
    lib.pgx_global_state.argtypes = [vp, C.POINTER(i32), i32, i32, vp, vp]
    lib.pgx_global_state.restype = C.c_int
    lib.pgx_global_state_check.argtypes = [i32, C.POINTER(i32), i32, i32, vp]
    lib.pgx_global_state_check.restype = C.c_int
    lib.pgx_agent_tokens.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.pgx_agent_tokens.restype = C.c_int
    lib.pgx_agent_tokens_length.argtypes = [i32, i32]
    lib.pgx_agent_tokens_length.restype = i64
    lib.pgx_goal_paths.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    lib.pgx_goal_paths.restype = C.c_int
    lib.pgx_agent_forecasts.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.pgx_agent_forecasts.restype = C.c_int
    lib.pgx_blocking.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.pgx_blocking.restype = C.c_int
    lib.pgx_path_conflicts.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.pgx_path_conflicts.restype = C.c_int
    lib.pgx_copy_envs.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.pgx_copy_envs.restype = C.c_int
    lib.pgx_set_map_pool.argtypes = [vp, vp, i32, vp, vp]
    lib.pgx_set_map_pool.restype = C.c_int
    lib.pgx_reset_pool.argtypes = [vp, u64, vp, i32, vp]
    lib.pgx_reset_pool.restype = C.c_int
    lib.pgx_regenerate_pool.argtypes = [vp, vp, u64, i32, vp, vp]
    lib.pgx_regenerate_pool.restype = C.c_int
    lib.pgx_get_map_index.argtypes = [vp, vp, vp]
    lib.pgx_get_map_index.restype = C.c_int
    lib.pgx_set_targets.argtypes = [vp, vp, vp, vp]
    lib.pgx_set_targets.restype = C.c_int
    lib.pgx_bad_action_count.argtypes = [vp, vp]
    lib.pgx_bad_action_count.restype = i64
    lib.pgx_time_observe.argtypes = [vp, vp, i32, C.POINTER(C.c_float), vp]
    lib.pgx_time_observe.restype = C.c_int
    lib.pgx_time_observe_pair.argtypes = [vp, vp, vp, i32, C.POINTER(C.c_float), vp]
    lib.pgx_time_observe_pair.restype = C.c_int
    lib.pgx_snapshot_bytes.argtypes = [vp]
    lib.pgx_snapshot_bytes.restype = i64
    lib.pgx_save_snapshot.argtypes = [vp, vp, vp]
    lib.pgx_load_snapshot.argtypes = [vp, vp, vp]
    lib.pgx_save_snapshot.restype = lib.pgx_load_snapshot.restype = C.c_int
    lib.pgx_step.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.pgx_step_held.argtypes = [vp, vp, C.c_int, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.pgx_held_available.argtypes = [vp]
    lib.pgx_step_held.restype = lib.pgx_held_available.restype = C.c_int
    lib.pgx_observe.argtypes = [vp, vp, vp]
    lib.pgx_set_metrics_buffers.argtypes = [vp, vp, vp]
    lib.pgx_get_state.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.pgx_generate.argtypes = [i32, i32, i32, i32, f32, u64, i64, i32, i32, vp, vp, vp]
    lib.pgx_place_agents.argtypes = [i32, i32, i32, i32, u64, i64, i32, i32, vp, i32, vp, vp]
    for name in ("pgx_create", "pgx_destroy", "pgx_reset_from_state", "pgx_reset_random", "pgx_regenerate", "pgx_get_map",
                 "pgx_step", "pgx_observe", "pgx_set_metrics_buffers", "pgx_set_metrics_buffers",
                 "pgx_get_state", "pgx_generate", "pgx_place_agents"):
        getattr(lib, name).restype = C.c_int
    if lib.pgx_abi_version() != PGX_ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {lib.pgx_abi_version()} != expected {PGX_ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(status: int) -> None:
    if status != 0:
        msg = load().pgx_last_error()
        raise PgxError(status, msg.decode("utf-8", "replace") if msg else "unknown error")
