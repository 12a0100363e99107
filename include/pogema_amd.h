/*
 * pogema_amd.h -- C-ABI of the MI355X-native vectorized POGEMA step engine.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * is pure Python and exposes no FFI; the entry points below are what a ctypes binding for
 * `pogema/grid.py` + `pogema/envs.py` (reset()/step()) binds instead of the per-agent Python loops.
 * The mounted reference is a stub (/root/reference/README.md:3,5 -- "code is hosted elsewhere"), so
 * upstream files are cited by name only, never by line; see DESIGN.md section 2.
 *
 * Conventions
 *   - every function returns an int status: 0 = ok, negative = error (PGX_E_*); nothing throws
 *     across the ABI; pgx_last_error() returns a thread-local human-readable message.
 *   - all I/O buffers are owned by the caller.  Pointers documented "device" must be device
 *     pointers on the engine's device (e.g. torch tensor .data_ptr()); "host" are host pointers.
 *   - the engine owns its internal SoA state (obstacle bitmaps, agent/target xy, active masks,
 *     step counters) in HBM on its device.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All device work is
 *     enqueued asynchronously on it; no entry point synchronises unless documented.
 *   - one pgx_env per device shard; a handle is not thread-safe, independent handles may be driven
 *     from different host threads.
 *   - coordinates at the ABI are UNPADDED map coordinates, (x = row, y = column), int32 pairs.
 */
#ifndef POGEMA_AMD_H
#define POGEMA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGX_ABI_VERSION 6

/* error codes */
#define PGX_OK 0
#define PGX_E_INVALID (-1)   /* bad argument / config out of the supported range      */
#define PGX_E_HIP (-2)       /* a HIP runtime call failed (message has the HIP error)  */
#define PGX_E_NOMEM (-3)
#define PGX_E_STATE (-4)     /* call order violated (e.g. step before reset)           */
#define PGX_E_PLACEMENT (-5) /* generator could not place the requested agents         */

/* collision systems -- replaces `Pogema.move_agents` branches (upstream pogema/envs.py) */
#define PGX_COLLISION_PRIORITY 0
#define PGX_COLLISION_BLOCK_BOTH 1
#define PGX_COLLISION_SOFT 2

/* on_target modes -- replaces Pogema / PogemaLifeLong / PogemaCoopFinish */
#define PGX_ON_TARGET_FINISH 0
#define PGX_ON_TARGET_RESTART 1
#define PGX_ON_TARGET_NOTHING 2

/* Switches for the semantics the builder recalls with LOW confidence (docs/SPEC.md open questions Q1, Q2, Q4, Q7; the
 * reference source is not mounted, /root/reference/README.md:3,5).  Value 0 is ALWAYS the recalled-literal behaviour of
 * upstream -- quirks included: bit-exactness targets what upstream does, not what would be tidier -- and the default of
 * every host binding; the other value is the plausible alternative, so that pinning against the real package is a config
 * flip, not a kernel edit.  Every variant is implemented in the step kernel and in both oracles and covered by the
 * parity matrix. */
#define PGX_SOFT_LOWEST_INDEX_WINS 0 /* Q1: `soft`, several movers claim one free/vacated cell: the lowest index moves
                                        (literal `used_cells[cell].remove(agent)` + reverse-index loop)               */
#define PGX_SOFT_ALL_STAY 1          /* Q1 alternative: every claimant of a contested cell stays (textbook MAPF)       */
#define PGX_COOP_REWARD_ALL_SOLVED 0 /* Q4: on_target = NOTHING pays 1.0 to every agent iff ALL are on their goals    */
#define PGX_COOP_REWARD_PER_AGENT 1  /* Q4 alternative: 1.0 to each agent standing on its own goal in this step        */
#define PGX_SOFT_OCCUPANCY_INDEX_ORDER 0 /* Q2: the literal `Grid.move_without_checks` loop as recalled -- clear the old cell,
                                           set the new one, agent by agent in index order: an agent entering the cell a
                                           HIGHER-index agent is leaving stands there but is missing from the occupancy
                                           array (`Grid.positions`: the `agents` planes, pgx_get_state's occupancy) until
                                           its next turn in a later step re-sets it.  (ABI <= 4 numbered this 1.)        */
#define PGX_SOFT_OCCUPANCY_EXACT 1       /* Q2 alternative: after a `soft` step the occupancy array is exactly the set of
                                           visible agents' cells (the invariant every other collision system keeps)      */
#define PGX_BAD_ACTION_NOOP 0        /* Q7: an action outside 0..4 is a noop                                           */
#define PGX_BAD_ACTION_FLAG 1        /* Q7 alternative: still a noop on the device, but counted -- pgx_bad_action_count()
                                        lets the host raise the reference's IndexError                               */

/* Stream of the lifelong (on_target = RESTART) target draw.
 *   BUILD  the build's own counter-based stream (docs/SPEC.md S5), keyed by (seed, global env, agent, draw number)
 *   NUMPY  per-agent numpy generators as upstream `PogemaLifeLong._initialize_grid` sets them up (recalled, conf.
 *          medium): main = default_rng(env_seed); seeds = main.integers(2^31 - 1, size=num_agents);
 *          generator[a] = default_rng(seeds[a]); new target = component[generator[a].integers(0, len(component))]
 *          (= `rnd_generator.choice(component, 1)`), re-created at every reset of the env.  env_seed = cfg.seed + global
 *          env index.  The numpy arithmetic is exact (pgx_np_streams); what stays build-defined is the ORDER of a
 *          component's cells (row-major here; upstream: the order its BFS produced). */
#define PGX_LIFELONG_RNG_BUILD 0
#define PGX_LIFELONG_RNG_NUMPY 1

/* dtype of the `actions` buffer handed to pgx_step */
#define PGX_ACTION_I8 0
#define PGX_ACTION_I32 1
#define PGX_ACTION_I64 2

/* dtype of the observation buffer (pgx_config.obs_dtype).  F32 is the reference's dtype (gymnasium Box float32) and
 * the drop-in default; the others write the same 0/1 planes in a lighter format -- non-drop-in modes for callers whose
 * policy network does not want float32 anyway: U8 one byte per cell (4x lighter; the caller casts), BF16 / F16 two bytes
 * per cell (2x lighter, consumed directly by a mixed-precision network: no cast pass at all -- uint8 plus a cast to
 * bfloat16 on the consumer's side moves as many HBM bytes as float32 did).  0.0 and 1.0 are exact in every format. */
#define PGX_OBS_F32 0
#define PGX_OBS_U8 1
#define PGX_OBS_BF16 2
#define PGX_OBS_F16 3

/* hard limits of this build (upstream's GridConfig admits size 2..1024, obs_radius 1..128, num_agents >= 1 -- recalled,
 * pogema/grid_config.py; README.md "Limits"):
 *   PGX_MAX_SIDE        every map GridConfig admits.  Small maps stage both padded bitmaps of an environment in LDS; from 64 KB
 *                       of bitmaps (~500 x 500 cells) the large-map layout keeps the occupancy bitmap only (pgx_geometry.multi_wave = 2)
 *   PGX_MAX_OBS_RADIUS  a window row is ONE 32-bit mask (2r+1 <= 31): obs_radius 16..128 are refused
 *   PGX_MAX_AGENTS      one workgroup (<= 1024 lanes, one lane per agent) per environment: more agents are refused
 *   LDS                 what one environment keeps in a CU's 160 KB: 4 * PH * ceil(PW / 32) bytes per padded bitmap (PH, PW =
 *                       map + 2r) plus 24 bytes per lane of exchange arrays plus the row masks -- 2 bytes per window row
 *                       and (agent, plane) aliased over the bitmaps for windows up to 16 wide, 4 bytes each IN ADDITION for
 *                       wider ones: e.g. 1024 agents with obs_radius >= 8 do not fit; pgx_check_config says so up front */
#define PGX_MAX_OBS_RADIUS 15   /* window side 2r+1 <= 31 (one 32-bit row mask per window row) */
#define PGX_MAX_AGENTS 1024
#define PGX_MAX_SIDE 1024

/* Mirrors the step-relevant fields of the reference's `GridConfig` (upstream
 * pogema/grid_config.py) plus the batch geometry. */
typedef struct pgx_config {
    int32_t batch;             /* envs held by this handle (this device's shard)               */
    int32_t height, width;     /* unpadded map size (rectangular maps allowed)                 */
    int32_t num_agents;
    int32_t obs_radius;
    int32_t collision_system;  /* PGX_COLLISION_*                                              */
    int32_t on_target;         /* PGX_ON_TARGET_*                                              */
    int32_t max_episode_steps; /* MultiTimeLimit; <= 0 disables truncation        */
    int32_t auto_reset;        /* 1: an env whose agents are all terminated or truncated is   */
                               /*    reset to its stored initial state inside the same step    */
    int32_t obs_dtype;         /* PGX_OBS_* (0 = float32, the reference's dtype; 1 u8, 2 bf16, 3 f16) */
    uint64_t seed;             /* lifelong (restart) target stream seed                        */
    int64_t env_index_base;    /* global index of env 0 of this shard (keeps lifelong streams  */
                               /* independent of how the batch is sharded over devices)        */
    int32_t random_outside;    /* 0: cells beyond the border ring are FREE (`empty_outside=True`, the     */
                               /*    reference's default); 1: Bernoulli(outside_density) obstacles there  */
                               /*    (`empty_outside=False`; the stream is this build's own, keyed by      */
                               /*    seed, global env index and the env's generation counter)             */
    float outside_density;
    int32_t soft_vertex_rule;  /* PGX_SOFT_*        (0 = recalled literal algorithm)                    */
    int32_t coop_reward;       /* PGX_COOP_REWARD_* (0 = recalled)                                       */
    int32_t bad_action;        /* PGX_BAD_ACTION_*  (0 = noop)                                           */
    int32_t lifelong_rng;      /* PGX_LIFELONG_RNG_* (0 = the build's counter-based stream)              */
    int32_t soft_occupancy;    /* PGX_SOFT_OCCUPANCY_* (0 = the literal index-order loop, recalled)      */
    int32_t abi_version;       /* must be PGX_ABI_VERSION of the header the caller was COMPILED against: pgx_create   */
                               /* refuses any other value, so a caller built against an older header fails loudly      */
                               /* instead of getting renumbered semantics (ABI 5 swapped the two soft_occupancy        */
                               /* values: 0 became the index-order loop).  ABI <= 5 had `reserved0 = 0` here.          */
} pgx_config;

typedef struct pgx_env pgx_env; /* opaque */

/* ---- lifecycle -------------------------------------------------------------------------------- */
int pgx_abi_version(void);
const char* pgx_last_error(void);

/* Allocates the device-resident SoA state for cfg->batch environments on `device`.
 * Replaces: constructing `batch` reference env objects (upstream pogema/envs.py `_make_pogema`). */
int pgx_create(const pgx_config* cfg, int device, pgx_env** out);
int pgx_destroy(pgx_env* env);
/* Every check of pgx_create that needs no device -- argument ranges, the limits above, the LDS budget of the launch shape --
 * with the same status codes and pgx_last_error() text: lets a host wrapper refuse a configuration (upstream: pydantic's
 * ValidationError of `GridConfig`) before it touches a GPU.  Needs no HIP device. */
int pgx_check_config(const pgx_config* cfg);

/* Sizes of the caller-owned output buffers, in elements. */
int64_t pgx_obs_elems(const pgx_env* env);   /* batch * agents * 3 * (2r+1)^2   (obs_dtype elements) */
int64_t pgx_agent_elems(const pgx_env* env); /* batch * agents                            */

/* ---- reset -------------------------------------------------------------------------------------- */
/* Installs initial states.  Replaces `Grid.__init__` + `add_artificial_border` (upstream
 * pogema/grid.py) for explicitly given maps/positions.
 *   obstacles  device u8  [batch, height, width]   0 = FREE, 1 = OBSTACLE
 *   agent_xy   device i32 [batch, agents, 2]       unpadded (row, col)
 *   target_xy  device i32 [batch, agents, 2]
 * The state is also stored as the auto-reset state.  For on_target = RESTART this call additionally
 * builds the component tables on the device.  Asynchronous on `stream`. */
int pgx_reset_from_state(pgx_env* env, const uint8_t* obstacles, const int32_t* agent_xy,
                         const int32_t* target_xy, void* stream);

/* On-device reset: draws the instances on the GPU.  Replaces `Grid.__init__` with a random map: upstream
 * pogema/generator.py `generate_obstacles` (Bernoulli(density) obstacles), the BFS component labelling and
 * `generate_positions_and_targets_fast` (starts/targets on distinct free cells, each pair inside one
 * 4-connected component) -- SURVEY L1 / section 8f rank 2 -- plus, for on_target = RESTART, the component
 * tables `PogemaLifeLong` draws new targets from.  The random stream is this build's own counter-based
 * generator (numpy's PCG64 is not reproduced -- DESIGN.md); pgx_generate draws the SAME instances on the
 * host.  Env i of the shard draws instance (seed, env_index_base + i): seed and global env index are separate key
 * components (hashed one after the other), so batches reset with different seeds share no instance.
 *   shared_map  device u8 [height, width] or NULL   given map for every env (GridConfig.map): only
 *                                                   starts/targets are drawn, `density` is ignored
 *   env_mask    device u8 [batch] or NULL           NULL: every env, generation 0 (a pure function of
 *                                                   seed and env index).  Otherwise only the flagged envs
 *                                                   get a NEW instance (their generation counter advances);
 *                                                   their step counters and metric accumulators restart.
 * One kernel builds one env per workgroup, retries included; the call then synchronises `stream` once to read the
 * device's failure count: PGX_E_PLACEMENT if an env cannot be filled after `max_retries` re-draws (<= 0: 10). */
int pgx_reset_random(pgx_env* env, float density, uint64_t seed, const uint8_t* shared_map,
                     const uint8_t* env_mask, int32_t max_retries, void* stream);

/* Asynchronous form of the masked reset, for use right after pgx_step: NEW instances for the envs flagged in
 * `env_mask` (device u8 [batch], e.g. the `episode_done` buffer of pgx_set_metrics_buffers), then -- when `obs` is
 * not NULL -- the observations of exactly those envs are rewritten in `obs` (same buffer/dtype as pgx_step's).
 * This is the reference's auto-reset wrapper with `seed=None` (a fresh random instance per episode) for a whole
 * batch, without a host round trip: nothing here synchronises.  An env that cannot be filled within `max_retries`
 * attempts (<= 0: 3) keeps its previous instance and is counted; pgx_regenerate_failures() returns that count
 * (it synchronises `stream`).  Needs one scratch slot per env (9 bytes per cell and env, allocated on first use). */
int pgx_regenerate(pgx_env* env, const uint8_t* env_mask, float density, uint64_t seed, const uint8_t* shared_map,
                   int32_t max_retries, void* obs, void* stream);
int64_t pgx_regenerate_failures(pgx_env* env, void* stream);

/* ---- map pool (docs/SPEC.md S10) ----------------------------------------------------------------------------- */
/* A pool is num_maps >= 1 maps of the handle's height x width, nonzero = obstacle.  With a pool installed,
 * pgx_reset_pool / pgx_regenerate_pool give env i (global index e = env_index_base + i, generation `epoch`) the map
 *   k = ((splitmix64(h0 ^ 0x504F4F4C00000000) >> 32) * num_maps) >> 32,   h0 = GEN v2's key of attempt 0
 * and place its agents on pool[k] exactly as pgx_reset_random does on a shared map.  The map choice depends on
 * (seed, e, epoch) only, so shards draw the same instances as one handle.
 *
 * pgx_set_map_pool copies `maps` (device u8 [num_maps, height, width]) into the handle, labels the components of every
 * map once and checks that each can hold num_agents start/target pairs (sum over its components of floor(size / 2)):
 * otherwise PGX_E_PLACEMENT naming the first such map, and no pool is installed.  `capacity_out` (host i32 [num_maps],
 * may be NULL) receives every map's capacity.  It synchronises `stream` once to read the capacities and is refused
 * (PGX_E_STATE) inside a graph capture.  A pool of the same num_maps reuses the handle's buffers (stream-ordered copy,
 * so a graph captured over pgx_regenerate_pool draws from the new pool); another size synchronises the device and
 * reallocates.  Current instances are kept until each env's next reset.  Device memory: 5 bytes per cell and map.
 * map_index (pgx_get_map_index, device i32 [batch]) is the pool index of each env's map, -1 after any other install
 * (pgx_reset_from_state, pgx_reset_random, pgx_regenerate, a snapshot taken without a pool) or before any pool.
 * A handle with a pool installed appends map_index to its snapshot (pgx_snapshot_bytes grows by the aligned size). */
int pgx_set_map_pool(pgx_env* env, const uint8_t* maps, int32_t num_maps, int32_t* capacity_out, void* stream);
/* pgx_reset_random on the pool: env_mask, max_retries (<= 0: 10), the generation counters, the status and the one
 * synchronisation are those of pgx_reset_random.  PGX_E_STATE without a pool. */
int pgx_reset_pool(pgx_env* env, uint64_t seed, const uint8_t* env_mask, int32_t max_retries, void* stream);
/* pgx_regenerate on the pool: asynchronous, no host sync; failures (max_retries <= 0: 3) keep the previous instance and
 * are counted by pgx_regenerate_failures.  Needs 4 bytes of scratch per cell and env (allocated on first use). */
int pgx_regenerate_pool(pgx_env* env, const uint8_t* env_mask, uint64_t seed, int32_t max_retries, void* obs,
                        void* stream);
int pgx_get_map_index(pgx_env* env, int32_t* map_index, void* stream);

/* The unpadded obstacle maps currently installed: device u8 [batch, height, width] (`Grid.get_obstacles`). */
int pgx_get_map(pgx_env* env, uint8_t* obstacles, void* stream);

/* ---- the hot path ------------------------------------------------------------------------------- */
/* One environment step for every env of the shard.  Replaces, per env, `Pogema.step` /
 * `PogemaLifeLong.step` / `PogemaCoopFinish.step` including `move_agents`, `Grid.move`, the
 * `_obs()` gather (`get_obstacles_for_agent`, `get_positions`, `get_square_target`) and
 * `MultiTimeLimit.step` (upstream pogema/envs.py, pogema/grid.py,
 * pogema/wrappers/multi_time_limit.py).
 *   actions      device [batch, agents] of action_dtype, values 0..4 (noop, up, down, left, right)
 *   obs          device f32 (or u8 / bf16 / f16, per pgx_config.obs_dtype) [batch, agents, 3, 2r+1, 2r+1]
 *                (obstacles, agents, target)                                               may be NULL
 *   rewards      device f32 [batch, agents]
 *   terminated   device u8  [batch, agents]
 *   truncated    device u8  [batch, agents]
 *   is_active    device u8  [batch, agents]   infos[i]['is_active'] after the step      may be NULL */
int pgx_step(pgx_env* env, const void* actions, int action_dtype, void* obs, float* rewards,
             uint8_t* terminated, uint8_t* truncated, uint8_t* is_active, void* stream);

/* pgx_step for an output set that the caller KEEPS between calls: the same step, the same five outputs, but the launch
 * may leave out stores of target-plane zeros that `obs` still holds from the previous pgx_step_held call that wrote it.
 *   held      device u8 [batch, agents], one per `obs` buffer, owned by the caller together with it: the flat window index
 *             (row * (2r+1) + col) of the 1.0 that the last pgx_step_held left in each agent's target plane of `obs`;
 *             255 = unknown.  Read and rewritten by the call.
 *   refresh   != 0: nothing is assumed about `obs` -- every byte is written, `held` is recorded.  Pass it whenever
 *             anything but pgx_step_held with this `held` may have written `obs` since (or `held` is not initialised).
 * With refresh == 0 the result is the one of pgx_step provided `obs` holds exactly what the previous call with this
 * `held` left in it.  Exists for float32 observations with obs_radius <= 7 outside the large-map layout
 * (pgx_held_available); for any other configuration, and with obs == NULL or held == NULL, this IS pgx_step.
 * Like pgx_step it only enqueues one launch (the kernel is configured at pgx_create) and can be captured in a HIP graph. */
int pgx_step_held(pgx_env* env, const void* actions, int action_dtype, void* obs, uint8_t* held, int32_t refresh,
                  float* rewards, uint8_t* terminated, uint8_t* truncated, uint8_t* is_active, void* stream);
/* 1 when pgx_step_held has a kernel of its own for this handle's configuration, 0 when it runs pgx_step */
int pgx_held_available(const pgx_env* env);

/* How pgx_step's workgroups (one per environment, or per group of small environments) are shared out over the 8 XCDs:
 * shares[x] of them run on XCD x (host pointer, 8 entries).  Equal by default.  The XCDs do not get through their
 * observation streams equally fast (the odd ones lag 5-15 %), and with equal shares the fast ones
 * idle at the end of every launch: pgx_xcd_tune() runs the observation pass into `obs` and `obs_alt` in turn (the buffers
 * pgx_step will write; obs_alt may be NULL) a few times, reads when each XCD finished its share, shifts work towards the fast ones and keeps the shares that gave
 * the shortest launch (never worse than equal: equal is the first candidate).  Synchronises `stream`; nothing in the
 * engine's state changes.  us_equal / us_tuned (may be NULL): the pass with equal shares and with the kept ones.
 * PGX_XCD_WEIGHTS=w0,...,w7 sets the shares at pgx_create instead (diagnostic). */
/* Both assume ONE compute partition of 8 XCDs (SPX): on any other device (pgx_geometry.xcd_aware == 0) the mapping is the
 * identity, the shares stay equal and pgx_xcd_tune returns at once with 0 / 0. */
int pgx_xcd_shares(pgx_env* env, int32_t* shares);
int pgx_xcd_tune(pgx_env* env, void* obs, void* obs_alt, int32_t rounds, float* us_equal, float* us_tuned, void* stream);

/* The launch shape pgx_step (for_rollout = 0) or pgx_rollout (1) uses for this handle -- read-only, for tests and
 * benchmarks that must show they ran the SAME kernel variant (tests/test_fullsize_gpu.py asserts that its parity
 * engines and bench.py's engine agree for every BASELINE config) and for reading a profile: which template instance
 * (lanes_per_env, multi_wave, p16), how many waves per workgroup and environments per wave, which store flavour.
 * Chosen once in pgx_create from (batch, num_agents, map, obs_radius, obs_dtype) and the PGX_* tuning overrides. */
typedef struct pgx_geometry {
    int32_t lanes_per_env;  /* G: lanes of a wave one environment occupies (power of two; 64 when multi_wave)       */
    int32_t waves;          /* waves per workgroup                                                                   */
    int32_t envs_per_wave;  /* environments per single-wave workgroup (1 when multi_wave)                            */
    int32_t multi_wave;     /* 1: one environment per workgroup of `waves` waves (num_agents > 64, or helper waves);
                               2: the same in the LARGE-MAP layout (the two padded bitmaps of an environment exceed 64 KB, ~500 x 500
                               cells and up): only the occupancy bitmap lives in LDS, obstacles are read through the L2  */
    int32_t p16;            /* 1: window side <= 16, packed 16-bit row masks                                         */
    int32_t stagger;        /* cohort stagger of the single-wave kernel (0 = off)                                    */
    int32_t store_policy;   /* observation stores AS EXECUTED: 0 plain, 1 nontemporal, 2 sc1 write-through (the lighter */
                            /* formats' generic funnels know 0 and 1 only: a chosen 2 runs -- and is reported -- as 0)  */
    int32_t state_stores;   /* when the small per-step result stores are issued: 0 at once, 1 after the LDS barrier, 2 after the stream */
    int32_t grid;           /* workgroups launched                                                                   */
    int32_t lds_bytes;      /* dynamic LDS per workgroup                                                             */
    int32_t for_rollout;    /* echo of the argument                                                                  */
    int32_t xcd_aware;      /* 1: the device is one 8-XCD compute partition (SPX, 256 CUs): XCD-contiguous workgroup mapping,
                               tunable per-XCD shares, cohort stagger.  0: anything else (CPX/DPX/QPX partitions, other parts):
                               identity mapping, equal shares, no stagger, pgx_xcd_tune is a no-op -- same results        */
} pgx_geometry;
int pgx_get_geometry(const pgx_env* env, int32_t for_rollout, pgx_geometry* out);

/* K steps in ONE launch: the same as `steps` consecutive pgx_step calls with actions[t] -- bit for bit, state and outputs
 * -- for callers that have the actions up front (executing MAPF plans, scripted or random policies, replaying recorded
 * episodes): upstream, the `for t in range(K): env.step(actions[t])` loop around `Pogema.step`.  Every workgroup takes its
 * own environments through all K steps, so there is no launch boundary between steps and one wave's collision resolve
 * runs under the other waves' observation streams.  All pointers are device pointers.
 *   actions       [steps, batch, agents] of action_dtype, or NULL: the engine's uniform random policy -- action
 *                 (h >> 32) * 5 >> 32 of a splitmix64 chain over (policy_seed, cfg.env_index_base + env, agent,
 *                 policy_step0 + t), the same whatever the sharding; written to actions_out ([steps, batch, agents] i8)
 *                 when that is not NULL
 *   obs           [obs_slots, batch, agents, 3, 2r+1, 2r+1] f32 (u8 with PGX_OBS_U8) or NULL; step t writes slot
 *                 t % obs_slots: obs_slots = steps keeps the whole trajectory, 1 only the last observation.
 *                 obs_slot_stride: bytes from one slot to the next; 0 = dense.  (pgx_buffers_stride() for a ring made
 *                 of zone-spread buffers.)
 *   rewards       [steps, batch, agents] f32
 *   terminated, truncated   [steps, batch, agents] u8
 *   is_active     [steps, batch, agents] u8 or NULL
 *   episode_done  [steps, batch] u8 or NULL          1 where the env's episode finished in that step
 *   metrics       [steps, batch, 6] f32 or NULL      written only where episode_done is 1 (as pgx_set_metrics_buffers)
 * The buffers of pgx_set_metrics_buffers are not touched.  auto_reset works as in pgx_step; pgx_regenerate has no
 * place inside the launch (PGX_E_INVALID is never returned for it: the caller simply does not call it). */
typedef struct pgx_rollout_io {
    const void* actions;
    void* obs;
    float* rewards;
    uint8_t* terminated;
    uint8_t* truncated;
    uint8_t* is_active;
    uint8_t* episode_done;
    float* metrics;
    int32_t action_dtype;
    int32_t obs_slots;
    int64_t obs_slot_stride;
    uint64_t policy_seed;
    int64_t policy_step0;
    int8_t* actions_out;
} pgx_rollout_io;
int pgx_rollout(pgx_env* env, int32_t steps, const pgx_rollout_io* io, void* stream);

/* Overwrites the current targets of the agents flagged in `agent_mask` (device u8 [batch, agents]; NULL = all agents).
 *   target_xy  device i32 [batch, agents, 2]  unpadded (row, col); must be free cells inside the map (not checked)
 * `PogemaLifeLong` draws new targets from per-agent numpy generators (upstream pogema/envs.py `_generate_new_target`,
 * pogema/generator.py); the engine's own lifelong stream is a different one (docs/SPEC.md S5).  This call lets a caller
 * supply the targets instead -- a user-defined task generator, or the recorded target sequence of a reference rollout
 * (tests/test_golden_reference.py replays lifelong fixtures this way).  The stored initial targets (auto-reset state)
 * are not touched.  Asynchronous on `stream`. */
int pgx_set_targets(pgx_env* env, const int32_t* target_xy, const uint8_t* agent_mask, void* stream);

/* Shortest-path expert (docs/SPEC.md "Shortest-path expert"), read from the current device state -- the state the next
 * pgx_step reads, which this call does not change.  For every agent:
 *   distance  device i32 [batch, agents]   length of a shortest 4-connected path from the agent's cell to its current
 *             target over the free cells of the height x width map (cells outside it are never traversed, whatever
 *             random_outside says); 0 on the target; -1 when there is no path or the agent is not active (bit 0 of
 *             is_active clear).  May be NULL.
 *   actions   device [batch, agents] of action_dtype (PGX_ACTION_*): the lowest of 1..4 (up, down, left, right) whose
 *             neighbour cell is at distance d - 1; 0 when d <= 0.
 *   flags     PGX_EXPERT_AGENTS_AS_OBSTACLES: the cell of every OTHER active agent is blocked too (never the agent's own
 *             cell or its own target cell).
 * Replaces a host BFS per agent over `Grid.get_obstacles` (upstream's A* baseline pogema/a_star_policy.py plans on its
 * remembered observations instead).  Asynchronous on `stream`, no host sync, capturable in a HIP graph.
 * PGX_E_STATE before the first reset, like pgx_step.
 * Maps wider or taller than 64: the first call with PGX_EXPERT_AGENTS_AS_OBSTACLES allocates 4 * batch * height *
 * ceil(width / 32) bytes of device scratch (an occupancy bitmap) that the handle keeps; made inside a graph capture, that
 * first call returns PGX_E_STATE instead -- make it once outside the capture. */
#define PGX_EXPERT_AGENTS_AS_OBSTACLES 1
int pgx_expert_actions(pgx_env* env, int32_t flags, void* actions, int32_t action_dtype, int32_t* distance, void* stream);

/* Cost-to-go windows (docs/SPEC.md S11), read from the current device state -- the state the next pgx_step reads, which
 * this call does not change.  For every agent, its (2r+1) x (2r+1) window (r = obs_radius) in the orientation of
 * observation plane 0:
 *   out   device i32 [batch, agents, 2r+1, 2r+1]; out[b, i, u, v] is the 4-connected shortest-path length from cell
 *         (x - r + u, y - r + v) to the agent's current target over the free cells of the height x width map (as
 *         pgx_expert_actions' distance: cells outside the map are never traversed); -1 outside the map, on an obstacle,
 *         for a cell not connected to the target, for every cell when the target is an obstacle, and for every cell of
 *         an agent that is not active (bit 0 of is_active clear).  The centre of an active agent equals
 *         pgx_expert_actions' distance without PGX_EXPERT_AGENTS_AS_OBSTACLES.
 *   flags reserved, must be 0.
 * The handle caches one distance field per agent and rebuilds it only when the agent is active and its field is missing,
 * was built for another target cell, or was built on another map of its env (a changed map invalidates the whole env);
 * every other field is reused, however the state changed (resets, auto-reset, map pools, pgx_set_targets, lifelong
 * draws, pgx_load_snapshot).  A call without a state change since the previous one builds nothing.
 * The first call allocates the cache, pgx_cost_to_go_bytes() bytes that the handle keeps until pgx_destroy; made inside a
 * graph capture, that first call returns PGX_E_STATE instead (make it once outside), and a failed allocation returns
 * PGX_E_NOMEM / PGX_E_HIP naming the bytes.  Afterwards asynchronous on `stream`, no host sync, capturable in a HIP graph.
 * PGX_E_STATE before the first reset, like pgx_step. */
int pgx_cost_to_go(pgx_env* env, int32_t flags, int32_t* out, void* stream);
/* Device bytes of pgx_cost_to_go's cache for `cfg`, needing no device: 16 (build counter) + the fields, B * A * H * W
 * cells of 2 bytes when H * W <= 65536 (a distance is at most 65534, 0xFFFF is "unreachable") and of 4 bytes above,
 * rounded up to a multiple of 16 + 4 * B * A (target tags) + 4 * B * H * ceil(W / 32) (map copies).  Returns the status
 * code of pgx_check_config for a configuration it refuses. */
int64_t pgx_cost_to_go_bytes(const pgx_config* cfg);
/* Distance fields pgx_cost_to_go, pgx_pibt_actions, pgx_pibt_plan, pgx_pibt_swap_plan, pgx_whca_plan, pgx_repair_plan, pgx_goal_directions
 * and pgx_shield_actions have built since the handle was created (0 before the first call of any of them).  Synchronises `stream`. */
int64_t pgx_cost_to_go_builds(pgx_env* env, void* stream);

/* Neighbour lists (docs/SPEC.md S12), read from the current device state -- the state the next pgx_step reads, which
 * this call does not change.  With r = obs_radius, agent j is VISIBLE to agent i of the same env iff j != i, bit 0 of
 * is_active[j] is set, and |dx| <= r and |dy| <= r for dx = x_j - x_i, dy = y_j - y_i: the square window of the
 * observation; obstacles hide nobody, as in observation plane 1.  An agent whose own bit 0 is clear sees nobody.  The
 * visible agents of i are ordered by the key (dx * dx + dy * dy, dx + r, dy + r, j), ascending, compared
 * lexicographically: nearest first, ties in the row-major order of the window, then by agent index.
 *   k       entries per agent, 1..PGX_MAX_NEIGHBOURS
 *   flags   reserved, must be 0
 *   index   device i32 [batch, agents, k]     the first min(count, k) visible agents in that order (agent index inside
 *           the env), then -1.  Must not be NULL.
 *   offset  device i8  [batch, agents, k, 2]  (dx, dy) of the same entries, (0, 0) where index is -1.  May be NULL.
 *   count   device i32 [batch, agents]        the number of visible agents, NOT capped by k (count > k: the list was
 *           truncated); 0 for an agent that is not active.  May be NULL.
 * index and count must be 4-byte aligned, offset 2-byte aligned.  Replaces a [batch, agents, agents] distance
 * broadcast and a top-k on the host side.  One kernel launch: allocates nothing (the first call included), asynchronous
 * on `stream`, no host sync, capturable in a HIP graph.  PGX_E_INVALID for a k outside its range, non-zero flags, a
 * NULL or misaligned output; PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_MAX_NEIGHBOURS 32
int pgx_visible_agents(pgx_env* env, int32_t k, int32_t flags, int32_t* index, int8_t* offset, int32_t* count, void* stream);

/* Cooperative one-step planner (docs/SPEC.md S13): PIBT, priority inheritance with backtracking, read from the current
 * device state -- the state the next pgx_step reads, which this call does not change.  An agent is PLANNED iff bit 0 of
 * is_active is set.  Every planned agent gets a next cell among its own cell and its four neighbours (inside the
 * height x width map, free of obstacles), preferred by the distance to its current target (pgx_cost_to_go's field of
 * the agent; unreachable = infinite), then unoccupied before occupied, then the lower action.  Agents are served by
 * (-priority, index); an agent that wants an occupied cell makes the cell's agent plan first (it inherits the turn) and
 * takes its next candidate when that agent cannot move away.  No two planned agents share a next cell, no two swap
 * cells.  Agents that are not planned get action 0 and their own cell; they occupy and reserve nothing.
 *   flags     reserved, must be 0
 *   priority  device i32 [batch, agents]; NULL: every priority is 0 (index order)
 *   actions   device [batch, agents] of action_dtype (PGX_ACTION_*): 0 stay, 1..4 up, down, left, right.  Must not be
 *             NULL.
 *   next_xy   device i32 [batch, agents, 2]: the next cells, unpadded (row, col).  May be NULL.
 * Under PGX_COLLISION_SOFT a pgx_step with these actions puts every planned agent on its next cell; under the other
 * two collision systems a move into a cell another agent leaves in the same step may be reverted.
 * Shares pgx_cost_to_go's distance-field cache: the call refreshes it (stale fields are rebuilt and counted by
 * pgx_cost_to_go_builds) and then plans in one more launch.  Whichever entry point that uses the cache is called first allocates
 * it (pgx_cost_to_go_bytes() bytes), under pgx_cost_to_go's rules: inside a graph capture that first call
 * returns PGX_E_STATE, a failed allocation returns PGX_E_NOMEM / PGX_E_HIP naming the bytes.  Afterwards asynchronous
 * on `stream`, no host sync, capturable in a HIP graph.  PGX_E_INVALID for a NULL `actions`, non-zero flags, a bad
 * action_dtype or a misaligned pointer (checked before the handle: no device needed); PGX_E_STATE before the first
 * reset, like pgx_step. */
int pgx_pibt_actions(pgx_env* env, int32_t flags, const int32_t* priority, void* actions, int32_t action_dtype,
                     int32_t* next_xy, void* stream);

/* Cooperative one-step planner with the swap operation (docs/SPEC.md S23): pgx_pibt_actions' planner -- the same planned
 * agents, candidate cells, order of the candidates, serving order, reservations and outputs -- plus the rule that lets
 * two agents change places in a corridor or a dead end.  An agent whose best cell leads into a corridor it cannot pass
 * while another agent has to come out of it (decided by two walks along the corridor, from the state alone) tries its
 * candidates BACK TO FRONT, and when its first-tried candidate holds, the other agent (its partner) is pulled into the
 * cell it leaves.  A walk takes at most PGX_SWAP_MAX_WALK steps; a longer corridor counts as "no swap" -- the cap is part
 * of the semantics.  Every guarantee of pgx_pibt_actions holds: no two planned agents share a next cell, no two swap
 * cells, and under PGX_COLLISION_SOFT a pgx_step with these actions puts every planned agent on its next cell.  A
 * heuristic: it solves corridor and dead-end instances the plain planner livelocks on and loses a few the plain planner
 * solves, which is why it is an entry point of its own.
 *   flags     reserved, must be 0
 *   priority, actions, action_dtype, next_xy   as in pgx_pibt_actions
 * Cache, allocation, capture, status codes and the order of the checks (arguments before the handle: no device needed)
 * are pgx_pibt_actions': the call refreshes pgx_cost_to_go's distance-field cache and then plans in one more launch. */
#define PGX_SWAP_MAX_WALK 2048
int pgx_pibt_swap_actions(pgx_env* env, int32_t flags, const int32_t* priority, void* actions, int32_t action_dtype,
                          int32_t* next_xy, void* stream);

/* Multi-step planner (docs/SPEC.md S16): pgx_pibt_actions' planner iterated `horizon` times inside one launch, on a
 * private copy of the positions -- the call reads the current device state and changes none of it.  The targets and
 * their distance fields are held for the whole lookahead.  Step h plans from the cells step h - 1 sent the agents to;
 * the agents planned at step 0 are those with bit 0 of is_active set, and under PGX_ON_TARGET_FINISH an agent stops
 * being planned once its next cell is its target (under the other two modes it stays planned, on the same target).  An
 * agent's priority becomes 0 when it is not planned any more or its next cell is its target and grows by 1 (two's
 * complement wrap) otherwise -- the textbook growing priorities.  pgx_pibt_actions' guarantees hold for every step.
 *   flags         0, or PGX_PLAN_FIXED_PRIORITY: the priorities stay as given for the whole lookahead
 *   horizon       K, 1..PGX_MAX_PLAN_HORIZON
 *   priority      device i32 [batch, agents], the priorities of step 0; NULL: all 0
 *   actions       device [K, batch, agents] of action_dtype (PGX_ACTION_*), the layout pgx_rollout reads.  Must not be
 *                 NULL.
 *   path_xy       device i32 [K, batch, agents, 2]: the cell step h sends each agent to, unpadded (row, col); an agent
 *                 that is not planned keeps its cell.  May be NULL.
 *   arrival       device i32 [batch, agents]: for an agent planned at step 0 the smallest h in 0..K such that it stands
 *                 on its target after h steps (0: it stands there now), -1 when there is none; -1 for every other agent.
 *                 May be NULL.
 *   priority_out  device i32 [batch, agents]: the priorities after step K - 1, to continue from.  May be NULL.
 * With horizon = 1, actions and path_xy are pgx_pibt_actions' outputs.  Under PGX_COLLISION_SOFT with
 * PGX_ON_TARGET_FINISH or PGX_ON_TARGET_NOTHING a pgx_rollout of `actions` puts every agent on path_xy[h] after step h
 * for as long as the env's episode lasts (the plan knows neither the step limit nor auto-reset); under
 * PGX_ON_TARGET_RESTART the plan is exact up to the first arrival in the env (the engine then draws a target the plan
 * cannot know); under the other collision systems pgx_pibt_actions' caveat applies from the first reverted move on.
 * Shares pgx_cost_to_go's distance-field cache under pgx_pibt_actions' rules: ONE refresh per call whatever K is, then
 * one more launch; whichever entry point that uses the cache is called first allocates it -- inside a graph capture
 * that first call returns PGX_E_STATE.  Afterwards asynchronous on `stream`, no host sync, capturable in a HIP graph.
 * PGX_E_INVALID for a NULL `actions`, unknown flag bits, a horizon outside its range, a bad action_dtype or a misaligned
 * pointer (checked before the handle: no device needed); PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_PLAN_FIXED_PRIORITY 1
#define PGX_MAX_PLAN_HORIZON 256
int pgx_pibt_plan(pgx_env* env, int32_t flags, int32_t horizon, const int32_t* priority, void* actions,
                  int32_t action_dtype, int32_t* path_xy, int32_t* arrival, int32_t* priority_out, void* stream);

/* Multi-step planner with the swap operation (docs/SPEC.md S27): pgx_pibt_plan's lookahead -- the private copy of the
 * positions, the targets and distance fields held for all steps, the planned / arrival / priority rules, the outputs --
 * with pgx_pibt_swap_actions' planner in place of pgx_pibt_actions' at every step.  The swap rule is evaluated on the
 * positions and the planned agents of the step it plans: an agent that stopped being planned under
 * PGX_ON_TARGET_FINISH stands in nobody's way, is nobody's partner and parks in no dead end.  A corridor walk takes at
 * most PGX_SWAP_MAX_WALK steps in every step of the lookahead; the cap is part of the semantics.  pgx_pibt_actions'
 * guarantees hold for every step.  With horizon = 1, actions and path_xy are pgx_pibt_swap_actions' outputs; in an env
 * in which the rule reverses no agent's candidates at any step, all four outputs are pgx_pibt_plan's.
 *   flags, horizon, priority, actions, action_dtype, path_xy, arrival, priority_out   as in pgx_pibt_plan
 * What pgx_pibt_plan says about pgx_rollout following path_xy holds here too.  Cache, allocation, capture (ONE refresh
 * per call whatever K is, then one more launch), status codes and the order of the checks (arguments before the handle:
 * no device needed) are pgx_pibt_plan's. */
int pgx_pibt_swap_plan(pgx_env* env, int32_t flags, int32_t horizon, const int32_t* priority, void* actions,
                       int32_t action_dtype, int32_t* path_xy, int32_t* arrival, int32_t* priority_out, void* stream);

/* Windowed cooperative A* against a reservation table (WHCA*, docs/SPEC.md S28): prioritized planning in space-time,
 * read from the current device state, which the call does not change.  The planned agents (bit 0 of is_active) of an env
 * are served in the order (-priority, index).  Each gets a path of K = horizon steps over its own cell and the free
 * cells of the map that avoids every cell (vertex reservation) and every head-on move (edge reservation) of the agents
 * served before it: layer R_h is the set of cells it can stand on after h steps, R_0 its own cell.  Under
 * PGX_ON_TARGET_FINISH the search ends at the first layer that holds the target, and the agent reserves nothing after
 * that step; otherwise it ends at the cell of R_K with the smallest (distance to the target, row-major index) -- the
 * distance is pgx_cost_to_go's field of the agent, the Manhattan distance to its own cell when the target cannot be
 * reached.  The path is read back from the end, the lowest action first, so an agent reaches its end cell as early as
 * the reservations allow and waits there.  An agent with an empty layer has FAILED: it stays on its cell, which it
 * reserves for the whole window, so that later agents plan around it.  Agents that are not planned get action 0, keep
 * their cell and reserve nothing; cells of agents not served yet are not reserved.  Prioritized planning is incomplete:
 * `failed` is how it says so, other priorities are the remedy.
 *   flags     reserved, must be 0
 *   horizon   K, 1..PGX_MAX_WHCA_HORIZON (the cap is part of the semantics: the box an agent can reach is 63 x 63 cells)
 *   priority  device i32 [batch, agents]; NULL: every priority is 0 (index order)
 *   actions   device [K, batch, agents] of action_dtype (PGX_ACTION_*), the layout pgx_rollout reads.  Must not be NULL.
 *   path_xy   device i32 [K, batch, agents, 2]: the cell after step h + 1, unpadded (row, col) -- pgx_pibt_plan's layout,
 *             what pgx_path_conflicts takes with PGX_CONFLICT_PATHS_PLAN.  May be NULL.
 *   arrival   device i32 [batch, agents]: for a planned agent the smallest h in 0..K at which its path stands on its
 *             target, -1 when there is none; -1 for every other agent.  May be NULL.
 *   failed    device i32 [batch, agents]: 1 for a failed agent, else 0.  May be NULL.
 * From a state in which the planned agents stand on distinct cells, no two planned agents that did not fail meet in a
 * cell or swap cells at any step (an agent that ended on its target under PGX_ON_TARGET_FINISH takes no part after
 * that step).  In an env without a failed agent, under PGX_COLLISION_SOFT with PGX_ON_TARGET_FINISH or
 * PGX_ON_TARGET_NOTHING, a pgx_rollout of `actions` puts every agent on path_xy[h] after step h for as long as the env's
 * episode lasts; pgx_pibt_plan's caveats for PGX_ON_TARGET_RESTART and the other collision systems apply.
 * Shares pgx_cost_to_go's distance-field cache under pgx_pibt_plan's rules: ONE refresh per call, then one more launch;
 * whichever entry point that uses the cache is called first allocates it -- inside a graph capture that first call
 * returns PGX_E_STATE.  Afterwards asynchronous on `stream`, no host sync, capturable in a HIP graph.  PGX_E_INVALID for
 * a NULL `actions`, non-zero flags, a horizon outside its range, a bad action_dtype or a misaligned pointer (checked
 * before the handle: no device needed); PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_MAX_WHCA_HORIZON 31
int pgx_whca_plan(pgx_env* env, int32_t flags, int32_t horizon, const int32_t* priority, void* actions,
                  int32_t action_dtype, int32_t* path_xy, int32_t* arrival, int32_t* failed, void* stream);

/* Plan repair (docs/SPEC.md S29): pgx_whca_plan for chosen agents, around the paths the others keep.  Read from the
 * current device state, which the call does not change.  For a planned agent i, given_i[0] is its cell and given_i[h] =
 * paths[h - 1, b, i].  Its given path is a WALK when, scanning h = 1, 2, ..., every given_i[h] lies inside the map (this
 * is checked first: the cells may be any int32), is no obstacle and differs from given_i[h - 1] by one of the five moves,
 * stay included.  Under PGX_ON_TARGET_FINISH the scan stops at the first h >= 1 with given_i[h] on the agent's target:
 * that h is the agent's last step and whatever `paths` holds after it is ignored; otherwise the last step is K.
 * A planned agent with replan == 0 (or replan NULL) whose given path is a walk is KEPT: its cells are the given ones up
 * to its last step and the last of them from there on.  Every other planned agent is REPLANNED.  All kept agents are
 * entered into the reservation table first -- the cell of every step up to the last, every real move; conflicts among
 * them are neither looked for nor resolved, that is pgx_path_conflicts' job.  Then the replanned agents are served in the
 * order (-priority, index), each exactly as pgx_whca_plan serves an agent, against the kept agents and the replanned
 * agents served before it.  Agents that are not planned are treated as by pgx_whca_plan; their `paths` rows are ignored.
 *   flags      reserved, must be 0
 *   horizon    K, 1..PGX_MAX_WHCA_HORIZON
 *   paths      device i32 [K, batch, agents, 2]: pgx_pibt_plan's / pgx_whca_plan's path_xy layout.  Must not be NULL.
 *   replan     device u8 [batch, agents], non-zero: replan this agent.  NULL: only agents whose path is no walk.
 *   priority   device i32 [batch, agents]; NULL: every priority is 0 (index order)
 *   actions    device [K, batch, agents] of action_dtype.  Must not be NULL.  A kept agent: the action from cell h to
 *              cell h + 1 up to its last step, 0 afterwards; the others as by pgx_whca_plan.
 *   path_xy    device i32 [K, batch, agents, 2], as pgx_whca_plan's.  May be NULL, and may be `paths` itself: a workgroup
 *              reads every `paths` row of its env before it stores anything.  Any other overlap of an output with
 *              `paths` or `replan` is undefined.
 *   arrival    device i32 [batch, agents]: pgx_whca_plan's rule on the output cells.  May be NULL.
 *   failed     device i32 [batch, agents]: 1 for a replanned agent whose search ran empty, else 0.  May be NULL.
 *   replanned  device i32 [batch, agents]: 1 for every replanned agent -- asked for, or its given path was no walk --
 *              else 0.  May be NULL.
 * With replan all ones the first four outputs are pgx_whca_plan's.  From a state with the planned agents on distinct
 * cells: where the kept agents are free of conflicts among themselves (an agent that arrived under PGX_ON_TARGET_FINISH
 * takes no part afterwards) and no agent failed, no two planned agents meet in a cell or swap cells at any step, and
 * what pgx_whca_plan says about pgx_rollout holds.  Cache, allocation, capture (ONE refresh per call, then one more
 * launch), LDS (pgx_whca_plan's formula), status codes and the order of the checks are pgx_whca_plan's; `paths` NULL or
 * misaligned is PGX_E_INVALID too. */
int pgx_repair_plan(pgx_env* env, int32_t flags, int32_t horizon, const int32_t* paths, const uint8_t* replan,
                    const int32_t* priority, void* actions, int32_t action_dtype, int32_t* path_xy, int32_t* arrival,
                    int32_t* failed, int32_t* replanned, void* stream);

/* Collision shielding (docs/SPEC.md S15): pgx_pibt_actions' planner -- the same planned agents, serving order
 * (-priority, index), priority inheritance, backtracking, outputs and guarantees -- with every agent's candidate cells
 * ordered by the caller's action scores instead of by the distance to its target.  Among the agent's own cell and its
 * four neighbours that lie inside the map and are free of obstacles (the others are dropped whatever their score: the
 * call is also the action mask), the higher score comes first, then the lower action; -0.0 equals +0.0, +inf and -inf
 * are ordinary values and a NaN ranks below -inf.  Every planned agent gets the best-scored action that is jointly
 * collision-free, for any scores.  The call is deterministic: to sample, add Gumbel noise to the logits first.
 *   flags       0, or PGX_SHIELD_TIE_DISTANCE: equal scores are ordered as pgx_pibt_actions orders its candidates
 *               (distance to the target, unoccupied first) before the action; with all five scores of every agent
 *               equal the result is pgx_pibt_actions' bit for bit
 *   scores      device [batch, agents, 5] of score_dtype (PGX_SCORES_*), contiguous, aligned to its element size;
 *               entry a is the score of action a.  Must not be NULL.
 *   priority    device i32 [batch, agents]; NULL: every priority is 0 (index order)
 *   actions     device [batch, agents] of action_dtype (PGX_ACTION_*).  Must not be NULL.
 *   next_xy     device i32 [batch, agents, 2]: the next cells, unpadded (row, col).  May be NULL.
 *   overridden  device u8 [batch, agents]: 1 iff the agent is planned and its action is not the argmax of its five
 *               scores (ties to the lowest action, NaN lowest), else 0.  May be NULL.
 * Without PGX_SHIELD_TIE_DISTANCE: one kernel launch that reads no distance field; allocates nothing (the first call
 * included), asynchronous on `stream`, no host sync, capturable in a HIP graph from the first call.  With it the call
 * shares pgx_cost_to_go's distance-field cache under pgx_pibt_actions' rules: it refreshes the cache, and whichever entry
 * point that uses the cache is called first allocates it -- inside a graph capture that first call returns PGX_E_STATE.
 * PGX_E_INVALID for a NULL `scores` or `actions`, unknown flag bits, a bad score_dtype or action_dtype or a misaligned
 * pointer (checked before the handle: no device needed); PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_SCORES_F32 0
#define PGX_SCORES_F16 1
#define PGX_SCORES_BF16 2
#define PGX_SHIELD_TIE_DISTANCE 1
int pgx_shield_actions(pgx_env* env, int32_t flags, const void* scores, int32_t score_dtype, const int32_t* priority,
                       void* actions, int32_t action_dtype, int32_t* next_xy, uint8_t* overridden, void* stream);

/* Move outcomes (docs/SPEC.md S17): what the move phase of pgx_step(actions) would do to every agent, and why a move
 * that fails does, read from the current device state -- the state the next pgx_step reads, which this call does not
 * change.  The engine's collision system and soft_vertex_rule apply.  An action outside 0..4 counts as 0 whatever
 * bad_action says: the call never fails for it and never moves pgx_bad_action_count.  With cur the agent's cell,
 * d = cur + MOVES[action], a mover = an agent with bit 0 of is_active set and an action of 1..4, o = the lowest-index
 * active agent standing on d, and next = the cell the agent stands on after the move phase (cur or d), the code of an
 * agent is the first that applies:
 *   PGX_OUTCOME_STAY       not a mover (inactive, noop, out-of-range action)
 *   PGX_OUTCOME_MOVED      next == d
 *   PGX_OUTCOME_OBSTACLE   d is an obstacle (the ring around the map included)
 *   PGX_OUTCOME_SWAP       o exists, is a mover and its d is this agent's cur
 *   PGX_OUTCOME_OCCUPIED   o exists and stays where it is
 *   PGX_OUTCOME_FOLLOW     o exists and leaves, no other mover claims d, and the collision system forbids following
 *   PGX_OUTCOME_CONTESTED  otherwise: another mover claims d
 *   actions   device [batch, agents] of action_dtype (PGX_ACTION_*), as pgx_step takes them.  Must not be NULL.
 *   flags     reserved, must be 0
 *   next_xy   device i32 [batch, agents, 2]: next, unpadded (row, col); an inactive agent's own cell.  May be NULL.
 *   outcome   device u8 [batch, agents]: the code.  May be NULL.
 *   blocker   device i32 [batch, agents]: o for SWAP, OCCUPIED and FOLLOW; for CONTESTED the lowest-index other mover
 *             that claims d; -1 otherwise.  May be NULL.
 *   counts    device i32 [batch, PGX_NUM_OUTCOMES]: active agents of the env per code; a row sums to the env's number
 *             of active agents.  May be NULL.
 * At least one output must not be NULL.  One kernel launch: allocates nothing (the first call included), asynchronous
 * on `stream`, no host sync, capturable in a HIP graph from the first call.  PGX_E_INVALID for a NULL `actions`, four
 * NULL outputs, non-zero flags, a bad action_dtype or a misaligned pointer (checked before the handle: no device
 * needed); PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_OUTCOME_STAY 0
#define PGX_OUTCOME_MOVED 1
#define PGX_OUTCOME_OBSTACLE 2
#define PGX_OUTCOME_SWAP 3
#define PGX_OUTCOME_OCCUPIED 4
#define PGX_OUTCOME_FOLLOW 5
#define PGX_OUTCOME_CONTESTED 6
#define PGX_NUM_OUTCOMES 7
int pgx_move_outcomes(pgx_env* env, const void* actions, int32_t action_dtype, int32_t flags, int32_t* next_xy,
                      uint8_t* outcome, int32_t* blocker, int32_t* counts, void* stream);

/* Direction-to-goal planes (docs/SPEC.md S14), the "heuristic channels" of learned MAPF policies, read from the current
 * device state -- the state the next pgx_step reads, which this call does not change.  For every agent, window cell
 * (u, v) = map cell c = (x - r + u, y - r + v) in the orientation of observation plane 0, and move a of 1..4 (up, down,
 * left, right): plane a - 1 is 1 at (u, v) iff the distance of c to the agent's current target (pgx_cost_to_go's field)
 * is defined and the distance of the cell move a leads to from c is defined and smaller.  That cell may lie outside the
 * window: it is looked up in the field all the same, which is what pgx_cost_to_go's windows cannot give.  All four
 * planes are 0 on the target cell, wherever pgx_cost_to_go gives -1 (outside the map, obstacles, cells not connected to
 * the target, every cell when the target is an obstacle) and for an agent that is not active (bit 0 of is_active
 * clear).  Other agents are not obstacles.  The lowest plane set at the window centre is pgx_expert_actions' action
 * without PGX_EXPERT_AGENTS_AS_OBSTACLES.
 *   flags   reserved, must be 0
 *   out     device buffer, must not be NULL, of `format`:
 *           PGX_DIRECTIONS_F32   f32 [batch, agents, 4, 2r+1, 2r+1]  0.0 / 1.0 (4-byte aligned)
 *           PGX_DIRECTIONS_U8    u8  [batch, agents, 4, 2r+1, 2r+1]  0 / 1
 *           PGX_DIRECTIONS_BITS  u8  [batch, agents, 2r+1, 2r+1]     bit a - 1 = plane a - 1, bits 4..7 zero
 *           Any alignment beyond that is accepted, at a price: a 16-byte aligned `out` is written with 16-byte
 *           stores, any other with one store per element (per byte for the two u8 formats), which is markedly
 *           slower.  Keep `out` 16-byte aligned on a hot path (a fresh device allocation is).
 * Shares pgx_cost_to_go's distance-field cache: the call refreshes it (stale fields are rebuilt and counted by
 * pgx_cost_to_go_builds) and then gathers in one more launch.  Whichever of pgx_cost_to_go, pgx_pibt_actions and this
 * entry point is called first allocates the cache (pgx_cost_to_go_bytes() bytes), under pgx_cost_to_go's rules: inside a
 * graph capture that first call returns PGX_E_STATE, a failed allocation returns PGX_E_NOMEM / PGX_E_HIP naming the
 * bytes.  Afterwards asynchronous on `stream`, no host sync, capturable in a HIP graph.  PGX_E_INVALID for non-zero
 * flags, a NULL `out`, an unknown format or a misaligned float32 `out` (checked before the handle: no device needed);
 * PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_DIRECTIONS_F32 0
#define PGX_DIRECTIONS_U8 1
#define PGX_DIRECTIONS_BITS 2
int pgx_goal_directions(pgx_env* env, int32_t flags, void* out, int32_t format, void* stream);

/* Path-to-goal planes and sub-goals (docs/SPEC.md S22), the input and the reward signal of planning-plus-learning
 * policies ("Learn to Follow" style), read from the current device state -- the state the next pgx_step reads, which
 * this call does not change.  With r = obs_radius, W = 2r + 1 and D the agent's distance field (pgx_cost_to_go's), the
 * PATH of an agent at cell p0 is p0, p1, ...: p(k+1) = p(k) + MOVES[a] for the lowest a of 1..4 (up, down, left, right)
 * whose destination has a defined distance strictly smaller than p(k)'s -- the lowest plane pgx_goal_directions sets
 * at p(k), so p1 is the cell pgx_expert_actions moves to.  The MARKED PREFIX p1..pn ends at the first of: p(n) is the
 * target; p(n+1) lies outside the agent's W x W window (nothing after it is marked, even if the path re-enters);
 * n = the cap.  n <= W * W - 1 whatever the field holds.  n = 0 for an agent that is not active (bit 0 of is_active
 * clear; its field is not read), stands on its target or has no path to it: zero planes, sub-goal (0, 0), length 0.
 *   flags    reserved, must be 0
 *   steps    0: no cap; 1..PGX_MAX_PATH_STEPS: the cap (one above W * W - 1 behaves like 0)
 *   format   of `planes`, checked even when `planes` is NULL:
 *            PGX_PATHS_F32   f32 [batch, agents, W, W]  1.0 at window cell (u, v) iff it is one of p1..pn, else 0.0
 *                            (4-byte aligned); the orientation of observation plane 0; the centre is never marked
 *            PGX_PATHS_U8    u8  [batch, agents, W, W]  1 / 0
 *            PGX_PATHS_ROWS  i32 [batch, agents, W]     bit v of word u = cell (u, v); bit 31 is never set (4-byte aligned)
 *   planes   device buffer of `format`, or NULL: no plane is written at all.  A 16-byte aligned `planes` is written
 *            with 16-byte stores, any other with one store per element.
 *   subgoal  device i8 [batch, agents, 2], or NULL: the offset (dx, dy) of p(n) from p0 in pgx_visible_agents' convention
 *   length   device i32 [batch, agents], 4-byte aligned, or NULL: n.  n <= the centre of pgx_cost_to_go's window, with
 *            equality iff the prefix ended on the target.
 * Shares pgx_cost_to_go's distance-field cache exactly as pgx_goal_directions does: the call refreshes it (stale fields
 * are rebuilt and counted by pgx_cost_to_go_builds) and then walks in one more launch; whichever entry point uses the
 * cache first allocates it -- inside a graph capture that first call returns PGX_E_STATE, a failed allocation
 * PGX_E_NOMEM / PGX_E_HIP naming the bytes.  Afterwards asynchronous on `stream`, no host sync, capturable in a HIP
 * graph.  PGX_E_INVALID when all three outputs are NULL, for non-zero flags, an unknown format, steps outside
 * 0..PGX_MAX_PATH_STEPS, a misaligned float32 or rows `planes` or a misaligned `length` (checked before the handle: no
 * device needed); PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_PATHS_F32 0
#define PGX_PATHS_U8 1
#define PGX_PATHS_ROWS 2
#define PGX_MAX_PATH_STEPS 960
int pgx_goal_paths(pgx_env* env, int32_t flags, int32_t steps, int32_t format, void* planes, int8_t* subgoal,
                   int32_t* length, void* stream);

/* Agent forecasts (docs/SPEC.md S24), the planes PRIMAL2-style policies add to their input: where the other agents an
 * observer can see are going to be at t+1 .. t+K if each follows its own shortest path -- read from the current device
 * state, the state the next pgx_step reads, which this call does not change.  With r = obs_radius, W = 2r + 1, K = steps
 * and D_j agent j's distance field (pgx_cost_to_go's), the FORECAST of an agent at cell p0 is q(0) = p0, q(s+1) = q(s) +
 * MOVES[a] for the lowest a of 1..4 (up, down, left, right) whose destination lies inside the map and has a defined
 * distance strictly smaller than q(s)'s -- pgx_goal_paths' rule with no window ending it -- and q(s+1) = q(s) when there is
 * no such move (on the target, or no defined distance at q(s)): it waits there for all later s.  Other agents are not
 * obstacles.  The trip count is exactly K whatever a field holds.  An agent that is not active (bit 0 of is_active
 * clear) has no forecast and its field is not read.
 *   steps    K, 1..PGX_MAX_FORECAST_STEPS
 *   format   of `planes`, checked even when `planes` is NULL:
 *            PGX_FORECAST_F32   f32 [batch, agents, K, W, W]  plane s-1 of observer i is 1.0 at window cell (u, v) iff i
 *                               is active and some active agent j != i that i sees NOW (|x_j - x_i| <= r and
 *                               |y_j - y_i| <= r, pgx_visible_agents' rule, every such agent however many) has
 *                               q_j(s) - p0_i = (u - r, v - r); else 0.0 (4-byte aligned).  The orientation of
 *                               observation plane 0.  A forecast cell outside the window is not drawn (no clamp), two
 *                               forecasts on one cell give 1, the ghost bit does not matter, the observer's own
 *                               forecast is not in its planes.
 *            PGX_FORECAST_U8    u8  [batch, agents, K, W, W]  1 / 0
 *            PGX_FORECAST_ROWS  i32 [batch, agents, K, W]     bit v of word u = cell (u, v); bit 31 is never set (4-byte
 *                               aligned)
 *   flags    reserved, must be 0
 *   planes   device buffer of `format`, or NULL: no plane is written at all.  A 16-byte aligned `planes` is written
 *            with 16-byte stores, any other with one store per element.
 *   cells    device i16 [batch, agents, K, 2], 2-byte aligned, never NULL (the plane pass reads it): cells[b, j, s-1] =
 *            q_j(s) as (x, y) in pgx_get_state's coordinates; (-1, -1) for every s of an agent that is not active.
 * Shares pgx_cost_to_go's distance-field cache exactly as pgx_goal_paths does: the call refreshes it (stale fields are
 * rebuilt and counted by pgx_cost_to_go_builds), then walks every agent in one launch and, with `planes`, gathers in a
 * second one; whichever entry point uses the cache first allocates it -- inside a graph capture that first call returns
 * PGX_E_STATE, a failed allocation PGX_E_NOMEM / PGX_E_HIP naming the bytes.  Afterwards asynchronous on `stream`, no
 * host sync, capturable in a HIP graph.  PGX_E_INVALID for a NULL `cells`, non-zero flags, an unknown format, steps
 * outside 1..PGX_MAX_FORECAST_STEPS, a misaligned float32 or rows `planes` or an odd `cells` address (checked before the
 * handle: no device needed); PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_FORECAST_F32 0
#define PGX_FORECAST_U8 1
#define PGX_FORECAST_ROWS 2
#define PGX_MAX_FORECAST_STEPS 8
int pgx_agent_forecasts(pgx_env* env, int32_t steps, int32_t format, int32_t flags, void* planes, int16_t* cells,
                        void* stream);

/* Blocking counts (docs/SPEC.md S25), the blocking penalty of PRIMAL / PRIMAL2 / SCRIMP style rewards: which agents
 * stand in the way of others -- read from the current device state, the state the next pgx_step reads, which this call
 * does not change.  Agents are never obstacles for each other's paths; only the one blocker under test is.  For an
 * ordered pair (i, j), i != j, of one env with c = cell of i, s = cell of j, t = target of j and d0 = D_j[s] (D_j agent j's
 * distance field, pgx_cost_to_go's), the pair is ELIGIBLE iff both are active (bit 0 of is_active), j is visible to i by
 * pgx_visible_agents' rule (|x_j - x_i| <= r and |y_j - y_i| <= r, every such agent however many) and, with
 * PGX_BLOCKING_ON_TARGET, i stands on its own target.  i BLOCKS j iff the pair is eligible, d0 is defined, s != c and no
 * path from s to t of at most d0 + inflation - 1 steps exists on the map with cell c made an obstacle: a detour of at
 * least `inflation` steps, a cut-off agent and c == t alike.
 *   inflation   1..PGX_MAX_BLOCKING_INFLATION (PRIMAL uses 10; 1: "c lies on every shortest path of j")
 *   flags       0 or PGX_BLOCKING_ON_TARGET
 *   count       device i32 [batch, agents], 4-byte aligned, or NULL: count[b, i] = the number of j that i blocks
 *   blocked_by  device i32 [batch, agents], 4-byte aligned, or NULL: blocked_by[b, j] = the number of i that block j
 * Agents that are not active get 0 in both; per env the two outputs have the same sum.  A pair with D_j[c] undefined or
 * D_j[c] + |c - s|_1 > d0 is not blocked and is dismissed without a search (c is on no shortest path of j); every other
 * eligible pair takes one breadth-first search of at most d0 + inflation - 1 levels that ends as soon as t is reached.
 * Shares pgx_cost_to_go's distance-field cache exactly as pgx_goal_paths does: the call refreshes it (stale fields are
 * rebuilt and counted by pgx_cost_to_go_builds) and then counts; whichever entry point uses the cache first allocates
 * it -- inside a graph capture that first call returns PGX_E_STATE, a failed allocation PGX_E_NOMEM / PGX_E_HIP naming the
 * bytes.  Afterwards asynchronous on `stream`, no host sync, capturable in a HIP graph.  PGX_E_INVALID when both outputs
 * are NULL, for an inflation outside 1..PGX_MAX_BLOCKING_INFLATION, an unknown flag bit or a misaligned output (checked
 * before the handle: no device needed); PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_BLOCKING_ON_TARGET 1
#define PGX_MAX_BLOCKING_INFLATION 64
int pgx_blocking(pgx_env* env, int32_t inflation, int32_t flags, int32_t* count, int32_t* blocked_by, void* stream);

/* Path conflicts (docs/SPEC.md S26): where K-step paths run into each other, per agent -- the conflict count and first
 * conflict of conflict-based priorities, the "who is in my way" of selective communication, a K-step collision signal,
 * and the validator of a plan.  Reads the current device state, the state the next pgx_step reads, and the caller's
 * paths; changes neither.  With K = steps, pos_0[i] the agent's current cell, pos_h[i] = the path's cell h (h = 1..K) and
 * tgt[i] its current target, agent i TAKES PART at h (h = 0..K) iff bit 0 of is_active is set, pos_h[i] lies inside the
 * H x W map and, when agents vanish, no h' < h has pos_h'[i] == tgt[i].  Cells are keys, not moves: consecutive cells need
 * not be adjacent, any int value is a cell outside the map.  For h >= 1 and agents i != j of one env:
 *   PGX_CONFLICT_VERTEX  both take part at h and pos_h[i] == pos_h[j]
 *   PGX_CONFLICT_EDGE    both take part at h and h-1, pos_h[i] == pos_h-1[j], pos_h[j] == pos_h-1[i], pos_h[i] != pos_h-1[i]
 *   PGX_CONFLICT_FOLLOW  (on the follower i only) both take part at h and h-1, pos_h[i] == pos_h-1[j],
 *                        pos_h[i] != pos_h-1[i], pos_h[j] != pos_h-1[j], and not an edge conflict
 * The kinds exclude each other for one (h, i, j).  An INCIDENCE of i is a pair (h, j) in a kind named in `flags`.
 *   paths       device buffer, never NULL, of `layout`:
 *               PGX_CONFLICT_PATHS_PLAN   i32 [K, batch, agents, 2], 4-byte aligned: pgx_pibt_plan's path_xy
 *               PGX_CONFLICT_PATHS_CELLS  i16 [batch, agents, K, 2], 2-byte aligned: pgx_agent_forecasts' cells
 *               unpadded (x, y) in pgx_get_state's coordinates
 *   steps       K, 1..PGX_MAX_CONFLICT_STEPS
 *   flags       at least one of PGX_CONFLICT_VERTEX / _EDGE / _FOLLOW: the kinds that exist for this call; and at most
 *               one of PGX_CONFLICT_STAY (an agent on its target keeps taking part) and PGX_CONFLICT_VANISH (it does not,
 *               from the step after the first one on its target); with neither, agents vanish iff on_target is
 *               PGX_ON_TARGET_FINISH -- pgx_pibt_plan's rule, so a plan is judged the way it was made
 *   first_step  device i32 [batch, agents]: the smallest h with an incidence, -1 if none
 *   partner     device i32 [batch, agents]: the lowest j over the incidences at first_step, -1 if none
 *   kind        device u8  [batch, agents]: the OR of the kind bits over the incidences at first_step, 0 if none
 *   count       device i32 [batch, agents]: the number of incidences over all h
 * Each output may be NULL, not all four; the int32 ones are 4-byte aligned.  An agent that is not active gets -1, -1, 0,
 * 0.  The results are a minimum, an OR and a sum over sets: deterministic.  One launch that reads no distance field and
 * allocates nothing: asynchronous on `stream`, no host sync, capturable in a HIP graph from the first call.
 * PGX_E_INVALID for a NULL `paths`, four NULL outputs, steps outside 1..PGX_MAX_CONFLICT_STEPS, an unknown layout, an
 * unknown flag bit, no kind bit, both arrival flags, a misaligned `paths` or int32 output (checked before the handle: no
 * device needed); PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_CONFLICT_PATHS_PLAN 0
#define PGX_CONFLICT_PATHS_CELLS 1
#define PGX_CONFLICT_VERTEX 1
#define PGX_CONFLICT_EDGE 2
#define PGX_CONFLICT_FOLLOW 4
#define PGX_CONFLICT_STAY 8
#define PGX_CONFLICT_VANISH 16
#define PGX_MAX_CONFLICT_STEPS 256
int pgx_path_conflicts(pgx_env* env, const void* paths, int32_t layout, int32_t steps, int32_t flags,
                       int32_t* first_step, int32_t* partner, uint8_t* kind, int32_t* count, void* stream);

/* Policy input (docs/SPEC.md S18): the stack of binary window planes a learnt MAPF policy reads, written once, in the
 * order and the number format the network takes -- read from the current device state, the state the next pgx_step
 * reads, which this call does not change.  Plane c of every agent's window is the channel channels[c]:
 *   PGX_CHANNEL_OBSTACLES    plane 0 of pgx_observe, bit for bit (the border ring and random_outside included)
 *   PGX_CHANNEL_AGENTS       plane 1 of pgx_observe, bit for bit (hidden agents absent, soft_occupancy honoured)
 *   PGX_CHANNEL_TARGET       plane 2 of pgx_observe, bit for bit (the agent's target, clamped per axis to the window)
 *   PGX_CHANNEL_OTHER_GOALS  1 at (r + clamp(fx_j - x, -r, r), r + clamp(fy_j - y, -r, r)) for the target (fx_j, fy_j)
 *                            of every agent j that pgx_visible_agents calls visible to this agent at (x, y) -- another
 *                            agent with bit 0 of is_active set, standing in the window -- however many there are; all
 *                            zero for an agent that is not active itself
 *   PGX_CHANNEL_UP, _DOWN, _LEFT, _RIGHT   planes 0..3 of pgx_goal_directions, bit for bit
 * For an agent that is not active, the first three are what pgx_observe writes for it and the other five are zero.
 *   channels      host array of num_channels distinct PGX_CHANNEL_* codes, read before the call returns
 *   num_channels  1..PGX_NUM_CHANNELS
 *   dtype         PGX_OBS_F32, PGX_OBS_U8, PGX_OBS_BF16 or PGX_OBS_F16: the elements of `out`, 0 / 1 in that format;
 *                 chosen per call, whatever obs_dtype the handle was created with
 *   out           device buffer [batch, agents, num_channels, 2r+1, 2r+1] of dtype, must not be NULL, aligned to its
 *                 element size.  A 16-byte aligned `out` is written with 16-byte stores, any other with one store per
 *                 element, which is markedly slower (a fresh device allocation is aligned).
 * Without a direction channel the call is one launch that reads no distance field and allocates nothing: asynchronous
 * on `stream`, no host sync, capturable in a HIP graph from the first call; pgx_cost_to_go_builds does not move.  With
 * one it shares pgx_cost_to_go's cache exactly as pgx_goal_directions does: the stale fields are rebuilt (and counted)
 * first, and whichever entry point uses the cache first allocates it -- inside a graph capture that first call returns
 * PGX_E_STATE, a failed allocation PGX_E_NOMEM / PGX_E_HIP naming the bytes.  PGX_E_INVALID for a NULL `channels` or
 * `out`, a count outside 1..PGX_NUM_CHANNELS, a code outside 0..7 or given twice, an unknown dtype or a misaligned `out`
 * (checked before the handle: no device needed); PGX_E_STATE before the first reset, like pgx_step. */
#define PGX_CHANNEL_OBSTACLES 0
#define PGX_CHANNEL_AGENTS 1
#define PGX_CHANNEL_TARGET 2
#define PGX_CHANNEL_OTHER_GOALS 3
#define PGX_CHANNEL_UP 4
#define PGX_CHANNEL_DOWN 5
#define PGX_CHANNEL_LEFT 6
#define PGX_CHANNEL_RIGHT 7
#define PGX_NUM_CHANNELS 8
int pgx_policy_input(pgx_env* env, const int32_t* channels, int32_t num_channels, int32_t dtype, void* out, void* stream);

/* Global state (docs/SPEC.md S20): the picture of the whole map a centralised critic, a value mixer or a central planner
 * reads, [batch, num_channels, H, W] with H, W the unpadded map size, row x, column y (pgx_get_map's orientation,
 * pgx_get_state's coordinates), written once, in the order and the number format the caller takes -- read from the
 * current device state, the state the next pgx_step reads, which this call does not change.  Plane c is the channel
 * channels[c]; its value at cell (x, y):
 *   PGX_GLOBAL_OBSTACLES   pgx_get_map's byte of the env as it is now (after regeneration, pool draws and pgx_copy_envs),
 *                          bit for bit for the 0 / 1 maps the engine installs
 *   PGX_GLOBAL_AGENTS      the interior of pgx_get_state's occupancy array, bit for bit: 1 iff an agent whose is_active
 *                          byte is exactly 1 stands there (hidden agents and soft_occupancy ghosts are absent, as in
 *                          observation plane 1)
 *   PGX_GLOBAL_TARGETS     1 iff it is the target of at least one agent with bit 0 of is_active set (a ghost's target
 *                          counts, a finished, hidden agent's does not)
 *   PGX_GLOBAL_AGENT_IDS   i + 1 for the lowest index i among the agents PGX_GLOBAL_AGENTS counts on the cell, else 0
 *   PGX_GLOBAL_TARGET_IDS  j + 1 for the lowest index j among the agents PGX_GLOBAL_TARGETS counts whose target is the
 *                          cell, else 0 (lifelong targets may coincide)
 *   channels      host array of num_channels distinct PGX_GLOBAL_* codes, read before the call returns
 *   num_channels  1..PGX_NUM_GLOBAL_CHANNELS
 *   dtype         PGX_OBS_F32, PGX_OBS_U8, PGX_OBS_BF16 or PGX_OBS_F16: the elements of `out`; chosen per call, whatever
 *                 obs_dtype the handle was created with.  With an id channel the format must hold num_agents exactly:
 *                 PGX_OBS_U8 up to PGX_GLOBAL_ID_MAX_U8 agents, PGX_OBS_BF16 up to PGX_GLOBAL_ID_MAX_BF16, the other two
 *                 every count the engine accepts
 *   out           device buffer [batch, num_channels, H, W] of dtype, must not be NULL, aligned to its element size.  A
 *                 16-byte aligned `out` is written with 16-byte stores but for the few elements around a plane whose
 *                 start is not 16-byte aligned (odd H * W in a narrow format); any other `out` works the same way,
 *                 with those few elements at every plane.
 * One launch that allocates nothing: asynchronous on `stream`, no host sync, capturable in a HIP graph from the first
 * call after a reset; pgx_cost_to_go_builds does not move.  A workgroup holds a band of whole rows of at most
 * PGX_GLOBAL_BAND_CELLS cells at a time (PGX_GLOBAL_BAND_CELLS / W rows).  PGX_E_INVALID for a NULL `channels` or `out`,
 * a count outside 1..PGX_NUM_GLOBAL_CHANNELS, a code outside 0..4 or given twice, an unknown dtype, a misaligned `out` or
 * an id channel in a format too narrow for the handle's num_agents (all checked before the device is touched);
 * PGX_E_STATE before the first reset, like pgx_step.
 * pgx_global_state_check makes the same argument checks, in the same order and with the same messages, for an engine of
 * `num_agents` agents without a handle: PGX_OK where pgx_global_state would go on to the handle. */
#define PGX_GLOBAL_OBSTACLES 0
#define PGX_GLOBAL_AGENTS 1
#define PGX_GLOBAL_TARGETS 2
#define PGX_GLOBAL_AGENT_IDS 3
#define PGX_GLOBAL_TARGET_IDS 4
#define PGX_NUM_GLOBAL_CHANNELS 5
#define PGX_GLOBAL_ID_MAX_U8 255
#define PGX_GLOBAL_ID_MAX_BF16 256
#define PGX_GLOBAL_BAND_CELLS 8192
int pgx_global_state(pgx_env* env, const int32_t* channels, int32_t num_channels, int32_t dtype, void* out, void* stream);
int pgx_global_state_check(int32_t num_agents, const int32_t* channels, int32_t num_channels, int32_t dtype, const void* out);

/* Agent tokens (docs/SPEC.md S21): the input of a token- or attention-based policy (MAPF-GPT style), one row of
 * `length` one-byte token ids per agent, written once in one launch -- read from the current device state, the state
 * the next pgx_step reads, which this call does not change.  With r = obs_radius, W = 2r + 1, S = slots and
 * L0 = W * W + PGX_TOKEN_SLOT_LEN * S (pgx_agent_tokens_length), the row of agent i of env b is
 *   an inactive agent (bit 0 of is_active clear): `length` times PGX_TOKEN_PAD;
 *   entries 0 .. W*W-1: the agent's pgx_cost_to_go window, row-major: PGX_TOKEN_BLOCKED where the window holds -1 or the
 *       agent's own cell (the window's centre) does, else clamp(cell - centre, -PGX_TOKEN_CLIP, PGX_TOKEN_CLIP) +
 *       PGX_TOKEN_CLIP;
 *   entries W*W + 10 s .. W*W + 10 s + 9, slot s: slot 0 is the agent itself with (dx, dy) = (0, 0), slot s >= 1 is
 *       entry s - 1 of pgx_visible_agents(k = S - 1): agent j at offset (dx, dy).  Ten times PGX_TOKEN_PAD where that
 *       list has no entry (index -1), else
 *         +0, +1   dx + PGX_TOKEN_CLIP, dy + PGX_TOKEN_CLIP
 *         +2, +3   clamp(target of j - position of i, -PGX_TOKEN_CLIP, PGX_TOKEN_CLIP) + PGX_TOKEN_CLIP, per axis
 *         +4..+8   history[b][j][0..4]: PGX_TOKEN_ACTION0 + v for v in 0..4, PGX_TOKEN_ACTION_NONE for every other
 *                  value and without a history
 *         +9       PGX_TOKEN_GREEDY0 + m, m = pgx_goal_directions' PGX_DIRECTIONS_BITS mask at the centre of j's window;
 *   entries L0 .. length-1: PGX_TOKEN_PAD.
 * Token ids 0 .. 2 * PGX_TOKEN_CLIP are the integers -PGX_TOKEN_CLIP .. PGX_TOKEN_CLIP; there are PGX_NUM_TOKENS ids.
 *   slots    1..PGX_MAX_TOKEN_SLOTS, the agent included
 *   length   L0..PGX_MAX_TOKEN_LENGTH
 *   flags    must be 0
 *   history  device buffer int8 [batch, num_agents, PGX_TOKEN_HISTORY], most recent action first, or NULL; only read
 *   tokens   device buffer uint8 [batch, num_agents, length], must not be NULL; any alignment works, rows whose bytes
 *            fill whole 16-byte lines of the buffer are written with 16-byte stores
 * Shares pgx_cost_to_go's cache: stale fields are rebuilt first (pgx_cost_to_go_builds counts them), and the first call
 * of any entry point that uses the cache allocates it -- PGX_E_STATE inside a graph capture; later calls are asynchronous
 * on `stream`, need no host sync and can be captured.  PGX_E_INVALID for slots, length or flags outside their ranges or
 * a NULL `tokens` (checked before the device is touched); PGX_E_STATE before the first reset, like pgx_step.
 * pgx_agent_tokens_length needs no handle: W * W + PGX_TOKEN_SLOT_LEN * slots, -1 for an obs_radius outside
 * 1..PGX_MAX_OBS_RADIUS or slots outside 1..PGX_MAX_TOKEN_SLOTS. */
#define PGX_TOKEN_CLIP 20
#define PGX_TOKEN_BLOCKED 41
#define PGX_TOKEN_ACTION_NONE 42
#define PGX_TOKEN_ACTION0 43
#define PGX_TOKEN_GREEDY0 48
#define PGX_TOKEN_PAD 64
#define PGX_NUM_TOKENS 65
#define PGX_TOKEN_HISTORY 5
#define PGX_TOKEN_SLOT_LEN 10
#define PGX_MAX_TOKEN_SLOTS 32
#define PGX_MAX_TOKEN_LENGTH 2048
int pgx_agent_tokens(pgx_env* env, int32_t slots, int32_t length, int32_t flags, const int8_t* history, uint8_t* tokens, void* stream);
int64_t pgx_agent_tokens_length(int32_t obs_radius, int32_t slots);

/* Number of out-of-range actions (outside 0..4) that ACTIVE agents submitted since the last call (bad_action =
 * PGX_BAD_ACTION_FLAG only; otherwise always 0).  Inactive agents' actions are never looked at, as in the reference's
 * `if self.grid.is_active[agent_idx]` guards.  Synchronises `stream`, then clears the counter.  The host side turns a
 * non-zero count into the reference's IndexError (`MOVES[action]`). */
int64_t pgx_bad_action_count(pgx_env* env, void* stream);

/* Episode metrics, fused into pgx_step.  Replaces the metric wrappers of upstream pogema/wrappers/metrics.py
 * (ISR / CSR / ep_length / SoC / makespan, their non-disappearing forms for on_target = NOTHING, and
 * avg_throughput for lifelong), which put `infos[0]['metrics']` on the step that ends an episode.
 * Registers caller-owned device buffers written by every following pgx_step (NULL disables either):
 *   metrics       f32 [batch, 6]  ISR, CSR, ep_length, SoC, makespan, avg_throughput -- a row is written only
 *                                 on the step in which that env's episode finishes
 *   episode_done  u8  [batch]     1 iff all agents of the env are terminated or truncated in this step */
#define PGX_NUM_METRICS 6
int pgx_set_metrics_buffers(pgx_env* env, float* metrics, uint8_t* episode_done);

/* Observation of the current state without stepping.  Replaces `PogemaBase._obs()` as called by
 * `reset()`. */
int pgx_observe(pgx_env* env, void* obs, void* stream);

/* Placement probe.  On MI355X the speed of the observation stream depends on WHERE the output buffer lives: equal
 * 2 MiB-aligned hipMalloc'd buffers fall into tiers of ~140 / ~144 / ~153 us per configs[2] step on one and the same
 * device (profiles/r1/placement_tiers.txt), presumably by how their physical pages spread over the HBM stacks.  This
 * call writes the current observations into `obs` `reps` times and returns the average duration, so that a caller
 * that owns a pool of candidate buffers can keep the well-placed ones (VecPogema(reuse_buffers=True) does).
 * Synchronises `stream`.  Nothing in the engine's state changes. */
int pgx_time_observe(pgx_env* env, void* obs, int32_t reps, float* microseconds, void* stream);
/* The same into `obs` and `obs_alt` in turn -- how a caller with two alternating output buffers writes.  Two buffers that
 * together exceed the 256 MiB Infinity Cache behave differently from one buffer that fits it. */
int pgx_time_observe_pair(pgx_env* env, void* obs, void* obs_alt, int32_t reps, float* microseconds, void* stream);

/* ---- zone-aware output buffers ------------------------------------------------------------------ */
/* Nothing in the reference corresponds to this: it is where the caller-owned observation buffers SHOULD live on an
 * MI355X.  Physical HBM falls into a few large zones (tens of GiB; three on the devices measured).  A store stream
 * confined to one zone sustains ~5.5 TB/s, the same stream with half of its bytes in another zone ~6.9 TB/s
 * (profiles/r2/placement_*.txt); a plain hipMalloc'd buffer is physically compact and therefore lies in one zone
 * unless it straddles a boundary by luck.  pgx_buffers_create returns `count` buffers of `bytes` bytes, each ONE
 * contiguous virtual range (HIP virtual-memory API) whose second half is backed by physical memory from another zone:
 * the allocator is walked there with temporary spacer allocations (at most `max_spacer_gib` GiB and 90 % of the free
 * memory, released before the call returns) and every candidate is verified by timing a store stream into the buffer.
 * Buffers below 128 MiB are returned without a walk.  The walk assumes that the allocator hands out memory roughly in
 * address order (true for a process that has not fragmented its HBM); when it finds nothing, the buffers are valid but
 * not spread and `spread` says so.  The call blocks the calling thread for ~0.1-2 s (it times kernels on a private
 * non-blocking stream; work the caller has in flight on the device perturbs the timings, so callers synchronise first).
 * WHILE IT RUNS, up to min(max_spacer_gib, 90 % of the free memory) of HBM is held: on a device shared with other
 * processes pass a budget that leaves them room (the Python host defaults to half of the free memory).
 *   max_spacer_gib <= 0  no search: the halves come from wherever the allocator is (still valid buffers)
 * Buffers are usable by any kernel / copy like hipMalloc'd memory and stay valid until pgx_buffers_destroy. */
typedef struct pgx_buffers pgx_buffers; /* opaque */
typedef struct pgx_buffers_info {
    int64_t bytes;        /* usable bytes per buffer                                                         */
    int32_t count;
    int32_t spread;       /* 1: the two halves of every buffer lie in different zones (verified by timing)   */
    int32_t candidates;   /* second-half candidates timed                                                    */
    int32_t reserved0;
    float same_zone_us;   /* probe stream (768 MiB) into two halves allocated back to back (same zone)       */
    float final_us;       /* probe stream with the second half taken where the buffers' second halves are      */
    double spacer_gib;    /* spacer memory held at the end of the search (released before returning)          */
    float buffer_gbs;     /* store-stream rate into the slowest buffer as returned (0 below 128 MiB: no walk --  */
                          /* such a stream is absorbed by the Infinity Cache and says nothing about placement)  */
    float reserved1;
} pgx_buffers_info;
int pgx_buffers_create(int device, size_t bytes, int count, double max_spacer_gib, pgx_buffers** out);
/* The same, with the first `skip_gib` of the walk passed over unprobed: for a caller whose own stream turned out slower
 * into the buffers of a first pool than its probe promised (the fast stretch was narrower than the buffers) and who
 * tries again further on (`info.spacer_gib` of the first pool + 16, say). */
int pgx_buffers_create_at(int device, size_t bytes, int count, double skip_gib, double max_spacer_gib, pgx_buffers** out);
void* pgx_buffers_ptr(pgx_buffers* pool, int index); /* device pointer of buffer `index`, NULL if out of range */
int64_t pgx_buffers_stride(pgx_buffers* pool);       /* all buffers lie in ONE virtual range: ptr(i) = ptr(0) + i * stride,
                                                        stride = bytes rounded up to 2 MiB (pgx_rollout_io.obs_slot_stride) */
int pgx_buffers_drop(pgx_buffers* pool, int index);  /* releases the memory of ONE buffer (its addresses stay reserved and
                                                        must not be touched again): a caller may ask for more buffers
                                                        than it needs, time its own stream into each and keep the best */
int pgx_buffers_get_info(pgx_buffers* pool, pgx_buffers_info* info);
int pgx_buffers_destroy(pgx_buffers* pool);          /* synchronises the device, then unmaps and frees        */
/* Address space (bytes) this process has reserved for pool buffers so far.  These ranges are never handed back to the
 * driver nor re-used (ROCm 7.2 keeps stale translations either way: DESIGN.md section 6, profiles/r3/vmm_va_remap_stale.txt),
 * so the figure grows by count x stride with every pool -- out of 128 TiB; a caller that builds pools in a loop can
 * watch it here.  The probe chunks of the zone walk are plain hipMalloc memory and do not count. */
int64_t pgx_buffers_va_reserved(void);

/* ---- numpy-compatible random primitives ----------------------------------------------------------- */
/* Upstream POGEMA draws everything random from numpy Generators (np.random.default_rng(seed): SeedSequence -> PCG64 ->
 * integers / choice / shuffle / binomial / random; pogema/generator.py and the per-agent generators of PogemaLifeLong).
 * The engine's own generator and lifelong streams are counter-based and different (docs/SPEC.md S5, S6); these entry
 * points provide the numpy PRIMITIVES bit for bit -- pinned against numpy itself (tests/golden/numpy_rng_vectors.npz,
 * tests/test_nprng*.py) -- so that a numpy-stream mode can follow the upstream call sequence once the source is at hand
 * (pgx_config.lifelong_rng = PGX_LIFELONG_RNG_NUMPY already uses them for the lifelong target draw).
 * `streams` independent generators default_rng(seeds[s]) are each advanced `draws` times:
 *   PGX_NP_UINT64       raw 64-bit outputs (bit_generator.random_raw)          out u64 [streams, draws]
 *   PGX_NP_RANDOM       Generator.random()                                     out f64 [streams, draws]
 *   PGX_NP_INTEGERS     Generator.integers(0, n) = Generator.choice(n)         out i64 [streams, draws]
 *   PGX_NP_BINOMIAL1    Generator.binomial(1, p)  (generate_obstacles)         out i64 [streams, draws]
 *   PGX_NP_PERMUTATION  Generator.permutation(draws) = shuffle(arange(draws))  out i64 [streams, draws]
 * pgx_np_streams: device pointers, one GPU thread per stream, asynchronous on `stream`; pgx_np_streams_host: the same
 * arithmetic on the host (host pointers). */
#define PGX_NP_UINT64 0
#define PGX_NP_RANDOM 1
#define PGX_NP_INTEGERS 2
#define PGX_NP_BINOMIAL1 3
#define PGX_NP_PERMUTATION 4
int pgx_np_streams(const uint64_t* seeds, int64_t streams, int32_t op, uint64_t n, double p, int64_t draws, void* out,
                   void* stream);
int pgx_np_streams_host(const uint64_t* seeds, int64_t streams, int32_t op, uint64_t n, double p, int64_t draws, void* out);

/* Instances drawn the way upstream draws them (pogema/generator.py `generate_obstacles` +
 * `generate_positions_and_targets_fast` / `placing`, RECALLED, conf. medium): obstacles =
 * default_rng(seed).binomial(1, density, (H, W)); the free cells, row-major, shuffled with default_rng(seed); every cell
 * linked to the next cell of its 4-connected component in that order; walking the order, a linked cell becomes a start
 * and its link the target; the first `num_agents` pairs are the agents.  Env b uses seeds[b].  With the recollection
 * right these are upstream's instances for that seed; the numpy arithmetic itself is exact.  Outputs are in the format
 * pgx_reset_from_state takes.  `given_map` (u8 [H*W], non-zero = obstacle; may be NULL) replaces the obstacle draw for
 * every env, as GridConfig.map does upstream.  status[b] = 1 when env b has fewer than `num_agents` pairs (upstream: OverflowError).
 *   pgx_np_generate       device pointers; one GPU thread per env; scratch u32 [batch * 4 * H * W]; asynchronous
 *   pgx_np_generate_host  host pointers; scratch u32 [4 * H * W] */
int pgx_np_generate(const uint64_t* seeds, int32_t batch, int32_t height, int32_t width, int32_t num_agents, double density,
                    const uint8_t* given_map, uint8_t* obstacles, int32_t* agent_xy, int32_t* target_xy, uint32_t* scratch, int32_t* status, void* stream);
int pgx_np_generate_host(const uint64_t* seeds, int32_t batch, int32_t height, int32_t width, int32_t num_agents, double density,
                         const uint8_t* given_map, uint8_t* obstacles, int32_t* agent_xy, int32_t* target_xy, uint32_t* scratch, int32_t* status);

/* ---- state export ------------------------------------------------------------------------------- */
/* Replaces `Grid.get_agents_xy` / `get_targets_xy` / `is_active` / the occupancy array (`positions`).
 * Any pointer may be NULL.  All device pointers.
 *   agent_xy, target_xy  i32 [batch, agents, 2] unpadded
 *   is_active            u8  [batch, agents]
 *   elapsed              i32 [batch]                        steps since the env's last reset
 *   occupancy            u8  [batch, height+2r, width+2r]   padded occupancy array */
int pgx_get_state(pgx_env* env, int32_t* agent_xy, int32_t* target_xy, uint8_t* is_active,
                  int32_t* elapsed, uint8_t* occupancy, void* stream);

/* ---- snapshot / restore -------------------------------------------------------------------------- */
/* The complete engine state (maps, bitmaps, agent/target cells, initial state, active flags, step counters, metric
 * accumulators, generation counters, lifelong tables and draw counters) as one opaque device blob of
 * pgx_snapshot_bytes() bytes.  Replaces `PersistentWrapper`'s per-step state history / `step_back` (upstream
 * pogema/wrappers/persistence.py) and gives checkpoint-resume: a loaded snapshot continues bit-identically.
 * The blob is only valid for a handle of the same configuration; the 64-byte header records ABI version, batch,
 * agents, map height/width, obs_radius, on_target, collision_system, max_episode_steps and the total byte count, and
 * pgx_load_snapshot refuses (PGX_E_INVALID) a blob whose header differs from the loading handle's in any of them.
 * Both calls synchronise `stream` once for the header; the payload copies are asynchronous. */
int64_t pgx_snapshot_bytes(pgx_env* env);
int pgx_save_snapshot(pgx_env* env, void* blob, void* stream);
int pgx_load_snapshot(pgx_env* env, const void* blob, void* stream);

/* ---- environment copies (docs/SPEC.md S19) -------------------------------------------------------- */
/* Branching on the device: for every pair k < count, environment dst[k] becomes a copy of environment src[k] as it
 * stood before the call -- agent and target cells, the auto-reset state, the active and ghost bits, the step counter,
 * the metric accumulators, the map (u8 and padded bitmap, the `empty_outside=False` bits included), under
 * on_target = restart the draw counters, the numpy generators and the component tables, and with a map pool the pool
 * index.  What belongs to the SLOT stays: the generation counter (a later regenerate / masked reset of dst[k] draws
 * what that slot would have drawn next) and the global env index every counter-based stream is keyed on (the default
 * lifelong stream, the random policy of pgx_rollout): the copy draws what env dst[k] draws at the copied counters.
 *   src, dst  device i32 [count].  One source may feed many destinations; src[k] == dst[k] is a no-op.  A pair with an
 *             index outside 0..batch-1 is skipped: nothing is read or written out of range.  Not supported (the result
 *             is unspecified for the envs involved, every other env is untouched): a destination given twice, and an
 *             env that is the destination of one pair and the source of another (no permutations, no swaps).
 *   flags     0, or PGX_COPY_NO_CACHE: leave the distance-field cache alone.  By default, when the cache is allocated,
 *             the pairs' rows of it (tags, map bits, fields) are copied too, so that queries after a branch build
 *             nothing; without them the next refresh rebuilds what no longer matches.  Results are the same either
 *             way, only pgx_cost_to_go_builds differs.  The call never allocates the cache.
 * Rows of map-sized arrays are skipped for a pair whose two envs already hold equal maps (a compare pass decides per
 * pair), so a branch inside one map moves ~17 bytes per agent.  Two kernel launches, three with the cache; allocates
 * nothing, asynchronous on `stream`, no host sync, capturable in a HIP graph.  Caller-owned outputs (observations,
 * metrics, episode_done) are not touched: the next pgx_step / pgx_observe shows the copied state.
 * PGX_E_INVALID, checked before the handle (no device needed), for a negative count, a NULL src or dst with count > 0,
 * unknown flag bits and a NULL env; PGX_E_STATE before the first reset.  count == 0: PGX_OK, nothing is launched. */
#define PGX_COPY_NO_CACHE 1
int pgx_copy_envs(pgx_env* env, const int32_t* src, const int32_t* dst, int32_t count, int32_t flags, void* stream);

/* ---- host-side synthetic map generator ------------------------------------------------------------ */
/* Fills host buffers with `batch` random solvable instances: Bernoulli(density) obstacles, starts and
 * targets on distinct free cells with each start/target pair in one 4-connected component.
 * Plays the role of upstream pogema/generator.py at reset; the random stream is this
 * build's own (numpy's PCG64 sequence is not reproduced -- DESIGN.md).  Env i draws instance
 * (seed0, env_index_base + i) -- the same one pgx_reset_random draws for that seed and global index.
 *   obstacles host u8 [batch, height, width]; agent_xy / target_xy host i32 [batch, agents, 2]
 * nthreads <= 0 picks the number of online cores.  Returns PGX_E_PLACEMENT if an env cannot be
 * filled after `max_retries` re-draws. */
int pgx_generate(int32_t batch, int32_t height, int32_t width, int32_t num_agents, float density,
                 uint64_t seed0, int64_t env_index_base, int32_t max_retries, int32_t nthreads,
                 uint8_t* obstacles, int32_t* agent_xy, int32_t* target_xy);

/* Same placement on GIVEN obstacle maps (custom `GridConfig.map`): only starts/targets are drawn.
 *   obstacles host u8 [batch, height, width], or [height, width] when shared_map != 0. */
int pgx_place_agents(int32_t batch, int32_t height, int32_t width, int32_t num_agents, uint64_t seed0,
                     int64_t env_index_base, int32_t max_retries, int32_t nthreads, const uint8_t* obstacles,
                     int32_t shared_map, int32_t* agent_xy, int32_t* target_xy);

#ifdef __cplusplus
}
#endif
#endif /* POGEMA_AMD_H */
