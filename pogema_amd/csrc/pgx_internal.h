// pgx_internal.h -- shared by the library's translation units: device code + launchers (pgx_*.hip), the C-ABI
// (pgx_api.cpp) and the host generator (pgx_generate.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pgx {

// ---- host side of the C-ABI translation units ----
// formats the message pgx_last_error() returns and passes `code` through (pgx_api.cpp)
int fail_msg(int code, const char* fmt, ...);

// makes `call` (a hipError_t expression) the entry point's result when it fails (PGX_E_HIP: include/pogema_amd.h)
#define PGX_HIP(call)                                                                                                      \
    do {                                                                                                                   \
        const hipError_t e__ = (call);                                                                                     \
        if (e__ != hipSuccess)                                                                                             \
            return pgx::fail_msg(PGX_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

// selects a device for the rest of the scope and restores the caller's on exit
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    hipError_t err = hipSuccess;
    DeviceGuard() = default;
    explicit DeviceGuard(int dev) { (void)select(dev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
    hipError_t select(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            changed = (err == hipSuccess);
        }
        return err;
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};

enum { MODE_STEP = 0, MODE_OBSERVE = 1 };
enum { COLLISION_PRIORITY = 0, COLLISION_BLOCK_BOTH = 1, COLLISION_SOFT = 2 };
enum { ON_TARGET_FINISH = 0, ON_TARGET_RESTART = 1, ON_TARGET_NOTHING = 2 };
// the per-agent `active` byte: bit 0 = `Grid.is_active`; bit 1 = the agent stands on its cell but is MISSING from the
// occupancy array (`Grid.positions`) -- the quirk of the literal `move_without_checks` loop (docs/SPEC.md Q2), see step_body
enum : uint32_t { ACTIVE_BIT = 1u, ACTIVE_GHOST = 2u };

// ---- instance generator "GEN v2" constants shared by the host generator and the device kernels ----
constexpr uint64_t GEN_TAG_OBST = 0x4F42535400000000ull;   // 'OBST'
constexpr uint64_t GEN_TAG_PLACE = 0x504C414300000000ull;  // 'PLAC'
constexpr uint64_t GEN_TAG_POOL = 0x504F4F4C00000000ull;   // 'POOL': the map of a pool an env runs (docs/SPEC.md S10)
inline uint32_t gen_density_threshold(float density) {      // obstacle <=> 24 hash bits < thr
    double t = (double)density * 16777216.0 + 0.5;
    if (t < 0.0) t = 0.0;
    if (t > 16777216.0) t = 16777216.0;
    return (uint32_t)t;
}
__host__ __device__ inline uint32_t gen_candidate_budget(uint32_t cells) { return 32u * cells + 64u; }

// `empty_outside=False`: obstacles beyond the border ring, a pure function of (seed, global env, generation, cell)
constexpr uint64_t GEN_TAG_OUTSIDE = 0x4F55545300000000ull;  // 'OUTS'
struct OutsideParams {
    int32_t enabled;
    uint32_t thr;            // obstacle <=> 24 hash bits < thr
    uint64_t seed;
    int64_t env_index_base;
    const uint32_t* epoch;   // [B] generation counters
};
// splitmix64: the one hash of every counter-based stream of the library (instances, lifelong targets, random policy)
__host__ __device__ __forceinline__ uint64_t gen_sm64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the key of one generator attempt; host (pgx_generate) and device (pgx_reset_random) must draw the same instances.
// Seed and global env index are separate key components: adjacent seeds share no instance.
__host__ __device__ __forceinline__ uint64_t gen_instance_hash(uint64_t seed, uint64_t env, uint32_t epoch, uint32_t attempt) {
    return gen_sm64(gen_sm64(gen_sm64(seed) ^ env) ^ (((uint64_t)epoch << 32) | attempt));
}
// is padded cell (x, y) beyond the ring? (the ring itself and the map interior are never "outside")
__host__ __device__ inline bool gen_is_outside(int x, int y, int PH, int PW, int r) {
    return x < r - 1 || x > PH - r || y < r - 1 || y > PW - r;
}
__host__ __device__ inline uint64_t gen_outside_hash(uint64_t seed, uint64_t env_global, uint32_t epoch) {
    return gen_sm64(gen_sm64(gen_sm64(seed) ^ env_global) ^ (GEN_TAG_OUTSIDE | epoch));
}
__host__ __device__ inline uint32_t gen_outside_bit(uint64_t h, int x, int y, int PW, uint32_t thr) {
    return (gen_sm64(h ^ (uint64_t)(x * PW + y)) >> 40) < thr ? 1u : 0u;
}

// One numpy Generator (PCG64) per agent, lifelong_rng = NUMPY: {state hi, state lo, inc hi, inc lo, has_uint32 << 32 | uinteger}
struct NpGen {
    uint64_t w[5];
};

// Kernel argument block of the step kernel (passed by value: lands in SGPRs / kernarg segment).
struct StepParams {
    // geometry
    int32_t batch, num_agents, r;
    int32_t wpr;       // 32-bit words per padded bitmap row
    int32_t bm_words;  // words per env bitmap = (H + 2r) * wpr
    int32_t map_w;     // unpadded width
    int32_t map_cells; // unpadded H * W
    uint32_t w_magic;  // ceil(2^32 / (2r+1)): exact division of flat window offsets by the window side
    uint32_t a_magic;  // ceil(2^32 / num_agents): agent slot -> environment of the wave (slots < 4096)
    // behaviour
    int32_t mode, collision, on_target, max_steps, auto_reset, action_dtype;
    int32_t epw;       // environments per wave (single-wave blocks, num_agents <= 64)
    int32_t obs_u8;    // 1: `obs` is uint8 (one byte per cell) instead of float32
    uint32_t obs_one;  // != 0: `obs` is a 16-bit float format and this is its bit pattern of 1.0 (bfloat16 0x3F80, float16 0x3C00)
    int32_t stagger;   // cohort stagger of the single-wave kernel (StepGeometry::stagger)
    int32_t store_policy;  // observation stores: 0 plain, 1 nontemporal, 2 sc1 write-through (StepGeometry::store_policy)
    int32_t state_stores;  // when the small per-step result stores are issued: 0 at once, 1 after the LDS barrier, 2 after the stream
    int32_t soft_rule;    // PGX_SOFT_*  (docs/SPEC.md Q1)
    int32_t soft_occupancy;  // PGX_SOFT_OCCUPANCY_* (Q2; 0 = the literal index-order loop)
    int32_t coop_reward;  // PGX_COOP_REWARD_* (Q4)
    int32_t bad_action;   // PGX_BAD_ACTION_* (Q7)
    int32_t xcd_n[8];     // workgroups (= environment slices) given to each XCD, proportional to its measured store rate
    int32_t xcd_base[8];  // first slice of each XCD (prefix sums of xcd_n): the slices of one XCD stay contiguous
    uint32_t flags;    // diagnostic switches (PGX_FLAGS env var at pgx_create): bit1 generic row path, bit2 time stamps, bit3 identity block mapping
    uint64_t seed;
    int64_t env_index_base;
    // SoA state in HBM
    const uint32_t* obst;  // [B][bm_words]   padded obstacle bitmap, 1 bit per cell
    uint32_t* pos;         // [B][A]          (x << 16) | y, padded coordinates
    uint32_t* tgt;         // [B][A]
    uint8_t* active;       // [B][A]          ACTIVE_BIT | ACTIVE_GHOST
    int32_t* elapsed;      // [B]
    const uint32_t* pos0;  // [B][A]          auto-reset state
    const uint32_t* tgt0;  // [B][A]
    // lifelong (on_target = restart) tables, unpadded cell index = x * map_w + y
    const uint32_t* comp_begin;  // [B][H*W]  offset of the cell's component inside comp_cells
    const uint32_t* comp_len;    // [B][H*W]  size of the cell's component
    const uint32_t* comp_cells;  // [B][H*W]  unpadded packed cells grouped by component, row-major inside
    uint32_t* tcount;            // [B][A]    targets drawn so far
    NpGen* np_state;             // [B][A]    lifelong_rng = NUMPY: the agents' generators (null otherwise)
    const NpGen* np_state0;      // [B][A]    ... as they are right after a reset of the env
    // metric accumulators (pogema/wrappers/metrics.py): {agents solved, sum of solve steps, max solve step, lifelong goals}
    int4* macc;                  // [B]
    float* metrics_out;          // [B][6] ISR, CSR, ep_length, SoC, makespan, avg_throughput (caller-owned, may be null)
    uint8_t* episode_done;       // [B]    1 when the env's episode finished in this step            (may be null)
    uint32_t* bad_count;         // [1]    out-of-range actions of active agents (bad_action = FLAG)
    // I/O (caller-owned device buffers)
    const void* actions;
    float* obs;
    float* rewards;
    uint8_t* terminated;
    uint8_t* truncated;
    uint8_t* act_out;
    const uint8_t* only;      // MODE_OBSERVE: write only workgroups holding a flagged env (may be null)
    unsigned long long* dbg;  // diagnostic (PGX_FLAGS bit2): per-workgroup {start, resolve done, first store, end} clocks
};

// step_held (pgx_step_held): what the output set still holds, the kernel's second argument
struct HeldParams {
    uint8_t* held;     // [B][A]  flat window index of the 1.0 in the agent's target plane of `obs` (255: unknown); read and rewritten
    int32_t refresh;   // 1: `obs` is not vouched for -- write everything, record the indices
    int32_t lds_word;  // where the skip bitmap starts in LDS (32-bit words; behind the step kernel's own layout)
    int32_t words;     // its size
};

// pgx_rollout: what changes from one step of the launch to the next
struct RolloutParams {
    int32_t steps;
    int32_t obs_slots;        // step t writes observation slot t % obs_slots
    int32_t resident_bitmap;  // 1: the obstacle bitmap is staged once and keeps its own LDS region (StepGeometry::resident_bitmap)
    int32_t reserved0;
    int64_t actions_stride;   // bytes between the action tensors of consecutive steps
    int64_t agents_stride;    // batch * num_agents: elements between per-agent outputs of consecutive steps
    int64_t envs_stride;      // batch: elements between per-env outputs of consecutive steps
    int64_t obs_stride;       // bytes between observation slots
    uint64_t policy_seed;     // actions == NULL: uniform random policy keyed by (policy_seed, global env, agent, policy_step0 + t)
    int64_t policy_step0;
    int8_t* actions_out;      // [steps, batch, agents] the policy's actions (may be null)
};

// How one configuration maps onto the step kernel (pgx_kernels.hip: step_geometry()).
struct StepGeometry {
    int G;            // lanes per environment group (power of two, 64 when multi_wave)
    int waves;        // waves per workgroup: 1, ceil(A / 64) when num_agents > 64, or 2..8 helper waves (small launches)
    int epw;          // environments per wave (1 when multi_wave)
    bool multi_wave;  // num_agents > 64: one environment per workgroup
    bool p16;         // window side <= 16: packed 16-bit row masks aliased over the LDS state
    int stagger;      // > 0: odd wave slots sleep this many x 8128 cycles after issuing their loads
    int store_policy; // observation store flavour (pgx_kernels.hip: store_obs16)
    int state_stores; // when the per-step result stores are issued (pgx_kernels.hip: emit_state)
    bool big;         // large-map layout: one env per workgroup, occupancy bitmap only in LDS, obstacles read through the L2
    bool pc;          // rollout launch shape only: resolver / streamer pair of waves per environment group (step_body, PC)
    bool resident_bitmap;  // rollout launch shape only: obstacle bitmap staged once per launch, LDS = bitmap + max(rest, rows)
    size_t lds_bytes;
    // shares of the launch's workgroups per XCD (xcd_partition; equal until pgx_xcd_tune or PGX_XCD_WEIGHTS)
    int grid;             // workgroups to launch: 8 * the largest share
    int32_t xcd_n[8], xcd_base[8];
};
StepGeometry step_geometry(int batch, int A, int bmw, int W, bool allow_p16, int epw_override, int obs_elem_bytes,
                           int waves_override, bool for_rollout = false);
hipError_t prepare_step(const StepGeometry& g, const StepGeometry& roll);
// the > 48 KB dynamic-LDS opt-in of kernel `fn` on the current device: only ever raised, never lowered (an attribute of
// the function, shared by every live handle; pgx_kernels.hip)
hipError_t raise_lds_limit(const void* fn, size_t lds_bytes);
hipError_t launch_step(const StepParams& p, const StepGeometry& g, hipStream_t stream);
// the held form of launch_step (pgx_kernels.hip: step_held): whether launch shape `g` has one, its LDS opt-in (once per
// handle), the launch
bool held_available(const StepGeometry& g, int A, int W, int obs_elem_bytes);
hipError_t prepare_step_held(const StepGeometry& g, int A, int W);
hipError_t launch_step_held(const StepParams& p, const StepGeometry& g, uint8_t* held, bool refresh, hipStream_t stream);
// splits `blocks` workgroups over the XCDs by `w`; returns the grid size (8 * the largest share)
int xcd_partition(int blocks, const float w[8], int32_t n[8], int32_t base[8]);
hipError_t launch_rollout(const StepParams& p, const RolloutParams& rp, const StepGeometry& g, hipStream_t stream);

// `only` (device u8 [batch], may be null): pack just the flagged environments
hipError_t launch_pack_obstacles(const uint8_t* obstacles, const uint8_t* only, uint32_t* bm, int batch, int H, int Wd,
                                 int r, int wpr, int bmw, const OutsideParams& outside, hipStream_t stream);

// ---- on-device reset (pgx_reset.hip) ----------------------------------------------------------------
// Kernel argument block of reset_env_kernel: one workgroup per environment of [env_begin, env_begin + env_count),
// scratch slot = workgroup index.
struct ResetParams {
    int32_t env_begin, env_count;
    int32_t H, Wd, A, r, wpr, bmw;
    int32_t lifelong;      // build the component tables (on_target = restart)
    int32_t given_state;   // map already installed (pgx_reset_from_state): components + tables only
    int32_t max_retries;
    uint32_t thr;          // obstacle <=> 24 hash bits < thr
    uint64_t gen_seed;     // env i of the shard draws instance (gen_seed, env_index_base + i)
    int64_t env_index_base;
    const uint8_t* shared_map;  // [H*W] given map for every env, or null
    uint8_t* todo;              // [B] in: envs to build; cleared on success
    const uint32_t* epoch;      // [B] generation counters
    uint8_t* scratch_map;       // [slots][H*W] draft maps
    uint32_t* labels;           // [slots][H*W]
    uint32_t* pending;          // [slots][H*W]
    uint8_t* map_u8;            // [B][H*W] installed maps
    uint32_t* obst_bm;          // [B][bmw] padded bitmaps
    uint32_t *pos, *tgt, *pos0, *tgt0;
    uint8_t* active;
    uint32_t* tcount;           // may be null
    NpGen* np_state;            // may be null (lifelong_rng = NUMPY)
    const NpGen* np_state0;
    int32_t* elapsed;
    int4* macc;
    uint32_t *comp_begin, *comp_len, *comp_cells;  // lifelong only
    uint32_t* fail_count;       // envs that could not be filled
    OutsideParams outside;      // `empty_outside=False`
    // map pool (launch_reset_pool only; scratch_map and labels unused there)
    int32_t pool_size;            // M
    const uint8_t* pool_maps;     // [M][H*W] 0/1
    const uint32_t* pool_labels;  // [M][H*W] min-index component labels of the pool maps
    int32_t* map_index;           // [B] pool index of the map each env runs
};
hipError_t launch_reset_begin(const uint8_t* mask, uint8_t* todo, uint8_t* regen, uint32_t* epoch, int batch,
                              hipStream_t s);
hipError_t launch_reset_env(const ResetParams& p, hipStream_t s);
// map pool: env e of the launch runs pool map k = ((sm64(instance_hash(seed, base + e, epoch, 0) ^ 'POOL') >> 32) * M) >> 32
__host__ __device__ inline uint32_t gen_pool_pick(uint64_t h0, uint32_t num_maps) {
    return (uint32_t)(((gen_sm64(h0 ^ GEN_TAG_POOL) >> 32) * (uint64_t)num_maps) >> 32);
}
hipError_t launch_reset_pool(const ResetParams& p, hipStream_t s);
// normalises `count` maps of src into dst (0/1), labels their components and reduces each map's pair capacity
// (sum over components of floor(size / 2)) into cap; cnt = one scratch slot of H*W words per map of the launch
hipError_t launch_pool_label(const uint8_t* src, uint8_t* dst, uint32_t* labels, uint32_t* cnt, uint32_t* cap, int count,
                             int H, int Wd, hipStream_t s);
// map_index[b] = -1 for every env b a non-pool reset just rebuilt (regen[b] set, todo[b] cleared)
hipError_t launch_clear_map_index(const uint8_t* regen, const uint8_t* todo, int32_t* map_index, int batch, hipStream_t s);
hipError_t launch_pack_agents(const int32_t* agent_xy, const int32_t* target_xy, uint32_t* pos, uint32_t* tgt,
                              uint32_t* pos0, uint32_t* tgt0, uint8_t* active, uint32_t* tcount, size_t n,
                              int r, hipStream_t stream, NpGen* np_state = nullptr, const NpGen* np_state0 = nullptr);
// np_state0[env][a] = generator of agent a of global env (env_index_base + env) right after a reset (lifelong_rng = NUMPY)
hipError_t launch_init_np_lifelong(NpGen* np_state0, uint64_t seed, int64_t env_index_base, int batch, int A, hipStream_t stream);
hipError_t launch_zero_i32(int32_t* v, size_t n, hipStream_t stream);
hipError_t launch_set_targets(const int32_t* target_xy, const uint8_t* mask, uint32_t* tgt, size_t n, int r,
                              hipStream_t stream);
hipError_t launch_unpack_state(const uint32_t* pos, const uint32_t* tgt, const uint8_t* active, int32_t* agent_xy,
                               int32_t* target_xy, uint8_t* act_out, size_t n, int r, hipStream_t stream);
hipError_t launch_occupancy(const uint32_t* pos, const uint8_t* active, uint8_t* occ, size_t n, int A, int PH,
                            int PW, hipStream_t stream);

// ---- read-only queries on the engine state -----------------------------------------------------------------
// The picture of the state a query kernel works on (pgx_api.cpp: state_view()); the argument blocks of the expert,
// the cost-to-go cache and the planner start with it, the neighbour lists copy the four fields they read.
struct StateView {
    int32_t batch, A;        // environments, agents per environment
    int32_t H, W;            // unpadded map size
    int32_t r;               // observation radius = width of the padding ring
    int32_t wpr;             // 32-bit words per padded bitmap row
    int32_t bmw;             // words per env bitmap = (H + 2r) * wpr
    const uint32_t* obst;    // [B][bmw] padded obstacle bitmaps, 1 bit per cell
    const uint32_t* pos;     // [B][A] (x << 16) | y, padded coordinates
    const uint32_t* tgt;     // [B][A]
    const uint8_t* active;   // [B][A] ACTIVE_BIT | ACTIVE_GHOST
};

// ---- shortest-path expert (pgx_expert.hip) ------------------------------------------------------------
struct ExpertParams : StateView {
    int32_t with_agents;     // other active agents block their cells
    int32_t action_dtype;    // PGX_ACTION_*
    uint32_t* occ;           // [B][H][ceil(W/32)] occupancy scratch of the large layout (expert_occupancy_words)
    void* actions;           // [B][A] of action_dtype
    int32_t* distance;       // [B][A], may be null
};
bool expert_large_layout(int H, int W);
size_t expert_occupancy_words(int batch, int H, int W);
hipError_t prepare_expert(int H, int W);
hipError_t launch_expert(const ExpertParams& p, hipStream_t stream);

// ---- cost-to-go windows (pgx_cost2go.hip) --------------------------------------------------------------
// One device allocation per handle, made by the first pgx_cost_to_go: [16 B build counter][fields, padded to 16 B]
// [target tags][map bits].
struct CostToGoLayout {
    size_t cell_bytes;                       // 2 when H * W <= 65536, else 4
    size_t builds_off, field_off, tag_off, map_off, bytes;
};
CostToGoLayout cost_to_go_layout(int batch, int A, int H, int W);
struct CostToGoParams : StateView {
    int32_t cell_bytes;      // of `field`: CostToGoLayout::cell_bytes
    uint32_t* map_bits;      // [B][H][ceil(W/32)] free bits the env's fields were built on
    uint32_t* tag;           // [B][A] packed padded target each field was built for; all ones: no field
    void* field;             // [B][A][H*W] distance to the tag's cell, u16 or u32 (cell_bytes); all ones: unreachable
    unsigned long long* builds;  // [1] fields built since the cache was allocated
    int32_t* out;            // [B][A][2r+1][2r+1]
};
hipError_t prepare_cost_to_go(int H, int W);
// invalidate + build: every active agent's field is valid for its current target afterwards (`out` is not used)
hipError_t launch_cost_to_go_refresh(const CostToGoParams& p, hipStream_t stream);
// the refresh, then the gather of the windows into `out`
hipError_t launch_cost_to_go(const CostToGoParams& p, hipStream_t stream);

// ---- direction-to-goal planes (pgx_directions.hip) ---------------------------------------------------------
enum { DIRECTIONS_F32 = 0, DIRECTIONS_U8 = 1, DIRECTIONS_BITS = 2 };  // PGX_DIRECTIONS_* (include/pogema_amd.h)
// the refresh of the cost-to-go cache `p` describes (`p.out` is not used), then the planes of every agent into `out`:
// [B][A][4][2r+1][2r+1] float32 or u8, or [B][A][2r+1][2r+1] u8 masks
hipError_t launch_goal_directions(const CostToGoParams& p, void* out, int format, hipStream_t stream);

// ---- path-to-goal planes and sub-goals (pgx_goal_paths.hip, docs/SPEC.md S22) -------------------------------
enum { PATHS_F32 = 0, PATHS_U8 = 1, PATHS_ROWS = 2 };  // PGX_PATHS_* (include/pogema_amd.h)
struct GoalPathParams : CostToGoParams {   // `out` is not used
    int32_t format;          // PATHS_*: the elements of `planes`
    int32_t cap;             // most cells marked per agent, 1..(2r+1)^2 - 1: the walk's trip count, whatever a field holds
    void* planes;            // [B][A][2r+1][2r+1] float32 or u8, or [B][A][2r+1] i32 row masks; may be null
    int8_t* subgoal;         // [B][A][2] offset (dx, dy) of the last marked cell; may be null
    int32_t* length;         // [B][A] cells marked; may be null
};
// the refresh of the cost-to-go cache `p` describes, then the paths of every agent in one launch
hipError_t launch_goal_paths(const GoalPathParams& p, hipStream_t stream);

// ---- agent forecasts (pgx_agent_forecasts.hip, docs/SPEC.md S24) ---------------------------------------------
enum { FORECAST_F32 = 0, FORECAST_U8 = 1, FORECAST_ROWS = 2 };  // PGX_FORECAST_* (include/pogema_amd.h)
struct ForecastParams : CostToGoParams {   // `out` is not used
    int32_t format;          // FORECAST_*: the elements of `planes`
    int32_t steps;           // K, 1..PGX_MAX_FORECAST_STEPS: the walk's trip count, whatever a field holds
    void* planes;            // [B][A][K][2r+1][2r+1] float32 or u8, or [B][A][K][2r+1] i32 row masks; may be null
    int16_t* cells;          // [B][A][K][2] unpadded (x, y) after 1..K steps, -1 for an inactive agent; never null
};
// the refresh of the cost-to-go cache `p` describes, then every agent's walk into `cells` and, with `planes`, the
// gather of the visible agents' cells into every observer's planes: two launches
hipError_t launch_agent_forecasts(const ForecastParams& p, hipStream_t stream);

// ---- blocking counts (pgx_blocking.hip, docs/SPEC.md S25) -----------------------------------------------------
struct BlockingParams : CostToGoParams {   // `out` is not used
    int32_t inflation;       // 1..PGX_MAX_BLOCKING_INFLATION: a search runs at most d0 + inflation - 1 levels
    int32_t on_target;       // only agents standing on their own target block (PGX_BLOCKING_ON_TARGET)
    int32_t* count;          // [B][A] agents this one blocks; may be null
    int32_t* blocked_by;     // [B][A] agents that block this one; may be null
};
// the refresh of the cost-to-go cache `p` describes, then the counts (small layout: one launch; large: a zeroing launch
// of `count` and the search launch)
hipError_t launch_blocking(const BlockingParams& p, hipStream_t stream);

// ---- path conflicts (pgx_path_conflicts.hip, docs/SPEC.md S26) ------------------------------------------------
enum { CONFLICT_PATHS_PLAN = 0, CONFLICT_PATHS_CELLS = 1 };            // PGX_CONFLICT_PATHS_* (include/pogema_amd.h)
enum { CONFLICT_VERTEX = 1, CONFLICT_EDGE = 2, CONFLICT_FOLLOW = 4 };  // PGX_CONFLICT_VERTEX / _EDGE / _FOLLOW
struct ConflictParams : StateView {
    const void* paths;       // PLAN: i32 [K][B][A][2]; CELLS: i16 [B][A][K][2]; unpadded (x, y), any values
    int32_t layout;          // CONFLICT_PATHS_*
    int32_t steps;           // K, 1..PGX_MAX_CONFLICT_STEPS: the step loop's trip count
    int32_t kinds;           // the CONFLICT_* kinds that exist for this call, at least one
    int32_t vanish;          // an agent takes no part after a step on its target
    int32_t* first_step;     // [B][A] may be null
    int32_t* partner;        // [B][A] may be null
    uint8_t* kind;           // [B][A] may be null
    int32_t* count;          // [B][A] may be null
};
// one launch; reads the state and `paths`, writes the four outputs only
hipError_t launch_path_conflicts(const ConflictParams& p, hipStream_t stream);

// ---- agent tokens (pgx_agent_tokens.hip): one row of token ids per agent (docs/SPEC.md S21) -------------------------
struct TokenParams : CostToGoParams {   // `out` is not used
    int32_t slots;           // S, 1..PGX_MAX_TOKEN_SLOTS: the agent itself and S - 1 neighbours
    int32_t length;          // bytes per row, W * W + 10 * S .. PGX_MAX_TOKEN_LENGTH
    const int8_t* history;   // [B][A][5] recorded actions, most recent first; may be null
    uint8_t* tokens;         // [B][A][length]
};
// the refresh of the cost-to-go cache `p` describes, then the rows of every agent in one launch
hipError_t launch_agent_tokens(const TokenParams& p, hipStream_t stream);

// ---- policy input (pgx_policy_input.hip): the network's window planes, chosen, ordered and typed per call ------------
enum { POLICY_INPUT_F32 = 0, POLICY_INPUT_U8 = 1, POLICY_INPUT_BF16 = 2, POLICY_INPUT_F16 = 3 };  // PGX_OBS_* (include/pogema_amd.h)
enum { POLICY_CHANNELS = 8 };                                                                     // PGX_NUM_CHANNELS
struct PolicyInputParams : CostToGoParams {   // without a direction channel only the StateView part is used
    int32_t num_channels;    // C, 1..POLICY_CHANNELS
    int32_t dtype;           // POLICY_INPUT_*
    uint32_t codes;          // the channel list: PGX_CHANNEL_* of output plane c in bits 4c .. 4c+3
    uint32_t need;           // bit k set: channel code k is in the list
    uint32_t one;            // the bit pattern of 1 in `dtype`
    void* planes;            // [B][A][C][2r+1][2r+1] of `dtype`
};
// with a direction channel (need & 0xF0): the refresh of the cost-to-go cache `p` describes, then the planes; without
// one: the planes alone, in one launch that reads no field
hipError_t launch_policy_input(const PolicyInputParams& p, hipStream_t stream);

// ---- global state (pgx_global_state.hip): whole-map planes, chosen, ordered and typed per call -----------------------
enum { GLOBAL_CHANNELS = 5 };                 // PGX_NUM_GLOBAL_CHANNELS
enum { GLOBAL_BAND_CELLS = 8192 };            // PGX_GLOBAL_BAND_CELLS: the cells of the band of rows a workgroup holds in LDS
struct GlobalStateParams : StateView {
    int32_t num_channels;    // C, 1..GLOBAL_CHANNELS
    int32_t dtype;           // POLICY_INPUT_* (PGX_OBS_*)
    uint32_t codes;          // the channel list: PGX_GLOBAL_* of output plane c in bits 4c .. 4c+3
    uint32_t need;           // bit k set: channel code k is in the list
    uint32_t one;            // the bit pattern of 1 in `dtype`
    void* planes;            // [B][C][H][W] of `dtype`
};
hipError_t launch_global_state(const GlobalStateParams& p, hipStream_t stream);

// ---- neighbour lists (pgx_neighbours.hip) ---------------------------------------------------------------
// (not derived from StateView: the kernel reads four of its fields, and this block of 56 bytes is fetched with two loads)
struct NeighbourParams {
    int32_t batch, A, r;     // as in StateView
    int32_t k;               // entries per agent, 1..PGX_MAX_NEIGHBOURS
    const uint32_t* pos;     // as in StateView
    const uint8_t* active;
    int32_t* index;          // [B][A][k]
    int8_t* offset;          // [B][A][k][2], 2-byte aligned, may be null
    int32_t* count;          // [B][A], may be null
};
hipError_t launch_visible_agents(const NeighbourParams& p, hipStream_t stream);

// ---- cooperative planner (pgx_pibt.hip) ---------------------------------------------------------------------
struct PibtParams : StateView {
    int32_t action_dtype;    // PGX_ACTION_*
    int32_t cell_bytes;      // of `field`: CostToGoLayout::cell_bytes
    const void* field;       // [B][A][H*W] the refreshed distance fields of the cost-to-go cache
    const int32_t* priority; // [B][A], null: every priority is 0
    void* actions;           // [B][A] of action_dtype
    int32_t* next_xy;        // [B][A][2] unpadded, may be null
};
hipError_t launch_pibt(const PibtParams& p, hipStream_t stream);
// the planner with the swap operation (pgx_pibt_swap.hip, docs/SPEC.md S23): the same arguments, `tgt` is read too
enum { SWAP_MAX_WALK = 2048 };                // PGX_SWAP_MAX_WALK: steps of one corridor walk
hipError_t launch_pibt_swap(const PibtParams& p, hipStream_t stream);

// ---- multi-step planner (pgx_pibt_horizon.hip): the planner iterated over a horizon in one launch ----------------
struct PibtPlanParams : PibtParams {   // `actions` is [horizon][B][A]; `next_xy` is not used
    int32_t horizon;         // steps of the lookahead, 1..PGX_MAX_PLAN_HORIZON
    int32_t finish;          // on_target = finish: an agent that reaches its target is not planned any more
    int32_t fixed_priority;  // the priorities are held instead of grown (PGX_PLAN_FIXED_PRIORITY)
    int32_t* path_xy;        // [horizon][B][A][2] unpadded, may be null
    int32_t* arrival;        // [B][A], may be null
    int32_t* priority_out;   // [B][A], may be null
};
hipError_t launch_pibt_plan(const PibtPlanParams& p, hipStream_t stream);
// the same lookahead over the planner with the swap operation (pgx_pibt_swap_horizon.hip, docs/SPEC.md S27)
hipError_t launch_pibt_swap_plan(const PibtPlanParams& p, hipStream_t stream);

// ---- windowed cooperative A* (pgx_whca.hip, docs/SPEC.md S28): space-time paths against a reservation table ----------
struct WhcaParams : StateView {
    int32_t action_dtype;    // PGX_ACTION_*
    int32_t cell_bytes;      // of `field`: CostToGoLayout::cell_bytes
    int32_t horizon;         // K, 1..PGX_MAX_WHCA_HORIZON: the window of the search
    int32_t finish;          // on_target = finish: a search ends on the target, and the agent reserves nothing afterwards
    const void* field;       // [B][A][H*W] the refreshed distance fields of the cost-to-go cache
    const int32_t* priority; // [B][A], null: every priority is 0
    void* actions;           // [K][B][A] of action_dtype
    int32_t* path_xy;        // [K][B][A][2] unpadded, may be null
    int32_t* arrival;        // [B][A], may be null
    int32_t* failed;         // [B][A], may be null
};
hipError_t launch_whca(const WhcaParams& p, hipStream_t stream);
// the repair (pgx_whca.hip: the same kernel with its prologue, docs/SPEC.md S29): chosen agents are served around the
// given paths the others keep
struct RepairParams : WhcaParams {
    const int32_t* paths;    // [K][B][A][2] unpadded, any int32; may be `path_xy` itself
    const uint8_t* replan;   // [B][A], null: nobody is asked for
    int32_t* replanned;      // [B][A], may be null
};
size_t repair_lds_bytes(int A, int K);   // dynamic LDS of one workgroup
hipError_t launch_repair(const RepairParams& p, hipStream_t stream);

// ---- collision shielding (pgx_shield.hip): the planner over the caller's action scores ------------------------------
enum { SCORES_F32 = 0, SCORES_F16 = 1, SCORES_BF16 = 2 };  // PGX_SCORES_* (include/pogema_amd.h)
struct ShieldParams : PibtParams {   // `field` is null without `tie_distance`
    int32_t score_dtype;     // SCORES_*
    int32_t tie_distance;    // equal scores are ordered by the planner's key (PGX_SHIELD_TIE_DISTANCE)
    const void* scores;      // [B][A][5] of score_dtype
    uint8_t* overridden;     // [B][A], may be null
};
hipError_t launch_shield(const ShieldParams& p, hipStream_t stream);

// ---- move outcomes (pgx_outcomes.hip): the resolve phase of the step as a read-only query ---------------------------
struct OutcomeParams : StateView {
    int32_t collision;       // COLLISION_*
    int32_t all_stay;        // soft: every claimant of a contested cell stays (PGX_SOFT_ALL_STAY)
    int32_t action_dtype;    // PGX_ACTION_*
    const void* actions;     // [B][A] of action_dtype
    int32_t* next_xy;        // [B][A][2] unpadded, may be null
    uint8_t* outcome;        // [B][A] PGX_OUTCOME_*, may be null
    int32_t* blocker;        // [B][A], may be null
    int32_t* counts;         // [B][PGX_NUM_OUTCOMES], may be null
};
hipError_t launch_move_outcomes(const OutcomeParams& p, hipStream_t stream);

// ---- environment copies (pgx_copy.hip): rows of the per-env state arrays, slot to slot -------------------------------
constexpr size_t COPY_CHUNK_VECS = 1024;   // a slice of a large row is at least this many 16-byte pieces (16 KiB)
constexpr size_t COPY_TARGET_GROUPS = 8192;  // workgroups a call spreads one array's large rows over, all pairs together
constexpr size_t COPY_SMALL_ROW = 2048;    // rows up to this many bytes share the pair's first workgroup
enum { COPY_MAX_SEGS = 16 };
struct CopySeg {
    char* base;              // [B][row] bytes
    size_t row;
    uint32_t chunk0, nchunks;  // the workgroups of a pair that copy this row (copy_plan_chunks)
    int32_t of_map;          // a function of the env's map: left alone where source and destination hold equal maps
    int32_t reserved0;
};
struct CopyParams {
    const int32_t* src;      // [count] device
    const int32_t* dst;      // [count] device
    int32_t count, batch;
    int32_t pair0;           // first pair of this launch
    uint32_t chunks;         // workgroups per pair
    int32_t nseg;
    int32_t reserved0;
    CopySeg seg[COPY_MAX_SEGS];
};
// fills chunk0 / nchunks of every segment from its row size and the number of pairs; returns the workgroups per pair
uint32_t copy_plan_chunks(CopySeg* seg, int nseg, int count);
// same_map[dst[k]] = 1 iff the padded bitmaps (and, with `map_index`, the pool indices) of src[k] and dst[k] are equal
hipError_t launch_copy_compare(CopyParams p, const uint32_t* obst, int bmw, const int32_t* map_index, uint8_t* same_map,
                               hipStream_t stream);
// the rows of every pair; `same_map` (may be null) as launch_copy_compare left it
hipError_t launch_copy_rows(CopyParams p, const uint8_t* same_map, hipStream_t stream);

}  // namespace pgx
