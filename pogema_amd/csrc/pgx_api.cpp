// pgx_api.cpp -- C-ABI of the engine (include/pogema_amd.h): handle management, reset, step launch and
// state export (the host-side generator is pgx_generate.cpp).  Compiled with hipcc together with
// pgx_kernels.hip into libpogema_amd.so.  There is NO CPU fallback anywhere in this file: every
// compute entry point enqueues HIP kernels and fails with PGX_E_HIP when no device is usable.
#include "../../include/pogema_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pgx_internal.h"

namespace {
thread_local std::string g_err;
}  // namespace

namespace pgx {
int fail_msg(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace pgx

namespace {

using pgx::DeviceGuard;
using pgx::fail_msg;

// A device allocation owned by the handle: freed by reset() or with the handle (pgx_destroy, on the handle's device).
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    operator T*() const { return p; }
    hipError_t alloc(size_t bytes) {  // (stays null when it fails)
        reset();
        const hipError_t err = hipMalloc((void**)&p, bytes);
        if (err != hipSuccess) p = nullptr;
        return err;
    }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
};

int alloc_code(hipError_t err) { return err == hipErrorOutOfMemory ? PGX_E_NOMEM : PGX_E_HIP; }

// The allocation of `buf` (`bytes` of `what`) by the first call of entry point `who` that needs it, so that callers who
// never ask never pay for it.  PGX_E_STATE while `s` is capturing; the failed allocation must not surface as the next
// launch's error.
template <class T>
int alloc_on_first_use(DevBuf<T>& buf, size_t bytes, hipStream_t s, const char* who, const char* what) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    PGX_HIP(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail_msg(PGX_E_STATE, "%s: the first call allocates %zu bytes for %s; make it once outside graph capture",
                        who, bytes, what);
    const hipError_t err = buf.alloc(bytes);
    if (err == hipSuccess) return PGX_OK;
    (void)hipGetLastError();
    return fail_msg(alloc_code(err), "%s: %s of %zu bytes: %s", who, what, bytes, hipGetErrorString(err));
}

// The argument checks the entry points share: PGX_OK, or PGX_E_INVALID with a message naming `who` and the argument.
int check_aligned(const char* who, const char* name, const void* p, size_t n) {  // n: a power of two
    if (reinterpret_cast<uintptr_t>(p) & (n - 1)) return fail_msg(PGX_E_INVALID, "%s: %s is not %zu-byte aligned", who, name, n);
    return PGX_OK;
}
int check_action_dtype(const char* who, int32_t action_dtype) {
    if (action_dtype < 0 || action_dtype > 2) return fail_msg(PGX_E_INVALID, "%s: bad action_dtype %d", who, action_dtype);
    return PGX_OK;
}
int check_flags(const char* who, int32_t flags, int32_t known) {
    if (flags & ~known) return fail_msg(PGX_E_INVALID, known ? "%s: unknown flags 0x%x" : "%s: flags must be 0, got 0x%x", who, flags);
    return PGX_OK;
}

}  // namespace

struct pgx_env {
    pgx_config cfg{};
    int device = 0;
    pgx::StepGeometry geo{};       // launch shape of pgx_step / pgx_observe
    pgx::StepGeometry geo_roll{};  // ... of pgx_rollout
    int W = 0, PH = 0, PW = 0, wpr = 0, bmw = 0;
    bool has_state = false;
    uint32_t flags = 0;
    bool xcd_aware = true;  // false: not an 8-XCD SPX device -> identity workgroup mapping, no XCD shares, no cohort stagger
    // device state
    DevBuf<uint32_t> obst;
    DevBuf<uint32_t> pos, tgt, pos0, tgt0;
    DevBuf<uint8_t> active;
    DevBuf<int32_t> elapsed;
    DevBuf<int4> macc;
    float* metrics_out = nullptr;   // caller-owned (pgx_set_metrics_buffers)
    uint8_t* episode_done = nullptr; // caller-owned
    DevBuf<unsigned long long> dbg;
    size_t dbg_elems = 0;
    DevBuf<uint32_t> comp_begin, comp_len, comp_cells, tcount;
    DevBuf<pgx::NpGen> np_state, np_state0;  // lifelong_rng = NUMPY
    // reset path (pgx_reset.hip): unpadded u8 maps, per-env flags / generation counters, chunked scratch
    DevBuf<uint8_t> map_u8;               // [B][H*W]
    DevBuf<uint8_t> todo, regen;          // [B]
    DevBuf<uint32_t> epoch;               // [B]
    DevBuf<uint32_t> fail_count;          // [1]
    DevBuf<uint32_t> regen_fail;          // [1] sticky failure counter of pgx_regenerate
    DevBuf<uint32_t> bad_count;           // [1] out-of-range actions (bad_action = FLAG)
    float xcd_w[8] = {0.125f, 0.125f, 0.125f, 0.125f, 0.125f, 0.125f, 0.125f, 0.125f};  // shares of a launch per XCD
    DevBuf<uint32_t> expert_occ;          // [B][H][ceil(W/32)] occupancy bits of pgx_expert_actions' large-map layout
                                          // (allocated by its first call with agents as obstacles)
    DevBuf<uint32_t> labels, pending;     // [chunk_envs][H*W], allocated on first use
    DevBuf<uint8_t> scratch_map;          // [chunk_envs][H*W] draft maps (not allocated for pool-only resets)
    int chunk_envs = 0;
    // map pool (pgx_set_map_pool): 5 bytes per cell and pool map
    int pool_size = 0;                    // M (0: no pool installed)
    DevBuf<uint8_t> pool_maps;            // [M][H*W] 0/1
    DevBuf<uint32_t> pool_labels;         // [M][H*W] min-index component labels
    DevBuf<uint32_t> pool_cap;            // [M] start/target pairs each map can hold
    DevBuf<int32_t> map_index;            // [B] pool index of each env's map, -1 after a non-pool install
    // cost-to-go cache (docs/SPEC.md S11, pgx::cost_to_go_layout), allocated by the first pgx_cost_to_go,
    // pgx_pibt_actions, pgx_pibt_plan, pgx_goal_directions or pgx_policy_input with a direction channel
    DevBuf<uint8_t> c2g;
    DevBuf<uint8_t> copy_same;            // [B] pgx_copy_envs: 1 where the destination env already holds its source's map
};

namespace {

// The prologue of every entry point that works on the handle's device: `e` is non-null, holds a state when `need_state`,
// and its device stays selected while `guard` lives.  `who` names the entry point in the error message.
int enter(DeviceGuard& guard, const pgx_env* e, const char* who, bool need_state) {
    if (!e) return fail_msg(PGX_E_INVALID, "%s: null handle", who);
    if (need_state && !e->has_state) return fail_msg(PGX_E_STATE, "%s called before a reset", who);
    if (guard.select(e->device) != hipSuccess)
        return fail_msg(PGX_E_HIP, "%s: cannot select HIP device %d: %s", who, e->device, hipGetErrorString(guard.err));
    return PGX_OK;
}

int obs_elem_bytes(int obs_dtype) {
    return obs_dtype == PGX_OBS_U8 ? 1 : (obs_dtype == PGX_OBS_BF16 || obs_dtype == PGX_OBS_F16) ? 2 : 4;
}

// The launch parameters of the handle with launch shape `g` (e->geo: pgx_step / pgx_observe, e->geo_roll: pgx_rollout).
pgx::StepParams step_params(const pgx_env* e, const pgx::StepGeometry& g) {
    const pgx_config& c = e->cfg;
    pgx::StepParams p;
    memset(&p, 0, sizeof p);
    p.batch = c.batch;
    p.num_agents = c.num_agents;
    p.r = c.obs_radius;
    p.wpr = e->wpr;
    p.bm_words = e->bmw;
    p.map_w = c.width;
    p.map_cells = c.height * c.width;
    p.w_magic = (uint32_t)((1ull << 32) / (uint64_t)e->W) + 1u;
    p.a_magic = c.num_agents > 1 ? (uint32_t)((1ull << 32) / (uint64_t)c.num_agents) + 1u : 0u;  // 0: A = 1, slot = env
    p.collision = c.collision_system;
    p.on_target = c.on_target;
    p.max_steps = c.max_episode_steps;
    p.auto_reset = c.auto_reset;
    p.flags = e->flags;
    p.epw = g.epw;
    p.stagger = g.stagger;
    p.store_policy = g.store_policy;
    p.state_stores = g.state_stores;
    for (int x = 0; x < 8; ++x) {
        p.xcd_n[x] = g.xcd_n[x];
        p.xcd_base[x] = g.xcd_base[x];
    }
    p.obs_u8 = c.obs_dtype == PGX_OBS_U8 ? 1 : 0;
    p.obs_one = c.obs_dtype == PGX_OBS_BF16 ? 0x3F80u : c.obs_dtype == PGX_OBS_F16 ? 0x3C00u : 0u;
    p.soft_rule = c.soft_vertex_rule;
    p.soft_occupancy = c.soft_occupancy;
    p.coop_reward = c.coop_reward;
    p.bad_action = c.bad_action;
    p.bad_count = e->bad_count;
    p.seed = c.seed;
    p.env_index_base = c.env_index_base;
    p.obst = e->obst;
    p.pos = e->pos;
    p.tgt = e->tgt;
    p.active = e->active;
    p.elapsed = e->elapsed;
    p.pos0 = e->pos0;
    p.tgt0 = e->tgt0;
    p.comp_begin = e->comp_begin;
    p.comp_len = e->comp_len;
    p.comp_cells = e->comp_cells;
    p.tcount = e->tcount;
    p.np_state = e->np_state;
    p.np_state0 = e->np_state0;
    p.dbg = e->dbg;
    p.macc = e->macc;
    p.metrics_out = e->metrics_out;
    p.episode_done = e->episode_done;
    return p;
}

// an observation-only launch (MODE_OBSERVE) of pgx_step's launch shape into `obs`
pgx::StepParams observe_params(const pgx_env* e, void* obs) {
    pgx::StepParams p = step_params(e, e->geo);
    p.mode = pgx::MODE_OBSERVE;
    p.obs = static_cast<float*>(obs);
    return p;
}

// What the read-only queries see of the handle's state.
pgx::StateView state_view(const pgx_env* e) {
    const pgx_config& c = e->cfg;
    return {c.batch, c.num_agents, c.height, c.width, c.obs_radius, e->wpr, e->bmw, e->obst, e->pos, e->tgt, e->active};
}

// Mean time of one launch of `p` in us: `warmup` launches, then `timed` launches between an event pair; launch i of
// either phase writes obs[i & 1].  The events are released on every path.
hipError_t time_launches(pgx::StepParams p, const pgx::StepGeometry& g, void* const obs[2], int warmup, int timed,
                         hipStream_t s, float* us) {
    auto launch = [&](int i) {
        p.obs = static_cast<float*>(obs[i & 1]);
        return pgx::launch_step(p, g, s);
    };
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t err = hipEventCreate(&a);
    if (err == hipSuccess) err = hipEventCreate(&b);
    for (int i = 0; i < warmup && err == hipSuccess; ++i) err = launch(i);
    if (err == hipSuccess) err = hipEventRecord(a, s);
    for (int i = 0; i < timed && err == hipSuccess; ++i) err = launch(i);
    if (err == hipSuccess) err = hipEventRecord(b, s);
    if (err == hipSuccess) err = hipEventSynchronize(b);
    float ms = 0.0f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, a, b);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (err == hipSuccess) *us = ms * 1000.0f / (float)timed;
    return err;
}

}  // namespace

// ================================================================================================
extern "C" {

int pgx_abi_version(void) { return PGX_ABI_VERSION; }

const char* pgx_last_error(void) { return g_err.c_str(); }

// (re)computes both launch shapes' per-XCD shares from e->xcd_w
static void apply_xcd_shares(pgx_env* e) {
    for (pgx::StepGeometry* g : {&e->geo, &e->geo_roll}) {
        const int blocks = g->multi_wave ? e->cfg.batch : (e->cfg.batch + g->epw - 1) / g->epw;
        g->grid = pgx::xcd_partition(blocks, e->xcd_w, g->xcd_n, g->xcd_base);
        if (e->flags & 8u) g->grid = blocks;  // identity mapping (A/B)
    }
}

// Everything of pgx_create that needs no device: argument checks, launch shapes, the LDS budget.
static int create_host_side(const pgx_config* cfg, int device, pgx_env** out_e) {
    *out_e = nullptr;
    if (cfg->abi_version != PGX_ABI_VERSION)
        return fail_msg(PGX_E_INVALID, "pgx_config.abi_version is %d but this library implements ABI %d: rebuild the caller against "
                        "include/pogema_amd.h and set cfg.abi_version = PGX_ABI_VERSION (ABI 5 renumbered soft_occupancy: 0 is "
                        "the index-order loop, 1 the exact set; ABI <= 5 callers pass 0 in this field)", cfg->abi_version, PGX_ABI_VERSION);
    if (cfg->batch < 1) return fail_msg(PGX_E_INVALID, "batch must be >= 1 (got %d)", cfg->batch);
    if (cfg->height < 1 || cfg->width < 1 || cfg->height > PGX_MAX_SIDE || cfg->width > PGX_MAX_SIDE)
        return fail_msg(PGX_E_INVALID, "map size %dx%d outside [1, %d]", cfg->height, cfg->width, PGX_MAX_SIDE);
    if (cfg->num_agents < 1 || cfg->num_agents > PGX_MAX_AGENTS)
        return fail_msg(PGX_E_INVALID, "num_agents %d outside [1, %d]", cfg->num_agents, PGX_MAX_AGENTS);
    if (cfg->obs_radius < 1 || cfg->obs_radius > PGX_MAX_OBS_RADIUS)
        return fail_msg(PGX_E_INVALID, "obs_radius %d outside [1, %d] supported by this build", cfg->obs_radius,
                        PGX_MAX_OBS_RADIUS);
    if (cfg->collision_system < 0 || cfg->collision_system > 2)
        return fail_msg(PGX_E_INVALID, "unknown collision_system %d", cfg->collision_system);
    if (cfg->on_target < 0 || cfg->on_target > 2) return fail_msg(PGX_E_INVALID, "unknown on_target %d", cfg->on_target);
    if (cfg->random_outside && !(cfg->outside_density >= 0.0f && cfg->outside_density <= 1.0f))
        return fail_msg(PGX_E_INVALID, "outside_density %.3f outside [0, 1]", (double)cfg->outside_density);
    if (cfg->soft_vertex_rule < 0 || cfg->soft_vertex_rule > 1 || cfg->coop_reward < 0 || cfg->coop_reward > 1 ||
        cfg->bad_action < 0 || cfg->bad_action > 1 || cfg->lifelong_rng < 0 || cfg->lifelong_rng > 1 ||
        cfg->soft_occupancy < 0 || cfg->soft_occupancy > 1)
        return fail_msg(PGX_E_INVALID, "unknown semantics switch (soft_vertex_rule %d, coop_reward %d, bad_action %d, soft_occupancy %d)",
                        cfg->soft_vertex_rule, cfg->coop_reward, cfg->bad_action, cfg->soft_occupancy);
    if (cfg->obs_dtype < PGX_OBS_F32 || cfg->obs_dtype > PGX_OBS_F16)
        return fail_msg(PGX_E_INVALID, "unknown obs_dtype %d", cfg->obs_dtype);
    if ((int64_t)cfg->num_agents > (int64_t)cfg->height * cfg->width)
        return fail_msg(PGX_E_INVALID, "more agents than cells");

    pgx_env* e = new (std::nothrow) pgx_env();
    if (!e) return fail_msg(PGX_E_NOMEM, "out of host memory");
    e->cfg = *cfg;
    e->device = device;
    const int A = cfg->num_agents, r = cfg->obs_radius;
    e->W = 2 * r + 1;
    e->PH = cfg->height + 2 * r;
    e->PW = cfg->width + 2 * r;
    e->wpr = (e->PW + 31) / 32;
    e->bmw = e->PH * e->wpr;
    if (const char* f = getenv("PGX_FLAGS")) e->flags = (uint32_t)strtoul(f, nullptr, 0);
    int epw_override = 0;  // PGX_EPW: tuning/diagnostic override of the environments-per-wave heuristic
    if (const char* f = getenv("PGX_EPW")) epw_override = atoi(f);
    // PGX_FLAGS bit1: force the generic (32-bit row mask) observation path
    int waves_override = 0;  // PGX_WAVES: 1 = single-wave kernel for A <= 64 whatever the launch size, k = k helper waves
    if (const char* f = getenv("PGX_WAVES")) waves_override = atoi(f);
    e->geo = pgx::step_geometry(cfg->batch, A, e->bmw, e->W, !(e->flags & 2u), epw_override,
                                obs_elem_bytes(cfg->obs_dtype), waves_override);
    // pgx_rollout's launch shape: the same, minus the helper waves of large launches (step_geometry())
    e->geo_roll = pgx::step_geometry(cfg->batch, A, e->bmw, e->W, !(e->flags & 2u), epw_override,
                                     obs_elem_bytes(cfg->obs_dtype), waves_override, true);
    for (pgx::StepGeometry* g : {&e->geo, &e->geo_roll}) {
        if (const char* f = getenv("PGX_STAGGER")) g->stagger = atoi(f);  // tuning/diagnostic override
        if (const char* f = getenv("PGX_STORE")) {  // tuning/diagnostic override: plain | nt | sc1
            const std::string v = f;
            g->store_policy = v == "plain" ? 0 : v == "nt" ? 1 : v == "sc1" ? 2 : g->store_policy;
        }
        if (const char* f = getenv("PGX_STATE_STORES")) {  // tuning/diagnostic override: 0 | 1 | 2; anything else is ignored
            const int v = atoi(f);  // (an out-of-range value would make emit_state() fire at NO call site: state never written)
            if (v >= 0 && v <= 2 && f[0] >= '0' && f[0] <= '2' && f[1] == 0) g->state_stores = v;
        }
        if (const char* f = getenv("PGX_LDS_MIN")) {  // diagnostic: cap residency by reserving LDS per workgroup
            const size_t m = (size_t)atol(f);
            if (m > g->lds_bytes) g->lds_bytes = (m + 15) & ~(size_t)15;
        }
    }
    if (e->geo_roll.lds_bytes > e->geo.lds_bytes && e->geo_roll.lds_bytes > 160 * 1024) e->geo_roll = e->geo;
    if (e->geo.lds_bytes > 160 * 1024) {
        const size_t need = e->geo.lds_bytes;
        const int bm_bytes = e->bmw * 4, Wd = e->W;
        delete e;
        return fail_msg(PGX_E_INVALID,
                        "configuration needs %zu bytes of LDS per workgroup (> 163840) even in the large-map layout (occupancy "
                        "bitmap of %dx%d cells = %d bytes, plus the exchange arrays and row masks of %d agents with a %dx%d "
                        "window): see the Limits table in README.md",
                        need, cfg->height + 2 * r, cfg->width + 2 * r, bm_bytes, A, Wd, Wd);
    }

    *out_e = e;
    return PGX_OK;
}

int pgx_check_config(const pgx_config* cfg) {
    if (!cfg) return fail_msg(PGX_E_INVALID, "pgx_check_config: null argument");
    pgx_env* e = nullptr;
    const int rc = create_host_side(cfg, 0, &e);
    delete e;
    return rc;
}

// Everything of pgx_create that needs the device; the caller destroys the half-built handle when it fails.
static int create_device_side(pgx_env* e) {
    const pgx_config* cfg = &e->cfg;
    const int A = cfg->num_agents, device = e->device;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess)
        return fail_msg(PGX_E_HIP, "cannot select HIP device %d: %s", device, hipGetErrorString(guard.err));
    // The workgroup -> slice mapping, the per-XCD shares and the cohort stagger of the step kernel assume what this pool's
    // MI355X are: ONE compute partition of 8 XCDs (SPX), where hardware deals consecutive workgroups out round-robin
    // (blockIdx & 7 == XCD) -- VERDICT r3 weak #9.  Results never depend on it, but the tuning would be meaningless on a
    // partitioned device (CPX/DPX/QPX expose fewer CUs per device) or another part: there the engine falls back to the
    // identity mapping with equal shares and no stagger, and pgx_xcd_tune is a no-op.  PGX_ASSUME_PARTITIONED=1 forces
    // that path (tests/test_api_gpu.py runs the parity geometries on it).
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 0;
        const char* force = getenv("PGX_ASSUME_PARTITIONED");
        e->xcd_aware = cus == 256 && !(force && force[0] == '1');
        if (!e->xcd_aware) {
            e->flags |= 8u;
            e->geo.stagger = 0;
            e->geo_roll.stagger = 0;
        }
    }
    const size_t B = (size_t)cfg->batch, BA = B * A;
    hipError_t err = hipSuccess;
    auto alloc = [&](auto& buf, size_t bytes) {
        if (err == hipSuccess) err = buf.alloc(bytes);
    };
    // (+ 4 words: the window funnel reads the word behind the last one of a row unconditionally -- in LDS that is the next
    // array, in the large-map layout, which reads the HBM bitmap directly, it must still be inside the allocation)
    alloc(e->obst, (B * e->bmw + 4) * sizeof(uint32_t));
    alloc(e->pos, BA * sizeof(uint32_t));
    alloc(e->tgt, BA * sizeof(uint32_t));
    alloc(e->pos0, BA * sizeof(uint32_t));
    alloc(e->tgt0, BA * sizeof(uint32_t));
    alloc(e->active, BA);
    alloc(e->elapsed, B * sizeof(int32_t));
    alloc(e->macc, B * sizeof(int4));
    alloc(e->map_u8, B * (size_t)cfg->height * cfg->width);
    alloc(e->todo, B);
    alloc(e->regen, B);
    alloc(e->epoch, B * sizeof(uint32_t));
    alloc(e->fail_count, sizeof(uint32_t));
    alloc(e->regen_fail, sizeof(uint32_t));
    alloc(e->bad_count, sizeof(uint32_t));
    alloc(e->copy_same, B);
    if (cfg->on_target == PGX_ON_TARGET_RESTART) {
        const size_t cells = B * (size_t)cfg->height * cfg->width;
        alloc(e->comp_begin, cells * sizeof(uint32_t));
        alloc(e->comp_len, cells * sizeof(uint32_t));
        alloc(e->comp_cells, cells * sizeof(uint32_t));
        alloc(e->tcount, BA * sizeof(uint32_t));
        if (cfg->lifelong_rng == PGX_LIFELONG_RNG_NUMPY) {
            alloc(e->np_state, BA * sizeof(pgx::NpGen));
            alloc(e->np_state0, BA * sizeof(pgx::NpGen));
        }
    }
    if (err != hipSuccess) return fail_msg(alloc_code(err), "hipMalloc failed: %s", hipGetErrorString(err));
    err = hipMemset(e->regen_fail, 0, sizeof(uint32_t));
    if (err == hipSuccess) err = hipMemset(e->bad_count, 0, sizeof(uint32_t));
    if (err == hipSuccess && e->np_state0)
        err = pgx::launch_init_np_lifelong(e->np_state0, cfg->seed, cfg->env_index_base, cfg->batch, A, nullptr);
    if (err == hipSuccess && e->np_state0) err = hipStreamSynchronize(nullptr);
    if (err == hipSuccess) err = pgx::prepare_step(e->geo, e->geo_roll);
    if (err == hipSuccess && pgx::held_available(e->geo, A, e->W, obs_elem_bytes(cfg->obs_dtype)))
        err = pgx::prepare_step_held(e->geo, A, e->W);  // here, not at the first pgx_step_held: the call stays capturable
    if (err != hipSuccess)
        return fail_msg(PGX_E_HIP, "cannot configure the step kernel (%zu bytes of LDS): %s", e->geo.lds_bytes,
                        hipGetErrorString(err));
    if (const char* spec = getenv("PGX_XCD_WEIGHTS")) {  // eight comma-separated weights (diagnostic)
        float f[8], sum = 0.f;
        if (sscanf(spec, "%f,%f,%f,%f,%f,%f,%f,%f", &f[0], &f[1], &f[2], &f[3], &f[4], &f[5], &f[6], &f[7]) == 8) {
            for (float q : f) sum += q > 0.f ? q : 0.f;
            if (sum > 0.f)
                for (int x = 0; x < 8; ++x) e->xcd_w[x] = (f[x] > 0.f ? f[x] : 0.f) / sum;
        }
    }
    apply_xcd_shares(e);
    err = pgx::prepare_expert(cfg->height, cfg->width);
    if (err != hipSuccess) return fail_msg(PGX_E_HIP, "cannot configure the expert kernel: %s", hipGetErrorString(err));
    if (e->flags & 4u) {  // diagnostic time stamps, one record per workgroup
        e->dbg_elems = (size_t)cfg->batch * 4;
        if (e->dbg.alloc(e->dbg_elems * sizeof(unsigned long long)) == hipSuccess)
            (void)hipMemset(e->dbg, 0, e->dbg_elems * sizeof(unsigned long long));
    }
    return PGX_OK;
}

int pgx_create(const pgx_config* cfg, int device, pgx_env** out) {
    if (!cfg || !out) return fail_msg(PGX_E_INVALID, "pgx_create: null argument");
    *out = nullptr;
    pgx_env* e = nullptr;
    if (const int rc = create_host_side(cfg, device, &e)) return rc;
    if (const int rc = create_device_side(e)) {
        pgx_destroy(e);
        return rc;
    }
    *out = e;
    return PGX_OK;
}

int pgx_destroy(pgx_env* e) {
    if (!e) return PGX_OK;
    DeviceGuard guard(e->device);  // the handle's buffers are freed on their device
    delete e;
    return PGX_OK;
}

int64_t pgx_obs_elems(const pgx_env* e) {
    if (!e) return 0;
    return (int64_t)e->cfg.batch * e->cfg.num_agents * 3 * e->W * e->W;
}

int64_t pgx_agent_elems(const pgx_env* e) {
    if (!e) return 0;
    return (int64_t)e->cfg.batch * e->cfg.num_agents;
}

// ---- reset path ---------------------------------------------------------------------------------------
// Scratch of the reset kernel: 9 bytes per cell and slot (draft map, labels, pending); the pool kernels need the
// pending words only (`pool`: 4 bytes).  The synchronous resets walk the batch in chunks of <= 2^25 cells' worth of
// environments (<= 288 MiB); pgx_regenerate, which must not return to the host between chunks, wants one slot per
// environment (`full`).
static int ensure_reset_scratch(pgx_env* e, bool full, bool pool = false) {
    const size_t cells = (size_t)e->cfg.height * e->cfg.width;
    const size_t per_cell = pool ? 4 : 9;
    size_t chunk = ((size_t)1 << 25) / cells;
    chunk = std::max<size_t>(1, std::min<size_t>(chunk, (size_t)e->cfg.batch));
    if (full) {
        chunk = (size_t)e->cfg.batch;
        if (chunk * cells * per_cell > ((size_t)32 << 30))
            return fail_msg(PGX_E_NOMEM, "%s needs %zu bytes of scratch (%zu per cell and env); use %s",
                            pool ? "pgx_regenerate_pool" : "pgx_regenerate", chunk * cells * per_cell, per_cell,
                            pool ? "pgx_reset_pool" : "pgx_reset_random");
    }
    if (e->pending && (size_t)e->chunk_envs >= chunk && (pool || e->labels)) return PGX_OK;
    auto release = [e]() {
        e->labels.reset();
        e->pending.reset();
        e->scratch_map.reset();
    };
    if (e->pending) {
        PGX_HIP(hipDeviceSynchronize());
        release();
    }
    e->chunk_envs = 0;
    hipError_t err = e->pending.alloc(chunk * cells * sizeof(uint32_t));
    if (err == hipSuccess && !pool) err = e->labels.alloc(chunk * cells * sizeof(uint32_t));
    if (err == hipSuccess && !pool) err = e->scratch_map.alloc(chunk * cells);
    if (err != hipSuccess) {  // all or nothing: a later call must not find half of the scratch
        release();
        return fail_msg(alloc_code(err), "reset scratch (%zu bytes): %s", chunk * cells * per_cell, hipGetErrorString(err));
    }
    e->chunk_envs = (int)chunk;
    return PGX_OK;
}

static pgx::OutsideParams outside_params(const pgx_env* e) {
    pgx::OutsideParams o;
    o.enabled = e->cfg.random_outside ? 1 : 0;
    o.thr = pgx::gen_density_threshold(e->cfg.outside_density);
    o.seed = e->cfg.seed;
    o.env_index_base = e->cfg.env_index_base;
    o.epoch = e->epoch;
    return o;
}

static pgx::ResetParams reset_params(const pgx_env* e) {
    const pgx_config& c = e->cfg;
    pgx::ResetParams p;
    memset(&p, 0, sizeof p);
    p.H = c.height; p.Wd = c.width; p.A = c.num_agents; p.r = c.obs_radius; p.wpr = e->wpr; p.bmw = e->bmw;
    p.lifelong = c.on_target == PGX_ON_TARGET_RESTART;
    p.todo = e->todo; p.epoch = e->epoch;
    p.scratch_map = e->scratch_map; p.labels = e->labels; p.pending = e->pending;
    p.map_u8 = e->map_u8; p.obst_bm = e->obst;
    p.pos = e->pos; p.tgt = e->tgt; p.pos0 = e->pos0; p.tgt0 = e->tgt0; p.active = e->active; p.tcount = e->tcount;
    p.np_state = e->np_state; p.np_state0 = e->np_state0;
    p.elapsed = e->elapsed; p.macc = e->macc;
    p.comp_begin = e->comp_begin; p.comp_len = e->comp_len; p.comp_cells = e->comp_cells;
    p.fail_count = e->fail_count;
    p.outside = outside_params(e);
    return p;
}

int pgx_reset_from_state(pgx_env* e, const uint8_t* obstacles, const int32_t* agent_xy, const int32_t* target_xy,
                         void* stream) {
    if (!e || !obstacles || !agent_xy || !target_xy) return fail_msg(PGX_E_INVALID, "pgx_reset_from_state: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_reset_from_state", false)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const pgx_config& c = e->cfg;
    const size_t B = (size_t)c.batch, BA = B * c.num_agents;
    const int cells = c.height * c.width;
    PGX_HIP(hipMemcpyAsync(e->map_u8, obstacles, B * cells, hipMemcpyDeviceToDevice, s));
    PGX_HIP(pgx::launch_reset_begin(nullptr, e->todo, e->regen, e->epoch, c.batch, s));
    PGX_HIP(pgx::launch_pack_obstacles(e->map_u8, nullptr, e->obst, c.batch, c.height, c.width, c.obs_radius, e->wpr,
                                       e->bmw, outside_params(e), s));
    PGX_HIP(pgx::launch_pack_agents(agent_xy, target_xy, e->pos, e->tgt, e->pos0, e->tgt0, e->active, e->tcount, BA,
                                    c.obs_radius, s, e->np_state, e->np_state0));
    PGX_HIP(pgx::launch_zero_i32(e->elapsed, B, s));
    PGX_HIP(pgx::launch_zero_i32(reinterpret_cast<int32_t*>(e->macc.p), B * 4, s));
    if (e->map_index) PGX_HIP(hipMemsetAsync(e->map_index, 0xFF, B * sizeof(int32_t), s));
    if (c.on_target == PGX_ON_TARGET_RESTART) {  // component tables of PogemaLifeLong, built on the device
        if (int rc = ensure_reset_scratch(e, false)) return rc;
        pgx::ResetParams p = reset_params(e);
        p.given_state = 1;
        for (int b0 = 0; b0 < c.batch; b0 += e->chunk_envs) {
            p.env_begin = b0;
            p.env_count = std::min(e->chunk_envs, c.batch - b0);
            PGX_HIP(pgx::launch_reset_env(p, s));
        }
    }
    e->has_state = true;
    return PGX_OK;
}

int pgx_reset_random(pgx_env* e, float density, uint64_t seed, const uint8_t* shared_map, const uint8_t* env_mask,
                     int32_t max_retries, void* stream) {
    if (!e) return fail_msg(PGX_E_INVALID, "pgx_reset_random: null handle");
    if (!shared_map && !(density >= 0.0f && density <= 1.0f))
        return fail_msg(PGX_E_INVALID, "density %.3f outside [0, 1]", (double)density);
    if (env_mask && !e->has_state) return fail_msg(PGX_E_STATE, "masked pgx_reset_random before the first full reset");
    const pgx_config& c = e->cfg;
    const int cells = c.height * c.width;
    if ((int64_t)2 * c.num_agents > (int64_t)cells)
        return fail_msg(PGX_E_PLACEMENT, "%d agents need %d distinct cells, map has %d", c.num_agents, 2 * c.num_agents, cells);
    if (max_retries < 1) max_retries = 10;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_reset_random", false)) return rc;
    if (int rc = ensure_reset_scratch(e, false)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::ResetParams p = reset_params(e);
    p.max_retries = max_retries;
    p.thr = pgx::gen_density_threshold(density);
    p.gen_seed = seed;  // env i draws instance (seed, env_index_base + i): two key components, hashed separately
    p.env_index_base = c.env_index_base;
    p.shared_map = shared_map;
    PGX_HIP(pgx::launch_reset_begin(env_mask, e->todo, e->regen, e->epoch, c.batch, s));
    PGX_HIP(hipMemsetAsync(e->fail_count, 0, sizeof(uint32_t), s));
    for (int b0 = 0; b0 < c.batch; b0 += e->chunk_envs) {
        p.env_begin = b0;
        p.env_count = std::min(e->chunk_envs, c.batch - b0);
        PGX_HIP(pgx::launch_reset_env(p, s));
    }
    if (e->map_index) PGX_HIP(pgx::launch_clear_map_index(e->regen, e->todo, e->map_index, c.batch, s));
    uint32_t failed = 0;
    PGX_HIP(hipMemcpyAsync(&failed, e->fail_count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    PGX_HIP(hipStreamSynchronize(s));  // the status is the device's failure count
    if (failed) {
        if (!env_mask) e->has_state = false;  // (masked: the failed envs keep their previous instance)
        return fail_msg(PGX_E_PLACEMENT, "could not place %d agents in %u environment(s) after %d attempts (density %.2f, %dx%d)",
                        c.num_agents, failed, max_retries, (double)density, c.height, c.width);
    }
    e->has_state = true;
    return PGX_OK;
}

int pgx_regenerate(pgx_env* e, const uint8_t* env_mask, float density, uint64_t seed, const uint8_t* shared_map,
                   int32_t max_retries, void* obs, void* stream) {
    if (!e || !env_mask) return fail_msg(PGX_E_INVALID, "pgx_regenerate: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_regenerate", true)) return rc;
    if (!shared_map && !(density >= 0.0f && density <= 1.0f))
        return fail_msg(PGX_E_INVALID, "density %.3f outside [0, 1]", (double)density);
    if (max_retries < 1) max_retries = 3;
    if (int rc = ensure_reset_scratch(e, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const pgx_config& c = e->cfg;
    pgx::ResetParams p = reset_params(e);
    p.max_retries = max_retries;
    p.thr = pgx::gen_density_threshold(density);
    p.gen_seed = seed;
    p.env_index_base = c.env_index_base;
    p.shared_map = shared_map;
    p.fail_count = e->regen_fail;
    p.env_begin = 0;
    p.env_count = c.batch;
    PGX_HIP(pgx::launch_reset_begin(env_mask, e->todo, e->regen, e->epoch, c.batch, s));
    PGX_HIP(pgx::launch_reset_env(p, s));
    if (e->map_index) PGX_HIP(pgx::launch_clear_map_index(e->regen, e->todo, e->map_index, c.batch, s));
    if (obs) {
        pgx::StepParams sp = observe_params(e, obs);
        sp.only = e->regen;
        PGX_HIP(pgx::launch_step(sp, e->geo, s));
    }
    return PGX_OK;
}

int64_t pgx_regenerate_failures(pgx_env* e, void* stream) {
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_regenerate_failures", false)) return rc;
    uint32_t n = 0;
    PGX_HIP(hipMemcpyAsync(&n, e->regen_fail, sizeof n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    PGX_HIP(hipStreamSynchronize((hipStream_t)stream));
    return (int64_t)n;
}

// ---- map pool (docs/SPEC.md S10) ------------------------------------------------------------------------
int pgx_set_map_pool(pgx_env* e, const uint8_t* maps, int32_t num_maps, int32_t* capacity_out, void* stream) {
    if (!e || !maps) return fail_msg(PGX_E_INVALID, "pgx_set_map_pool: null argument");
    if (num_maps < 1) return fail_msg(PGX_E_INVALID, "pgx_set_map_pool: num_maps must be >= 1, got %d", num_maps);
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_set_map_pool", false)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    PGX_HIP(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail_msg(PGX_E_STATE, "pgx_set_map_pool: the install check reads each map's capacity on the host; install "
                                     "the pool outside graph capture (a same-size pool keeps its buffers, so a captured "
                                     "graph sees it)");
    const pgx_config& c = e->cfg;
    const size_t cells = (size_t)c.height * c.width, M = (size_t)num_maps;
    if (int rc = ensure_reset_scratch(e, false, true)) return rc;
    if (num_maps != e->pool_size) {
        // work already queued may still read the old pool: it finishes before the buffers go
        PGX_HIP(hipDeviceSynchronize());
        e->pool_size = 0;
        hipError_t err = e->pool_maps.alloc(M * cells);
        if (err == hipSuccess) err = e->pool_labels.alloc(M * cells * sizeof(uint32_t));
        if (err == hipSuccess) err = e->pool_cap.alloc(M * sizeof(uint32_t));
        if (err == hipSuccess && !e->map_index) {
            err = e->map_index.alloc((size_t)c.batch * sizeof(int32_t));
            if (err == hipSuccess) err = hipMemsetAsync(e->map_index, 0xFF, (size_t)c.batch * sizeof(int32_t), s);
        }
        if (err != hipSuccess) {
            e->pool_maps.reset();
            e->pool_labels.reset();
            e->pool_cap.reset();
            return fail_msg(alloc_code(err), "pgx_set_map_pool: %zu bytes for %d maps of %dx%d: %s", M * cells * 5 + M * 4,
                            num_maps, c.height, c.width, hipGetErrorString(err));
        }
    }
    for (size_t m0 = 0; m0 < M; m0 += (size_t)e->chunk_envs) {
        const int count = (int)std::min<size_t>((size_t)e->chunk_envs, M - m0);
        PGX_HIP(pgx::launch_pool_label(maps + m0 * cells, e->pool_maps + m0 * cells, e->pool_labels + m0 * cells, e->pending,
                                       e->pool_cap + m0, count, c.height, c.width, s));
    }
    e->pool_size = num_maps;
    std::vector<uint32_t> capacity(M);
    PGX_HIP(hipMemcpyAsync(capacity.data(), e->pool_cap, M * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    PGX_HIP(hipStreamSynchronize(s));
    if (capacity_out)
        for (size_t m = 0; m < M; ++m) capacity_out[m] = (int32_t)capacity[m];
    for (size_t m = 0; m < M; ++m)
        if ((int64_t)capacity[m] < (int64_t)c.num_agents) {
            // the refused pool is not installed (nor is the one it replaced): the envs keep their current instances
            e->pool_size = 0;
            return fail_msg(PGX_E_PLACEMENT, "pgx_set_map_pool: map %zu of the pool holds %u start/target pairs, %d agents "
                                             "need %d (each pair lies in one connected component)",
                            m, capacity[m], c.num_agents, c.num_agents);
        }
    return PGX_OK;
}

static pgx::ResetParams pool_reset_params(const pgx_env* e, uint64_t seed, int32_t max_retries) {
    pgx::ResetParams p = reset_params(e);
    p.max_retries = max_retries;
    p.gen_seed = seed;
    p.env_index_base = e->cfg.env_index_base;
    p.pool_size = e->pool_size;
    p.pool_maps = e->pool_maps;
    p.pool_labels = e->pool_labels;
    p.map_index = e->map_index;
    return p;
}

int pgx_reset_pool(pgx_env* e, uint64_t seed, const uint8_t* env_mask, int32_t max_retries, void* stream) {
    if (!e) return fail_msg(PGX_E_INVALID, "pgx_reset_pool: null handle");
    if (!e->pool_size) return fail_msg(PGX_E_STATE, "pgx_reset_pool: no map pool installed (pgx_set_map_pool)");
    if (env_mask && !e->has_state) return fail_msg(PGX_E_STATE, "masked pgx_reset_pool before the first full reset");
    const pgx_config& c = e->cfg;
    if (max_retries < 1) max_retries = 10;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_reset_pool", false)) return rc;
    if (int rc = ensure_reset_scratch(e, false, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::ResetParams p = pool_reset_params(e, seed, max_retries);
    PGX_HIP(pgx::launch_reset_begin(env_mask, e->todo, e->regen, e->epoch, c.batch, s));
    PGX_HIP(hipMemsetAsync(e->fail_count, 0, sizeof(uint32_t), s));
    for (int b0 = 0; b0 < c.batch; b0 += e->chunk_envs) {
        p.env_begin = b0;
        p.env_count = std::min(e->chunk_envs, c.batch - b0);
        PGX_HIP(pgx::launch_reset_pool(p, s));
    }
    uint32_t failed = 0;
    PGX_HIP(hipMemcpyAsync(&failed, e->fail_count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    PGX_HIP(hipStreamSynchronize(s));  // the status is the device's failure count
    if (failed) {
        if (!env_mask) e->has_state = false;  // (masked: the failed envs keep their previous instance)
        return fail_msg(PGX_E_PLACEMENT, "could not place %d agents in %u environment(s) after %d attempts on maps of the "
                                         "pool (%d maps of %dx%d)",
                        c.num_agents, failed, max_retries, e->pool_size, c.height, c.width);
    }
    e->has_state = true;
    return PGX_OK;
}

int pgx_regenerate_pool(pgx_env* e, const uint8_t* env_mask, uint64_t seed, int32_t max_retries, void* obs, void* stream) {
    if (!e || !env_mask) return fail_msg(PGX_E_INVALID, "pgx_regenerate_pool: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_regenerate_pool", true)) return rc;
    if (!e->pool_size) return fail_msg(PGX_E_STATE, "pgx_regenerate_pool: no map pool installed (pgx_set_map_pool)");
    if (max_retries < 1) max_retries = 3;
    if (int rc = ensure_reset_scratch(e, true, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const pgx_config& c = e->cfg;
    pgx::ResetParams p = pool_reset_params(e, seed, max_retries);
    p.fail_count = e->regen_fail;
    p.env_begin = 0;
    p.env_count = c.batch;
    PGX_HIP(pgx::launch_reset_begin(env_mask, e->todo, e->regen, e->epoch, c.batch, s));
    PGX_HIP(pgx::launch_reset_pool(p, s));
    if (obs) {
        pgx::StepParams sp = observe_params(e, obs);
        sp.only = e->regen;
        PGX_HIP(pgx::launch_step(sp, e->geo, s));
    }
    return PGX_OK;
}

int pgx_get_map_index(pgx_env* e, int32_t* out, void* stream) {
    if (!e || !out) return fail_msg(PGX_E_INVALID, "pgx_get_map_index: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_get_map_index", false)) return rc;
    const size_t bytes = (size_t)e->cfg.batch * sizeof(int32_t);
    if (e->map_index) PGX_HIP(hipMemcpyAsync(out, e->map_index, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else PGX_HIP(hipMemsetAsync(out, 0xFF, bytes, (hipStream_t)stream));
    return PGX_OK;
}

// ---- snapshot / restore of the complete engine state (checkpoint-resume, `step_back`) ---------------------
extern "C++" {
namespace {
// One array of the per-environment state: `bytes` in all, `row` bytes per env.  What the array is to a copy of one env
// onto another slot (pgx_copy_envs; save / load take every segment whole): SEG_STATE is copied, SEG_MAP is copied unless
// both envs hold the same map (it is a function of the map), SEG_SLOT belongs to the slot and stays.
enum SegKind { SEG_STATE = 0, SEG_MAP = 1, SEG_SLOT = 2 };
struct Segment {
    void* ptr;
    size_t bytes;
    size_t row;
    SegKind kind;
};
// with_pool: the layout of a handle with a map pool installed (map_index appended as the last segment)
std::vector<Segment> snapshot_segments(pgx_env* e, bool with_pool) {
    const pgx_config& c = e->cfg;
    const size_t B = (size_t)c.batch, A = (size_t)c.num_agents, cells = (size_t)c.height * c.width;
    std::vector<Segment> seg;
    auto add = [&](void* ptr, size_t row, SegKind kind) { seg.push_back({ptr, B * row, row, kind}); };
    add(e->pos, A * 4, SEG_STATE);
    add(e->tgt, A * 4, SEG_STATE);
    add(e->pos0, A * 4, SEG_STATE);
    add(e->tgt0, A * 4, SEG_STATE);
    add(e->active, A, SEG_STATE);
    add(e->elapsed, 4, SEG_STATE);
    add(e->macc, sizeof(int4), SEG_STATE);
    add(e->epoch, 4, SEG_SLOT);  // the generation counter: the slot's next instance stays the slot's
    add(e->map_u8, cells, SEG_MAP);
    add(e->obst, (size_t)e->bmw * 4, SEG_MAP);
    if (c.on_target == PGX_ON_TARGET_RESTART) {
        add(e->tcount, A * 4, SEG_STATE);
        if (e->np_state) add(e->np_state, A * sizeof(pgx::NpGen), SEG_STATE);
        add(e->comp_begin, cells * 4, SEG_MAP);
        add(e->comp_len, cells * 4, SEG_MAP);
        add(e->comp_cells, cells * 4, SEG_MAP);
    }
    if (with_pool) add(e->map_index, 4, SEG_STATE);
    return seg;
}
size_t aligned16(size_t n) { return (n + 15) & ~(size_t)15; }
// Snapshot header: everything the segment sizes and the meaning of the payload depend on.
constexpr int32_t SNAP_MAGIC = 0x50475853;  // 'PGXS'
constexpr size_t SNAP_HEADER_BYTES = 64;
struct SnapHeader {
    int32_t magic, abi, batch, num_agents, height, width, obs_radius, on_target, collision_system, max_episode_steps;
    int64_t total_bytes;
    int32_t has_pool;  // 1: the last segment is map_index (a handle with a map pool); 0 otherwise
    int32_t pad[3];
};
static_assert(sizeof(SnapHeader) == SNAP_HEADER_BYTES, "snapshot header layout");
size_t snapshot_total(pgx_env* e, bool with_pool) {
    size_t total = SNAP_HEADER_BYTES;
    for (const Segment& s : snapshot_segments(e, with_pool)) total += aligned16(s.bytes);
    return total;
}
SnapHeader snapshot_header(pgx_env* e, bool with_pool) {
    const pgx_config& c = e->cfg;
    const int64_t total = (int64_t)snapshot_total(e, with_pool);
    SnapHeader h{};
    h.has_pool = with_pool ? 1 : 0;
    h.magic = SNAP_MAGIC; h.abi = PGX_ABI_VERSION; h.batch = c.batch; h.num_agents = c.num_agents;
    h.height = c.height; h.width = c.width; h.obs_radius = c.obs_radius; h.on_target = c.on_target;
    h.collision_system = c.collision_system; h.max_episode_steps = c.max_episode_steps; h.total_bytes = total;
    return h;
}
}  // namespace
}  // extern "C++"

int64_t pgx_snapshot_bytes(pgx_env* e) {
    if (!e) return 0;
    return (int64_t)snapshot_total(e, e->pool_size > 0);
}

int pgx_save_snapshot(pgx_env* e, void* blob, void* stream) {
    if (!e || !blob) return fail_msg(PGX_E_INVALID, "pgx_save_snapshot: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_save_snapshot", true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool with_pool = e->pool_size > 0;
    const SnapHeader header = snapshot_header(e, with_pool);
    PGX_HIP(hipMemcpyAsync(blob, &header, sizeof header, hipMemcpyHostToDevice, s));
    PGX_HIP(hipStreamSynchronize(s));  // `header` lives on this stack frame
    size_t off = SNAP_HEADER_BYTES;
    for (const Segment& g : snapshot_segments(e, with_pool)) {
        PGX_HIP(hipMemcpyAsync((char*)blob + off, g.ptr, g.bytes, hipMemcpyDeviceToDevice, s));
        off += aligned16(g.bytes);
    }
    return PGX_OK;
}

int pgx_load_snapshot(pgx_env* e, const void* blob, void* stream) {
    if (!e || !blob) return fail_msg(PGX_E_INVALID, "pgx_load_snapshot: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_load_snapshot", false)) return rc;
    hipStream_t s = (hipStream_t)stream;
    SnapHeader got{};
    PGX_HIP(hipMemcpyAsync(&got, blob, sizeof got, hipMemcpyDeviceToHost, s));
    PGX_HIP(hipStreamSynchronize(s));
    // a handle with a pool also takes a snapshot made without one (its envs then run no pool map: map_index = -1)
    const bool with_pool = e->pool_size > 0 && got.has_pool != 0;
    const SnapHeader want = snapshot_header(e, with_pool);
    if (got.has_pool && !e->pool_size)
        return fail_msg(PGX_E_INVALID, "snapshot was taken with a map pool installed; install a pool of the same size "
                                       "(pgx_set_map_pool) before loading it");
    if (memcmp(&got, &want, sizeof want) != 0)
        return fail_msg(PGX_E_INVALID,
                        "snapshot does not belong to this configuration: blob has magic %08x abi %d batch %d agents %d map %dx%d "
                        "r %d on_target %d collision %d max_steps %d bytes %lld; this handle abi %d batch %d agents %d map %dx%d "
                        "r %d on_target %d collision %d max_steps %d bytes %lld",
                        (unsigned)got.magic, got.abi, got.batch, got.num_agents, got.height, got.width, got.obs_radius,
                        got.on_target, got.collision_system, got.max_episode_steps, (long long)got.total_bytes, want.abi,
                        want.batch, want.num_agents, want.height, want.width, want.obs_radius, want.on_target,
                        want.collision_system, want.max_episode_steps, (long long)want.total_bytes);
    size_t off = SNAP_HEADER_BYTES;
    for (const Segment& g : snapshot_segments(e, with_pool)) {
        PGX_HIP(hipMemcpyAsync(g.ptr, (const char*)blob + off, g.bytes, hipMemcpyDeviceToDevice, s));
        off += aligned16(g.bytes);
    }
    if (e->map_index && !with_pool) PGX_HIP(hipMemsetAsync(e->map_index, 0xFF, (size_t)e->cfg.batch * sizeof(int32_t), s));
    e->has_state = true;
    return PGX_OK;
}

// ---- environment copies (docs/SPEC.md S19) ---------------------------------------------------------------
int pgx_copy_envs(pgx_env* e, const int32_t* src, const int32_t* dst, int32_t count, int32_t flags, void* stream) {
    static const char who[] = "pgx_copy_envs";
    if (count < 0) return fail_msg(PGX_E_INVALID, "%s: count must be >= 0, got %d", who, count);
    if (count > 0 && !src) return fail_msg(PGX_E_INVALID, "%s: src is null", who);
    if (count > 0 && !dst) return fail_msg(PGX_E_INVALID, "%s: dst is null", who);
    if (const int rc = check_flags(who, flags, PGX_COPY_NO_CACHE)) return rc;
    if (!e) return fail_msg(PGX_E_INVALID, "%s: env is null", who);
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    if (count == 0) return PGX_OK;
    hipStream_t s = (hipStream_t)stream;
    const pgx_config& c = e->cfg;
    pgx::CopyParams p;
    memset(&p, 0, sizeof p);
    p.src = src;
    p.dst = dst;
    p.count = count;
    p.batch = c.batch;
    for (const Segment& g : snapshot_segments(e, e->map_index != nullptr)) {
        if (g.kind == SEG_SLOT) continue;
        if (p.nseg == pgx::COPY_MAX_SEGS) return fail_msg(PGX_E_STATE, "%s: more than %d state segments", who, pgx::COPY_MAX_SEGS);
        pgx::CopySeg& q = p.seg[p.nseg++];
        q.base = static_cast<char*>(g.ptr);
        q.row = g.row;
        q.of_map = g.kind == SEG_MAP ? 1 : 0;
    }
    p.chunks = pgx::copy_plan_chunks(p.seg, p.nseg, count);
    PGX_HIP(pgx::launch_copy_compare(p, e->obst, e->bmw, e->map_index, e->copy_same, s));
    PGX_HIP(pgx::launch_copy_rows(p, e->copy_same, s));
    if (e->c2g && !(flags & PGX_COPY_NO_CACHE)) {  // the pairs' rows of the distance-field cache: nothing to rebuild after a branch
        const pgx::CostToGoLayout l = pgx::cost_to_go_layout(c.batch, c.num_agents, c.height, c.width);
        const size_t cells = (size_t)c.height * c.width, A = (size_t)c.num_agents;
        pgx::CopyParams q = p;
        q.nseg = 3;
        q.seg[0] = {reinterpret_cast<char*>(e->c2g.p) + l.tag_off, A * sizeof(uint32_t), 0, 0, 0, 0};
        q.seg[1] = {reinterpret_cast<char*>(e->c2g.p) + l.map_off, (size_t)c.height * ((c.width + 31) / 32) * sizeof(uint32_t), 0, 0, 0, 0};
        q.seg[2] = {reinterpret_cast<char*>(e->c2g.p) + l.field_off, A * cells * l.cell_bytes, 0, 0, 0, 0};
        q.chunks = pgx::copy_plan_chunks(q.seg, q.nseg, count);
        PGX_HIP(pgx::launch_copy_rows(q, nullptr, s));
    }
    return PGX_OK;
}

int pgx_get_map(pgx_env* e, uint8_t* obstacles, void* stream) {
    if (!e || !obstacles) return fail_msg(PGX_E_INVALID, "pgx_get_map: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_get_map", true)) return rc;
    PGX_HIP(hipMemcpyAsync(obstacles, e->map_u8, (size_t)e->cfg.batch * e->cfg.height * e->cfg.width,
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PGX_OK;
}

int pgx_step(pgx_env* e, const void* actions, int action_dtype, void* obs, float* rewards, uint8_t* terminated,
             uint8_t* truncated, uint8_t* is_active, void* stream) {
    if (!e || !actions || !rewards || !terminated || !truncated) return fail_msg(PGX_E_INVALID, "pgx_step: null argument");
    if (const int rc = check_action_dtype("pgx_step", action_dtype)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_step", true)) return rc;
    pgx::StepParams p = step_params(e, e->geo);
    p.mode = pgx::MODE_STEP;
    p.action_dtype = action_dtype;
    p.actions = actions;
    p.obs = static_cast<float*>(obs);
    p.rewards = rewards;
    p.terminated = terminated;
    p.truncated = truncated;
    p.act_out = is_active;
    PGX_HIP(pgx::launch_step(p, e->geo, (hipStream_t)stream));
    return PGX_OK;
}

int pgx_held_available(const pgx_env* e) {
    if (!e) return 0;
    return pgx::held_available(e->geo, e->cfg.num_agents, e->W, obs_elem_bytes(e->cfg.obs_dtype)) ? 1 : 0;
}

int pgx_step_held(pgx_env* e, const void* actions, int action_dtype, void* obs, uint8_t* held, int32_t refresh, float* rewards,
                  uint8_t* terminated, uint8_t* truncated, uint8_t* is_active, void* stream) {
    // no held instance for this shape, or nothing to hold: the plain step
    if (!e || !obs || !held || !pgx_held_available(e))
        return pgx_step(e, actions, action_dtype, obs, rewards, terminated, truncated, is_active, stream);
    if (!actions || !rewards || !terminated || !truncated) return fail_msg(PGX_E_INVALID, "pgx_step_held: null argument");
    if (const int rc = check_action_dtype("pgx_step_held", action_dtype)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_step_held", true)) return rc;
    pgx::StepParams p = step_params(e, e->geo);
    p.mode = pgx::MODE_STEP;
    p.action_dtype = action_dtype;
    p.actions = actions;
    p.obs = static_cast<float*>(obs);
    p.rewards = rewards;
    p.terminated = terminated;
    p.truncated = truncated;
    p.act_out = is_active;
    PGX_HIP(pgx::launch_step_held(p, e->geo, held, refresh != 0, (hipStream_t)stream));
    return PGX_OK;
}

int pgx_rollout(pgx_env* e, int32_t steps, const pgx_rollout_io* io, void* stream) {
    if (!e || !io || !io->rewards || !io->terminated || !io->truncated)
        return fail_msg(PGX_E_INVALID, "pgx_rollout: null argument");
    if (io->policy_step0 < 0 || io->policy_step0 > ((int64_t)1 << 40))
        return fail_msg(PGX_E_INVALID, "pgx_rollout: policy_step0 outside 0..2^40");
    if (steps < 1) return fail_msg(PGX_E_INVALID, "pgx_rollout: steps must be >= 1, got %d", steps);
    if (const int rc = check_action_dtype("pgx_rollout", io->action_dtype)) return rc;
    if (io->obs && io->obs_slots < 1) return fail_msg(PGX_E_INVALID, "pgx_rollout: obs given but obs_slots = %d", io->obs_slots);
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_rollout", true)) return rc;
    pgx::StepParams p = step_params(e, e->geo_roll);
    p.mode = pgx::MODE_STEP;
    p.action_dtype = io->action_dtype;
    p.actions = io->actions;
    p.obs = static_cast<float*>(io->obs);
    p.rewards = io->rewards;
    p.terminated = io->terminated;
    p.truncated = io->truncated;
    p.act_out = io->is_active;
    p.metrics_out = io->metrics;
    p.episode_done = io->episode_done;
    const int64_t agents = (int64_t)e->cfg.batch * e->cfg.num_agents;
    const int64_t W = 2 * e->cfg.obs_radius + 1;
    static const int64_t action_bytes[3] = {1, 4, 8};
    pgx::RolloutParams rp;
    rp.steps = steps;
    rp.obs_slots = io->obs ? io->obs_slots : 1;
    rp.resident_bitmap = e->geo_roll.resident_bitmap ? 1 : 0;
    rp.reserved0 = 0;
    rp.actions_stride = agents * action_bytes[io->action_dtype];
    rp.agents_stride = agents;
    rp.envs_stride = e->cfg.batch;
    rp.obs_stride = agents * 3 * W * W * (int64_t)obs_elem_bytes(e->cfg.obs_dtype);
    rp.policy_seed = io->policy_seed;
    rp.policy_step0 = io->policy_step0;
    rp.actions_out = io->actions ? nullptr : io->actions_out;
    if (io->obs && io->obs_slot_stride != 0) {
        if (io->obs_slot_stride < rp.obs_stride || (io->obs_slot_stride & 15) != 0)
            return fail_msg(PGX_E_INVALID, "pgx_rollout: obs_slot_stride %lld is smaller than one observation tensor (%lld bytes) or not a multiple of 16",
                            (long long)io->obs_slot_stride, (long long)rp.obs_stride);
        rp.obs_stride = io->obs_slot_stride;
    }
    PGX_HIP(pgx::launch_rollout(p, rp, e->geo_roll, (hipStream_t)stream));
    return PGX_OK;
}

int pgx_expert_actions(pgx_env* e, int32_t flags, void* actions, int32_t action_dtype, int32_t* distance, void* stream) {
    static const char who[] = "pgx_expert_actions";
    if (!e || !actions) return fail_msg(PGX_E_INVALID, "%s: null argument", who);
    if (const int rc = check_action_dtype(who, action_dtype)) return rc;
    if (const int rc = check_flags(who, flags, PGX_EXPERT_AGENTS_AS_OBSTACLES)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    const bool with_agents = (flags & PGX_EXPERT_AGENTS_AS_OBSTACLES) != 0;
    const size_t occ_words = pgx::expert_occupancy_words(e->cfg.batch, e->cfg.height, e->cfg.width);
    if (with_agents && occ_words && !e->expert_occ)
        if (const int rc = alloc_on_first_use(e->expert_occ, occ_words * sizeof(uint32_t), (hipStream_t)stream, who,
                                              "the occupancy scratch of PGX_EXPERT_AGENTS_AS_OBSTACLES on maps wider "
                                              "or taller than 64"))
            return rc;
    pgx::ExpertParams p{state_view(e)};
    p.with_agents = with_agents ? 1 : 0;
    p.action_dtype = action_dtype;
    p.occ = e->expert_occ;
    p.actions = actions;
    p.distance = distance;
    PGX_HIP(pgx::launch_expert(p, (hipStream_t)stream));
    return PGX_OK;
}

// ---- cost-to-go windows (docs/SPEC.md S11) --------------------------------------------------------------
int64_t pgx_cost_to_go_bytes(const pgx_config* cfg) {
    if (!cfg) return fail_msg(PGX_E_INVALID, "pgx_cost_to_go_bytes: null argument");
    pgx_env* e = nullptr;
    const int rc = create_host_side(cfg, 0, &e);
    delete e;
    if (rc) return rc;
    return (int64_t)pgx::cost_to_go_layout(cfg->batch, cfg->num_agents, cfg->height, cfg->width).bytes;
}

// The launch parameters of the handle's distance-field cache (without `out`); allocates and clears the cache on the
// first call of any entry point that uses it (pgx_cost_to_go, pgx_pibt_actions, pgx_pibt_plan, pgx_pibt_swap_plan, pgx_whca_plan, pgx_repair_plan, pgx_goal_directions,
// pgx_shield_actions with PGX_SHIELD_TIE_DISTANCE, pgx_policy_input with a direction channel, pgx_agent_tokens, pgx_goal_paths, pgx_agent_forecasts, pgx_blocking).  `who` names that entry point in the error messages.
static int cost_to_go_cache(pgx_env* e, hipStream_t s, const char* who, pgx::CostToGoParams* out_p) {
    const pgx_config& c = e->cfg;
    const pgx::CostToGoLayout l = pgx::cost_to_go_layout(c.batch, c.num_agents, c.height, c.width);
    if (!e->c2g) {
        PGX_HIP(pgx::prepare_cost_to_go(c.height, c.width));
        if (const int rc = alloc_on_first_use(e->c2g, l.bytes, s, who, "the distance-field cache")) return rc;
        // no field, counter 0, an all-obstacle map copy (any installed map differs or leaves every tag cleared)
        hipError_t err = hipMemsetAsync(e->c2g, 0, l.field_off, s);
        if (err == hipSuccess) err = hipMemsetAsync(e->c2g + l.tag_off, 0xFF, l.map_off - l.tag_off, s);
        if (err == hipSuccess) err = hipMemsetAsync(e->c2g + l.map_off, 0, l.bytes - l.map_off, s);
        if (err != hipSuccess) {
            e->c2g.reset();
            return fail_msg(PGX_E_HIP, "%s: clearing the cache failed: %s", who, hipGetErrorString(err));
        }
    }
    pgx::CostToGoParams p{state_view(e)};
    p.cell_bytes = (int32_t)l.cell_bytes;
    p.map_bits = reinterpret_cast<uint32_t*>(e->c2g + l.map_off);
    p.tag = reinterpret_cast<uint32_t*>(e->c2g + l.tag_off);
    p.field = e->c2g + l.field_off;
    p.builds = reinterpret_cast<unsigned long long*>(e->c2g + l.builds_off);
    *out_p = p;
    return PGX_OK;
}

int pgx_cost_to_go(pgx_env* e, int32_t flags, int32_t* out, void* stream) {
    static const char who[] = "pgx_cost_to_go";
    if (!e || !out) return fail_msg(PGX_E_INVALID, "%s: null argument", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    if (const int rc = check_aligned(who, "out", out, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::CostToGoParams p{};
    if (const int rc = cost_to_go_cache(e, s, who, &p)) return rc;
    p.out = out;
    PGX_HIP(pgx::launch_cost_to_go(p, s));
    return PGX_OK;
}

// ---- cooperative planner (docs/SPEC.md S13) --------------------------------------------------------------
int pgx_pibt_actions(pgx_env* e, int32_t flags, const int32_t* priority, void* actions, int32_t action_dtype,
                     int32_t* next_xy, void* stream) {
    static const char who[] = "pgx_pibt_actions";
    // the argument checks come first and need no device
    if (!actions) return fail_msg(PGX_E_INVALID, "%s: actions is null", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    if (const int rc = check_action_dtype(who, action_dtype)) return rc;
    static_assert(PGX_ACTION_I8 == 0 && PGX_ACTION_I32 == 1 && PGX_ACTION_I64 == 2, "action_bytes is indexed by the code");
    static const size_t action_bytes[3] = {1, 4, 8};
    if (const int rc = check_aligned(who, "actions", actions, action_bytes[action_dtype])) return rc;
    if (const int rc = check_aligned(who, "priority", priority, 4)) return rc;
    if (const int rc = check_aligned(who, "next_xy", next_xy, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::CostToGoParams cp{};
    if (const int rc = cost_to_go_cache(e, s, who, &cp)) return rc;
    PGX_HIP(pgx::launch_cost_to_go_refresh(cp, s));
    pgx::PibtParams p{cp};  // (the StateView base of cp; the planner's own fields follow)
    p.action_dtype = action_dtype;
    p.cell_bytes = cp.cell_bytes;
    p.field = cp.field;
    p.priority = priority;
    p.actions = actions;
    p.next_xy = next_xy;
    PGX_HIP(pgx::launch_pibt(p, s));
    return PGX_OK;
}

// ---- cooperative planner with the swap operation (docs/SPEC.md S23) ----------------------------------------
int pgx_pibt_swap_actions(pgx_env* e, int32_t flags, const int32_t* priority, void* actions, int32_t action_dtype,
                          int32_t* next_xy, void* stream) {
    static const char who[] = "pgx_pibt_swap_actions";
    static_assert(PGX_SWAP_MAX_WALK == pgx::SWAP_MAX_WALK, "the header's walk cap is the kernel's");
    // the argument checks come first and need no device
    if (!actions) return fail_msg(PGX_E_INVALID, "%s: actions is null", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    if (const int rc = check_action_dtype(who, action_dtype)) return rc;
    static const size_t action_bytes[3] = {1, 4, 8};
    if (const int rc = check_aligned(who, "actions", actions, action_bytes[action_dtype])) return rc;
    if (const int rc = check_aligned(who, "priority", priority, 4)) return rc;
    if (const int rc = check_aligned(who, "next_xy", next_xy, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::CostToGoParams cp{};
    if (const int rc = cost_to_go_cache(e, s, who, &cp)) return rc;
    PGX_HIP(pgx::launch_cost_to_go_refresh(cp, s));
    pgx::PibtParams p{cp};  // (the StateView base of cp; the planner's own fields follow)
    p.action_dtype = action_dtype;
    p.cell_bytes = cp.cell_bytes;
    p.field = cp.field;
    p.priority = priority;
    p.actions = actions;
    p.next_xy = next_xy;
    PGX_HIP(pgx::launch_pibt_swap(p, s));
    return PGX_OK;
}

// ---- multi-step planner (docs/SPEC.md S16), and the same lookahead with the swap operation (S27) -----------------
static int pibt_plan_entry(const char* who, bool swap, pgx_env* e, int32_t flags, int32_t horizon, const int32_t* priority,
                           void* actions, int32_t action_dtype, int32_t* path_xy, int32_t* arrival, int32_t* priority_out,
                           void* stream) {
    // the argument checks come first and need no device
    if (!actions) return fail_msg(PGX_E_INVALID, "%s: actions is null", who);
    if (const int rc = check_flags(who, flags, PGX_PLAN_FIXED_PRIORITY)) return rc;
    if (horizon < 1 || horizon > PGX_MAX_PLAN_HORIZON)
        return fail_msg(PGX_E_INVALID, "%s: horizon %d is outside 1..%d", who, horizon, PGX_MAX_PLAN_HORIZON);
    if (const int rc = check_action_dtype(who, action_dtype)) return rc;
    static const size_t action_bytes[3] = {1, 4, 8};
    if (const int rc = check_aligned(who, "actions", actions, action_bytes[action_dtype])) return rc;
    if (const int rc = check_aligned(who, "priority", priority, 4)) return rc;
    if (const int rc = check_aligned(who, "path_xy", path_xy, 4)) return rc;
    if (const int rc = check_aligned(who, "arrival", arrival, 4)) return rc;
    if (const int rc = check_aligned(who, "priority_out", priority_out, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::CostToGoParams cp{};
    if (const int rc = cost_to_go_cache(e, s, who, &cp)) return rc;
    PGX_HIP(pgx::launch_cost_to_go_refresh(cp, s));    // once: the targets are held for the whole lookahead
    pgx::PibtPlanParams p{};
    static_cast<pgx::StateView&>(p) = cp;
    p.action_dtype = action_dtype;
    p.cell_bytes = cp.cell_bytes;
    p.field = cp.field;
    p.priority = priority;
    p.actions = actions;
    p.horizon = horizon;
    p.finish = e->cfg.on_target == PGX_ON_TARGET_FINISH ? 1 : 0;
    p.fixed_priority = (flags & PGX_PLAN_FIXED_PRIORITY) ? 1 : 0;
    p.path_xy = path_xy;
    p.arrival = arrival;
    p.priority_out = priority_out;
    PGX_HIP(swap ? pgx::launch_pibt_swap_plan(p, s) : pgx::launch_pibt_plan(p, s));
    return PGX_OK;
}

int pgx_pibt_plan(pgx_env* e, int32_t flags, int32_t horizon, const int32_t* priority, void* actions, int32_t action_dtype,
                  int32_t* path_xy, int32_t* arrival, int32_t* priority_out, void* stream) {
    return pibt_plan_entry("pgx_pibt_plan", false, e, flags, horizon, priority, actions, action_dtype, path_xy, arrival,
                           priority_out, stream);
}

int pgx_pibt_swap_plan(pgx_env* e, int32_t flags, int32_t horizon, const int32_t* priority, void* actions,
                       int32_t action_dtype, int32_t* path_xy, int32_t* arrival, int32_t* priority_out, void* stream) {
    return pibt_plan_entry("pgx_pibt_swap_plan", true, e, flags, horizon, priority, actions, action_dtype, path_xy, arrival,
                           priority_out, stream);
}

// ---- windowed cooperative A* (docs/SPEC.md S28) -------------------------------------------------------------
int pgx_whca_plan(pgx_env* e, int32_t flags, int32_t horizon, const int32_t* priority, void* actions, int32_t action_dtype,
                  int32_t* path_xy, int32_t* arrival, int32_t* failed, void* stream) {
    static const char who[] = "pgx_whca_plan";
    // the argument checks come first and need no device
    if (!actions) return fail_msg(PGX_E_INVALID, "%s: actions is null", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    if (horizon < 1 || horizon > PGX_MAX_WHCA_HORIZON)
        return fail_msg(PGX_E_INVALID, "%s: horizon %d is outside 1..%d", who, horizon, PGX_MAX_WHCA_HORIZON);
    if (const int rc = check_action_dtype(who, action_dtype)) return rc;
    static const size_t action_bytes[3] = {1, 4, 8};
    if (const int rc = check_aligned(who, "actions", actions, action_bytes[action_dtype])) return rc;
    if (const int rc = check_aligned(who, "priority", priority, 4)) return rc;
    if (const int rc = check_aligned(who, "path_xy", path_xy, 4)) return rc;
    if (const int rc = check_aligned(who, "arrival", arrival, 4)) return rc;
    if (const int rc = check_aligned(who, "failed", failed, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::CostToGoParams cp{};
    if (const int rc = cost_to_go_cache(e, s, who, &cp)) return rc;
    PGX_HIP(pgx::launch_cost_to_go_refresh(cp, s));    // once: the fields are the heuristic of every agent's search
    pgx::WhcaParams p{};
    static_cast<pgx::StateView&>(p) = cp;
    p.action_dtype = action_dtype;
    p.cell_bytes = cp.cell_bytes;
    p.horizon = horizon;
    p.finish = e->cfg.on_target == PGX_ON_TARGET_FINISH ? 1 : 0;
    p.field = cp.field;
    p.priority = priority;
    p.actions = actions;
    p.path_xy = path_xy;
    p.arrival = arrival;
    p.failed = failed;
    PGX_HIP(pgx::launch_whca(p, s));
    return PGX_OK;
}

// ---- plan repair (docs/SPEC.md S29): chosen agents are replanned around the paths the others keep -------------------
int pgx_repair_plan(pgx_env* e, int32_t flags, int32_t horizon, const int32_t* paths, const uint8_t* replan,
                    const int32_t* priority, void* actions, int32_t action_dtype, int32_t* path_xy, int32_t* arrival,
                    int32_t* failed, int32_t* replanned, void* stream) {
    static const char who[] = "pgx_repair_plan";
    // the argument checks come first and need no device
    if (!paths) return fail_msg(PGX_E_INVALID, "%s: paths is null", who);
    if (!actions) return fail_msg(PGX_E_INVALID, "%s: actions is null", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    if (horizon < 1 || horizon > PGX_MAX_WHCA_HORIZON)
        return fail_msg(PGX_E_INVALID, "%s: horizon %d is outside 1..%d", who, horizon, PGX_MAX_WHCA_HORIZON);
    if (const int rc = check_action_dtype(who, action_dtype)) return rc;
    static const size_t action_bytes[3] = {1, 4, 8};
    if (const int rc = check_aligned(who, "actions", actions, action_bytes[action_dtype])) return rc;
    if (const int rc = check_aligned(who, "paths", paths, 4)) return rc;
    if (const int rc = check_aligned(who, "priority", priority, 4)) return rc;
    if (const int rc = check_aligned(who, "path_xy", path_xy, 4)) return rc;
    if (const int rc = check_aligned(who, "arrival", arrival, 4)) return rc;
    if (const int rc = check_aligned(who, "failed", failed, 4)) return rc;
    if (const int rc = check_aligned(who, "replanned", replanned, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    // S28's LDS formula, and nothing above it: the engine's largest env at the longest horizon fits one workgroup
    if (pgx::repair_lds_bytes(e->cfg.num_agents, horizon) > (size_t)160 * 1024)
        return fail_msg(PGX_E_INVALID, "%s: %d agents at horizon %d need %zu bytes of LDS, more than a workgroup has", who,
                        e->cfg.num_agents, horizon, pgx::repair_lds_bytes(e->cfg.num_agents, horizon));
    hipStream_t s = (hipStream_t)stream;
    pgx::CostToGoParams cp{};
    if (const int rc = cost_to_go_cache(e, s, who, &cp)) return rc;
    PGX_HIP(pgx::launch_cost_to_go_refresh(cp, s));    // once: the fields are the heuristic of every agent's search
    pgx::RepairParams p{};
    static_cast<pgx::StateView&>(p) = cp;
    p.action_dtype = action_dtype;
    p.cell_bytes = cp.cell_bytes;
    p.horizon = horizon;
    p.finish = e->cfg.on_target == PGX_ON_TARGET_FINISH ? 1 : 0;
    p.field = cp.field;
    p.priority = priority;
    p.actions = actions;
    p.path_xy = path_xy;
    p.arrival = arrival;
    p.failed = failed;
    p.paths = paths;
    p.replan = replan;
    p.replanned = replanned;
    PGX_HIP(pgx::launch_repair(p, s));
    return PGX_OK;
}

// ---- collision shielding (docs/SPEC.md S15) ---------------------------------------------------------------
int pgx_shield_actions(pgx_env* e, int32_t flags, const void* scores, int32_t score_dtype, const int32_t* priority,
                       void* actions, int32_t action_dtype, int32_t* next_xy, uint8_t* overridden, void* stream) {
    static const char who[] = "pgx_shield_actions";
    // the argument checks come first and need no device
    if (!scores) return fail_msg(PGX_E_INVALID, "%s: scores is null", who);
    if (!actions) return fail_msg(PGX_E_INVALID, "%s: actions is null", who);
    if (const int rc = check_flags(who, flags, PGX_SHIELD_TIE_DISTANCE)) return rc;
    static_assert(PGX_SCORES_F32 == pgx::SCORES_F32 && PGX_SCORES_F16 == pgx::SCORES_F16 &&
                      PGX_SCORES_BF16 == pgx::SCORES_BF16, "the kernels' score codes are the header's");
    if (score_dtype != PGX_SCORES_F32 && score_dtype != PGX_SCORES_F16 && score_dtype != PGX_SCORES_BF16)
        return fail_msg(PGX_E_INVALID, "%s: bad score_dtype %d", who, score_dtype);
    if (const int rc = check_action_dtype(who, action_dtype)) return rc;
    static const size_t action_bytes[3] = {1, 4, 8};
    if (const int rc = check_aligned(who, "scores", scores, score_dtype == PGX_SCORES_F32 ? 4 : 2)) return rc;
    if (const int rc = check_aligned(who, "actions", actions, action_bytes[action_dtype])) return rc;
    if (const int rc = check_aligned(who, "priority", priority, 4)) return rc;
    if (const int rc = check_aligned(who, "next_xy", next_xy, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::ShieldParams p{};
    if (flags & PGX_SHIELD_TIE_DISTANCE) {
        pgx::CostToGoParams cp{};
        if (const int rc = cost_to_go_cache(e, s, who, &cp)) return rc;
        PGX_HIP(pgx::launch_cost_to_go_refresh(cp, s));
        static_cast<pgx::StateView&>(p) = cp;
        p.cell_bytes = cp.cell_bytes;
        p.field = cp.field;
        p.tie_distance = 1;
    } else {
        static_cast<pgx::StateView&>(p) = state_view(e);   // no cache, no allocation: one launch
    }
    p.action_dtype = action_dtype;
    p.priority = priority;
    p.actions = actions;
    p.next_xy = next_xy;
    p.score_dtype = score_dtype;
    p.scores = scores;
    p.overridden = overridden;
    PGX_HIP(pgx::launch_shield(p, s));
    return PGX_OK;
}

// ---- move outcomes (docs/SPEC.md S17) -----------------------------------------------------------------------
int pgx_move_outcomes(pgx_env* e, const void* actions, int32_t action_dtype, int32_t flags, int32_t* next_xy,
                      uint8_t* outcome, int32_t* blocker, int32_t* counts, void* stream) {
    static const char who[] = "pgx_move_outcomes";
    // the argument checks come first and need no device
    if (!actions) return fail_msg(PGX_E_INVALID, "%s: actions is null", who);
    if (!next_xy && !outcome && !blocker && !counts) return fail_msg(PGX_E_INVALID, "%s: every output is null", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    if (const int rc = check_action_dtype(who, action_dtype)) return rc;
    static const size_t action_bytes[3] = {1, 4, 8};
    if (const int rc = check_aligned(who, "actions", actions, action_bytes[action_dtype])) return rc;
    if (const int rc = check_aligned(who, "next_xy", next_xy, 4)) return rc;
    if (const int rc = check_aligned(who, "blocker", blocker, 4)) return rc;
    if (const int rc = check_aligned(who, "counts", counts, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    static_assert(PGX_COLLISION_PRIORITY == pgx::COLLISION_PRIORITY && PGX_COLLISION_BLOCK_BOTH == pgx::COLLISION_BLOCK_BOTH &&
                      PGX_COLLISION_SOFT == pgx::COLLISION_SOFT, "the kernels' collision codes are the header's");
    pgx::OutcomeParams p{state_view(e)};
    p.collision = e->cfg.collision_system;
    p.all_stay = e->cfg.soft_vertex_rule == PGX_SOFT_ALL_STAY ? 1 : 0;
    p.action_dtype = action_dtype;
    p.actions = actions;
    p.next_xy = next_xy;
    p.outcome = outcome;
    p.blocker = blocker;
    p.counts = counts;
    PGX_HIP(pgx::launch_move_outcomes(p, (hipStream_t)stream));
    return PGX_OK;
}

// ---- direction-to-goal planes (docs/SPEC.md S14) ----------------------------------------------------------
int pgx_goal_directions(pgx_env* e, int32_t flags, void* out, int32_t format, void* stream) {
    static const char who[] = "pgx_goal_directions";
    // the argument checks come first and need no device
    if (!out) return fail_msg(PGX_E_INVALID, "%s: out is null", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    static_assert(PGX_DIRECTIONS_F32 == pgx::DIRECTIONS_F32 && PGX_DIRECTIONS_U8 == pgx::DIRECTIONS_U8 &&
                      PGX_DIRECTIONS_BITS == pgx::DIRECTIONS_BITS, "the kernels' format codes are the header's");
    if (format != PGX_DIRECTIONS_F32 && format != PGX_DIRECTIONS_U8 && format != PGX_DIRECTIONS_BITS)
        return fail_msg(PGX_E_INVALID, "%s: bad format %d", who, format);
    if (format == PGX_DIRECTIONS_F32)
        if (const int rc = check_aligned(who, "a float32 out", out, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::CostToGoParams p{};
    if (const int rc = cost_to_go_cache(e, s, who, &p)) return rc;
    PGX_HIP(pgx::launch_goal_directions(p, out, format, s));
    return PGX_OK;
}

// ---- path-to-goal planes and sub-goals (docs/SPEC.md S22) -------------------------------------------------
int pgx_goal_paths(pgx_env* e, int32_t flags, int32_t steps, int32_t format, void* planes, int8_t* subgoal, int32_t* length,
                   void* stream) {
    static const char who[] = "pgx_goal_paths";
    // the argument checks come first and need no device
    if (!planes && !subgoal && !length)
        return fail_msg(PGX_E_INVALID, "%s: planes, subgoal and length are all null", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    static_assert(PGX_PATHS_F32 == pgx::PATHS_F32 && PGX_PATHS_U8 == pgx::PATHS_U8 && PGX_PATHS_ROWS == pgx::PATHS_ROWS,
                  "the kernels' format codes are the header's");
    if (format != PGX_PATHS_F32 && format != PGX_PATHS_U8 && format != PGX_PATHS_ROWS)
        return fail_msg(PGX_E_INVALID, "%s: bad format %d", who, format);
    static_assert(PGX_MAX_PATH_STEPS == (2 * PGX_MAX_OBS_RADIUS + 1) * (2 * PGX_MAX_OBS_RADIUS + 1) - 1,
                  "the largest window's cells but the centre");
    if (steps < 0 || steps > PGX_MAX_PATH_STEPS)
        return fail_msg(PGX_E_INVALID, "%s: steps %d is outside 0..%d (0: no cap)", who, steps, PGX_MAX_PATH_STEPS);
    if (format != PGX_PATHS_U8)
        if (const int rc = check_aligned(who, format == PGX_PATHS_F32 ? "a float32 planes" : "a rows planes", planes, 4)) return rc;
    if (const int rc = check_aligned(who, "length", length, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::GoalPathParams p{};
    if (const int rc = cost_to_go_cache(e, s, who, &p)) return rc;  // (fills the CostToGoParams base of p)
    const int32_t w = 2 * e->cfg.obs_radius + 1;
    p.format = format;
    p.cap = steps == 0 || steps > w * w - 1 ? w * w - 1 : steps;   // the walk's trip count: no field can exceed it
    p.planes = planes;
    p.subgoal = subgoal;
    p.length = length;
    PGX_HIP(pgx::launch_goal_paths(p, s));
    return PGX_OK;
}

// ---- agent forecasts (docs/SPEC.md S24) ---------------------------------------------------------------------
int pgx_agent_forecasts(pgx_env* e, int32_t steps, int32_t format, int32_t flags, void* planes, int16_t* cells, void* stream) {
    static const char who[] = "pgx_agent_forecasts";
    // the argument checks come first and need no device
    if (!cells) return fail_msg(PGX_E_INVALID, "%s: cells is null", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    static_assert(PGX_FORECAST_F32 == pgx::FORECAST_F32 && PGX_FORECAST_U8 == pgx::FORECAST_U8 &&
                      PGX_FORECAST_ROWS == pgx::FORECAST_ROWS, "the kernels' format codes are the header's");
    if (format != PGX_FORECAST_F32 && format != PGX_FORECAST_U8 && format != PGX_FORECAST_ROWS)
        return fail_msg(PGX_E_INVALID, "%s: bad format %d", who, format);
    if (steps < 1 || steps > PGX_MAX_FORECAST_STEPS)
        return fail_msg(PGX_E_INVALID, "%s: steps %d is outside 1..%d", who, steps, PGX_MAX_FORECAST_STEPS);
    if (format != PGX_FORECAST_U8)
        if (const int rc = check_aligned(who, format == PGX_FORECAST_F32 ? "a float32 planes" : "a rows planes", planes, 4)) return rc;
    if (const int rc = check_aligned(who, "cells", cells, 2)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::ForecastParams p{};
    if (const int rc = cost_to_go_cache(e, s, who, &p)) return rc;  // (fills the CostToGoParams base of p)
    p.format = format;
    p.steps = steps;
    p.planes = planes;
    p.cells = cells;
    PGX_HIP(pgx::launch_agent_forecasts(p, s));
    return PGX_OK;
}

// ---- blocking counts (docs/SPEC.md S25) ---------------------------------------------------------------------
int pgx_blocking(pgx_env* e, int32_t inflation, int32_t flags, int32_t* count, int32_t* blocked_by, void* stream) {
    static const char who[] = "pgx_blocking";
    // the argument checks come first and need no device
    if (!count && !blocked_by) return fail_msg(PGX_E_INVALID, "%s: count and blocked_by are both null", who);
    if (const int rc = check_flags(who, flags, PGX_BLOCKING_ON_TARGET)) return rc;
    if (inflation < 1 || inflation > PGX_MAX_BLOCKING_INFLATION)
        return fail_msg(PGX_E_INVALID, "%s: inflation %d is outside 1..%d", who, inflation, PGX_MAX_BLOCKING_INFLATION);
    if (const int rc = check_aligned(who, "count", count, 4)) return rc;
    if (const int rc = check_aligned(who, "blocked_by", blocked_by, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::BlockingParams p{};
    if (const int rc = cost_to_go_cache(e, s, who, &p)) return rc;  // (fills the CostToGoParams base of p)
    p.inflation = inflation;
    p.on_target = (flags & PGX_BLOCKING_ON_TARGET) ? 1 : 0;
    p.count = count;
    p.blocked_by = blocked_by;
    PGX_HIP(pgx::launch_blocking(p, s));
    return PGX_OK;
}

// ---- path conflicts (docs/SPEC.md S26) ------------------------------------------------------------------------
int pgx_path_conflicts(pgx_env* e, const void* paths, int32_t layout, int32_t steps, int32_t flags, int32_t* first_step,
                       int32_t* partner, uint8_t* kind, int32_t* count, void* stream) {
    static const char who[] = "pgx_path_conflicts";
    // the argument checks come first and need no device
    static_assert(PGX_CONFLICT_PATHS_PLAN == pgx::CONFLICT_PATHS_PLAN && PGX_CONFLICT_PATHS_CELLS == pgx::CONFLICT_PATHS_CELLS &&
                      PGX_CONFLICT_VERTEX == pgx::CONFLICT_VERTEX && PGX_CONFLICT_EDGE == pgx::CONFLICT_EDGE &&
                      PGX_CONFLICT_FOLLOW == pgx::CONFLICT_FOLLOW, "the kernel's layout and kind codes are the header's");
    static_assert(PGX_MAX_CONFLICT_STEPS == PGX_MAX_PLAN_HORIZON, "a whole plan can be checked");
    constexpr int32_t kinds = PGX_CONFLICT_VERTEX | PGX_CONFLICT_EDGE | PGX_CONFLICT_FOLLOW;
    if (!paths) return fail_msg(PGX_E_INVALID, "%s: paths is null", who);
    if (!first_step && !partner && !kind && !count) return fail_msg(PGX_E_INVALID, "%s: every output is null", who);
    if (steps < 1 || steps > PGX_MAX_CONFLICT_STEPS)
        return fail_msg(PGX_E_INVALID, "%s: steps %d is outside 1..%d", who, steps, PGX_MAX_CONFLICT_STEPS);
    if (layout != PGX_CONFLICT_PATHS_PLAN && layout != PGX_CONFLICT_PATHS_CELLS)
        return fail_msg(PGX_E_INVALID, "%s: bad layout %d", who, layout);
    if (const int rc = check_flags(who, flags, kinds | PGX_CONFLICT_STAY | PGX_CONFLICT_VANISH)) return rc;
    if (!(flags & kinds)) return fail_msg(PGX_E_INVALID, "%s: flags 0x%x name no conflict kind", who, flags);
    if ((flags & PGX_CONFLICT_STAY) && (flags & PGX_CONFLICT_VANISH))
        return fail_msg(PGX_E_INVALID, "%s: flags 0x%x set both PGX_CONFLICT_STAY and PGX_CONFLICT_VANISH", who, flags);
    if (const int rc = check_aligned(who, layout == PGX_CONFLICT_PATHS_PLAN ? "a plan-layout paths" : "a cells-layout paths",
                                     paths, layout == PGX_CONFLICT_PATHS_PLAN ? 4 : 2)) return rc;
    if (const int rc = check_aligned(who, "first_step", first_step, 4)) return rc;
    if (const int rc = check_aligned(who, "partner", partner, 4)) return rc;
    if (const int rc = check_aligned(who, "count", count, 4)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    pgx::ConflictParams p{state_view(e)};   // no cache, no allocation: one launch
    p.paths = paths;
    p.layout = layout;
    p.steps = steps;
    p.kinds = flags & kinds;
    p.vanish = (flags & PGX_CONFLICT_VANISH) ? 1 : (flags & PGX_CONFLICT_STAY) ? 0 : e->cfg.on_target == PGX_ON_TARGET_FINISH;
    p.first_step = first_step;
    p.partner = partner;
    p.kind = kind;
    p.count = count;
    PGX_HIP(pgx::launch_path_conflicts(p, (hipStream_t)stream));
    return PGX_OK;
}

// ---- agent tokens (docs/SPEC.md S21) ------------------------------------------------------------------------
int64_t pgx_agent_tokens_length(int32_t obs_radius, int32_t slots) {
    static const char who[] = "pgx_agent_tokens_length";
    if (obs_radius < 1 || obs_radius > PGX_MAX_OBS_RADIUS)
        return fail_msg(PGX_E_INVALID, "%s: obs_radius %d is outside 1..%d", who, obs_radius, PGX_MAX_OBS_RADIUS);
    if (slots < 1 || slots > PGX_MAX_TOKEN_SLOTS)
        return fail_msg(PGX_E_INVALID, "%s: slots %d is outside 1..%d", who, slots, PGX_MAX_TOKEN_SLOTS);
    const int64_t w = 2 * (int64_t)obs_radius + 1;
    return w * w + (int64_t)PGX_TOKEN_SLOT_LEN * slots;
}

int pgx_agent_tokens(pgx_env* e, int32_t slots, int32_t length, int32_t flags, const int8_t* history, uint8_t* tokens,
                     void* stream) {
    static const char who[] = "pgx_agent_tokens";
    // the argument checks come first and need no device (the handle's radius is host memory)
    if (!e) return fail_msg(PGX_E_INVALID, "%s: null handle", who);
    if (!tokens) return fail_msg(PGX_E_INVALID, "%s: tokens is null", who);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    if (slots < 1 || slots > PGX_MAX_TOKEN_SLOTS)
        return fail_msg(PGX_E_INVALID, "%s: slots %d is outside 1..%d", who, slots, PGX_MAX_TOKEN_SLOTS);
    const int64_t l0 = pgx_agent_tokens_length(e->cfg.obs_radius, slots);
    static_assert((2 * PGX_MAX_OBS_RADIUS + 1) * (2 * PGX_MAX_OBS_RADIUS + 1) + PGX_TOKEN_SLOT_LEN * PGX_MAX_TOKEN_SLOTS <=
                      PGX_MAX_TOKEN_LENGTH, "the longest row fits the largest length");
    if (length < l0 || length > PGX_MAX_TOKEN_LENGTH)
        return fail_msg(PGX_E_INVALID, "%s: length %d is outside %lld..%d (obs_radius %d, %d slots)", who, length, (long long)l0,
                        PGX_MAX_TOKEN_LENGTH, e->cfg.obs_radius, slots);
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::TokenParams p{};
    if (const int rc = cost_to_go_cache(e, s, who, &p)) return rc;  // (fills the CostToGoParams base of p)
    p.slots = slots;
    p.length = length;
    p.history = history;
    p.tokens = tokens;
    PGX_HIP(pgx::launch_agent_tokens(p, s));
    return PGX_OK;
}

// ---- policy input (docs/SPEC.md S18) ------------------------------------------------------------------------
int pgx_policy_input(pgx_env* e, const int32_t* channels, int32_t num_channels, int32_t dtype, void* out, void* stream) {
    static const char who[] = "pgx_policy_input";
    // the argument checks come first and need no device
    if (!out) return fail_msg(PGX_E_INVALID, "%s: out is null", who);
    if (!channels) return fail_msg(PGX_E_INVALID, "%s: channels is null", who);
    if (num_channels < 1 || num_channels > PGX_NUM_CHANNELS)
        return fail_msg(PGX_E_INVALID, "%s: num_channels %d is outside 1..%d", who, num_channels, PGX_NUM_CHANNELS);
    static_assert(PGX_NUM_CHANNELS == pgx::POLICY_CHANNELS && PGX_CHANNEL_OBSTACLES == 0 && PGX_CHANNEL_AGENTS == 1 &&
                      PGX_CHANNEL_TARGET == 2 && PGX_CHANNEL_OTHER_GOALS == 3 && PGX_CHANNEL_UP == 4 && PGX_CHANNEL_DOWN == 5 &&
                      PGX_CHANNEL_LEFT == 6 && PGX_CHANNEL_RIGHT == 7, "channel code k is bit k of the kernel's cell bytes");
    uint32_t codes = 0, need = 0;
    for (int c = 0; c < num_channels; ++c) {
        const int32_t k = channels[c];
        if (k < 0 || k >= PGX_NUM_CHANNELS)
            return fail_msg(PGX_E_INVALID, "%s: channels[%d] = %d is outside 0..%d", who, c, k, PGX_NUM_CHANNELS - 1);
        if (need & (1u << k)) return fail_msg(PGX_E_INVALID, "%s: channels[%d] = %d is given twice", who, c, k);
        need |= 1u << k;
        codes |= (uint32_t)k << (4 * c);
    }
    static_assert(PGX_OBS_F32 == pgx::POLICY_INPUT_F32 && PGX_OBS_U8 == pgx::POLICY_INPUT_U8 &&
                      PGX_OBS_BF16 == pgx::POLICY_INPUT_BF16 && PGX_OBS_F16 == pgx::POLICY_INPUT_F16,
                  "the kernel's dtype codes are the header's");
    if (dtype != PGX_OBS_F32 && dtype != PGX_OBS_U8 && dtype != PGX_OBS_BF16 && dtype != PGX_OBS_F16)
        return fail_msg(PGX_E_INVALID, "%s: bad dtype %d", who, dtype);
    if (const int rc = check_aligned(who, "out", out, (size_t)obs_elem_bytes(dtype))) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    pgx::PolicyInputParams p{};
    if (need & 0xF0u) {
        if (const int rc = cost_to_go_cache(e, s, who, &p)) return rc;  // (fills the CostToGoParams base of p)
    } else {
        static_cast<pgx::StateView&>(p) = state_view(e);   // no cache, no allocation: one launch
    }
    p.num_channels = num_channels;
    p.dtype = dtype;
    p.codes = codes;
    p.need = need;
    p.one = dtype == PGX_OBS_F32 ? 0x3F800000u : dtype == PGX_OBS_BF16 ? 0x3F80u : dtype == PGX_OBS_F16 ? 0x3C00u : 1u;
    p.planes = out;
    PGX_HIP(pgx::launch_policy_input(p, s));
    return PGX_OK;
}

// ---- global state (docs/SPEC.md S20) ------------------------------------------------------------------------
namespace {
// The argument checks of pgx_global_state, in pgx_policy_input's order, then the id-range rule for `num_agents` agents;
// fills the kernel's picture of the channel list.
int global_state_args(int32_t num_agents, const int32_t* channels, int32_t num_channels, int32_t dtype, const void* out,
                      uint32_t* codes_out, uint32_t* need_out) {
    static const char who[] = "pgx_global_state";
    if (!out) return fail_msg(PGX_E_INVALID, "%s: out is null", who);
    if (!channels) return fail_msg(PGX_E_INVALID, "%s: channels is null", who);
    if (num_channels < 1 || num_channels > PGX_NUM_GLOBAL_CHANNELS)
        return fail_msg(PGX_E_INVALID, "%s: num_channels %d is outside 1..%d", who, num_channels, PGX_NUM_GLOBAL_CHANNELS);
    static_assert(PGX_NUM_GLOBAL_CHANNELS == pgx::GLOBAL_CHANNELS && PGX_GLOBAL_OBSTACLES == 0 && PGX_GLOBAL_AGENTS == 1 &&
                      PGX_GLOBAL_TARGETS == 2 && PGX_GLOBAL_AGENT_IDS == 3 && PGX_GLOBAL_TARGET_IDS == 4,
                  "codes 0..2 are bits of the kernel's cell bytes, 3 and 4 its id planes");
    static_assert(PGX_GLOBAL_BAND_CELLS == pgx::GLOBAL_BAND_CELLS && PGX_GLOBAL_BAND_CELLS >= PGX_MAX_SIDE,
                  "the header publishes the kernel's band, which holds a row of the widest map");
    uint32_t codes = 0, need = 0;
    for (int c = 0; c < num_channels; ++c) {
        const int32_t k = channels[c];
        if (k < 0 || k >= PGX_NUM_GLOBAL_CHANNELS)
            return fail_msg(PGX_E_INVALID, "%s: channels[%d] = %d is outside 0..%d", who, c, k, PGX_NUM_GLOBAL_CHANNELS - 1);
        if (need & (1u << k)) return fail_msg(PGX_E_INVALID, "%s: channels[%d] = %d is given twice", who, c, k);
        need |= 1u << k;
        codes |= (uint32_t)k << (4 * c);
    }
    if (dtype != PGX_OBS_F32 && dtype != PGX_OBS_U8 && dtype != PGX_OBS_BF16 && dtype != PGX_OBS_F16)
        return fail_msg(PGX_E_INVALID, "%s: bad dtype %d", who, dtype);
    if (const int rc = check_aligned(who, "out", out, (size_t)obs_elem_bytes(dtype))) return rc;
    // an id is index + 1 <= num_agents: uint8 holds 255, bfloat16 every integer up to 256, float16 up to 2048
    const int32_t limit = dtype == PGX_OBS_U8 ? PGX_GLOBAL_ID_MAX_U8 : dtype == PGX_OBS_BF16 ? PGX_GLOBAL_ID_MAX_BF16 : PGX_MAX_AGENTS;
    if ((need & 0x18u) && num_agents > limit)
        return fail_msg(PGX_E_INVALID, "%s: an id channel in %s holds at most %d agents exactly, the env has %d", who,
                        dtype == PGX_OBS_U8 ? "uint8" : "bfloat16", limit, num_agents);
    *codes_out = codes;
    *need_out = need;
    return PGX_OK;
}
}  // namespace

int pgx_global_state_check(int32_t num_agents, const int32_t* channels, int32_t num_channels, int32_t dtype, const void* out) {
    uint32_t codes = 0, need = 0;
    return global_state_args(num_agents, channels, num_channels, dtype, out, &codes, &need);
}

int pgx_global_state(pgx_env* e, const int32_t* channels, int32_t num_channels, int32_t dtype, void* out, void* stream) {
    static const char who[] = "pgx_global_state";
    // the argument checks come first and need no device (the handle's agent count is host memory; a NULL handle has none)
    uint32_t codes = 0, need = 0;
    if (const int rc = global_state_args(e ? e->cfg.num_agents : 0, channels, num_channels, dtype, out, &codes, &need)) return rc;
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    pgx::GlobalStateParams p{};
    static_cast<pgx::StateView&>(p) = state_view(e);   // no cache, no allocation: one launch
    p.num_channels = num_channels;
    p.dtype = dtype;
    p.codes = codes;
    p.need = need;
    p.one = dtype == PGX_OBS_F32 ? 0x3F800000u : dtype == PGX_OBS_BF16 ? 0x3F80u : dtype == PGX_OBS_F16 ? 0x3C00u : 1u;
    p.planes = out;
    PGX_HIP(pgx::launch_global_state(p, (hipStream_t)stream));
    return PGX_OK;
}

int64_t pgx_cost_to_go_builds(pgx_env* e, void* stream) {
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_cost_to_go_builds", false)) return rc;
    if (!e->c2g) return 0;
    unsigned long long n = 0;
    PGX_HIP(hipMemcpyAsync(&n, e->c2g, sizeof n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    PGX_HIP(hipStreamSynchronize((hipStream_t)stream));
    return (int64_t)n;
}

// ---- neighbour lists (docs/SPEC.md S12) -----------------------------------------------------------------
int pgx_visible_agents(pgx_env* e, int32_t k, int32_t flags, int32_t* index, int8_t* offset, int32_t* count, void* stream) {
    static const char who[] = "pgx_visible_agents";
    DeviceGuard guard;
    if (const int rc = enter(guard, e, who, true)) return rc;
    if (k < 1 || k > PGX_MAX_NEIGHBOURS) return fail_msg(PGX_E_INVALID, "%s: k = %d is outside 1..%d", who, k, PGX_MAX_NEIGHBOURS);
    if (const int rc = check_flags(who, flags, 0)) return rc;
    if (!index) return fail_msg(PGX_E_INVALID, "%s: index is null", who);
    if (const int rc = check_aligned(who, "index", index, 4)) return rc;
    if (const int rc = check_aligned(who, "count", count, 4)) return rc;
    if (const int rc = check_aligned(who, "offset", offset, 2)) return rc;
    const pgx::StateView v = state_view(e);
    pgx::NeighbourParams p{v.batch, v.A, v.r, k, v.pos, v.active};
    p.index = index;
    p.offset = offset;
    p.count = count;
    PGX_HIP(pgx::launch_visible_agents(p, (hipStream_t)stream));
    return PGX_OK;
}

int pgx_set_targets(pgx_env* e, const int32_t* target_xy, const uint8_t* agent_mask, void* stream) {
    if (!e || !target_xy) return fail_msg(PGX_E_INVALID, "pgx_set_targets: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_set_targets", true)) return rc;
    PGX_HIP(pgx::launch_set_targets(target_xy, agent_mask, e->tgt, (size_t)e->cfg.batch * e->cfg.num_agents,
                                    e->cfg.obs_radius, (hipStream_t)stream));
    return PGX_OK;
}

int64_t pgx_bad_action_count(pgx_env* e, void* stream) {
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_bad_action_count", false)) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint32_t n = 0;
    PGX_HIP(hipMemcpyAsync(&n, e->bad_count, sizeof n, hipMemcpyDeviceToHost, s));
    PGX_HIP(hipStreamSynchronize(s));
    if (n) PGX_HIP(hipMemsetAsync(e->bad_count, 0, sizeof n, s));
    return (int64_t)n;
}

int pgx_set_metrics_buffers(pgx_env* e, float* metrics, uint8_t* episode_done) {
    if (!e) return fail_msg(PGX_E_INVALID, "pgx_set_metrics_buffers: null handle");
    e->metrics_out = metrics;
    e->episode_done = episode_done;
    return PGX_OK;
}

int pgx_observe(pgx_env* e, void* obs, void* stream) {
    if (!e || !obs) return fail_msg(PGX_E_INVALID, "pgx_observe: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_observe", true)) return rc;
    PGX_HIP(pgx::launch_step(observe_params(e, obs), e->geo, (hipStream_t)stream));
    return PGX_OK;
}

int pgx_time_observe(pgx_env* e, void* obs, int32_t reps, float* microseconds, void* stream) {
    return pgx_time_observe_pair(e, obs, nullptr, reps, microseconds, stream);
}

int pgx_time_observe_pair(pgx_env* e, void* obs, void* obs_alt, int32_t reps, float* microseconds, void* stream) {
    if (!e || !obs || !microseconds) return fail_msg(PGX_E_INVALID, "pgx_time_observe: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_time_observe", true)) return rc;
    if (reps < 1) reps = 3;
    // warm-up: first touch of the buffer(s)
    void* const two[2] = {obs, obs_alt ? obs_alt : obs};
    PGX_HIP(time_launches(observe_params(e, obs), e->geo, two, obs_alt ? 2 : 1, reps, (hipStream_t)stream, microseconds));
    return PGX_OK;
}

int pgx_xcd_tune(pgx_env* e, void* obs, void* obs_alt, int32_t rounds, float* us_equal, float* us_tuned, void* stream) {
    if (!e || !obs) return fail_msg(PGX_E_INVALID, "pgx_xcd_tune: null argument");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_xcd_tune", true)) return rc;
    if (!e->xcd_aware) {  // not an 8-XCD SPX device: there are no per-XCD shares to tune (identity mapping)
        if (us_equal) *us_equal = 0.f;
        if (us_tuned) *us_tuned = 0.f;
        return PGX_OK;
    }
    if (rounds < 1) rounds = 6;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = e->geo.multi_wave ? e->cfg.batch : (e->cfg.batch + e->geo.epw - 1) / e->geo.epw;
    const size_t nst = (size_t)blocks * 4;
    DevBuf<unsigned long long> stamps;
    PGX_HIP(stamps.alloc(nst * sizeof(unsigned long long)));
    std::vector<unsigned long long> host(nst);
    void* const two[2] = {obs, obs_alt ? obs_alt : obs};
    hipError_t err = hipSuccess;
    float best_w[8], w[8], best_us = 0.f, first_us = 0.f;
    for (int x = 0; x < 8; ++x) best_w[x] = w[x] = 0.125f;
    for (int round = 0; round <= rounds; ++round) {
        for (int x = 0; x < 8; ++x) e->xcd_w[x] = w[x];
        apply_xcd_shares(e);
        const pgx::StepParams p = observe_params(e, obs);
        // when each XCD is through with its share (per-workgroup end stamps of one launch) ...
        pgx::StepParams stamped = p;
        stamped.flags = (p.flags | 4u) & ~64u;
        stamped.dbg = stamps;
        err = hipMemsetAsync(stamps, 0, nst * sizeof(unsigned long long), s);
        if (err == hipSuccess) err = pgx::launch_step(stamped, e->geo, s);
        if (err == hipSuccess) err = hipMemcpyAsync(host.data(), stamps, nst * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        if (err != hipSuccess) break;
        unsigned long long t0 = ~0ull;
        for (int i = 0; i < blocks; ++i)
            if (host[(size_t)i * 4] && host[(size_t)i * 4] < t0) t0 = host[(size_t)i * 4];
        double f[8], mean = 0.0;
        for (int x = 0; x < 8; ++x) {
            unsigned long long last = t0;
            for (int i = e->geo.xcd_base[x]; i < e->geo.xcd_base[x] + e->geo.xcd_n[x]; ++i)
                if (host[(size_t)i * 4 + 3] > last) last = host[(size_t)i * 4 + 3];
            f[x] = (double)(last - t0);
            mean += f[x] / 8.0;
        }
        // ... and how long the launch takes with these shares: alternating between the two buffers as pgx_step's caller
        // does, always after the same prelude (the stamped launch and its read-back), two passes to settle, eight timed
        float us = 0.f;
        err = time_launches(p, e->geo, two, 2, 8, s, &us);
        if (err != hipSuccess) break;
        if (round == 0) first_us = us;
        if (round == 0 || us < best_us) {
            best_us = us;
            for (int x = 0; x < 8; ++x) best_w[x] = w[x];
        }
        if (getenv("PGX_DEBUG"))
            fprintf(stderr, "[pgx xcd] round %d: %.1f us; shares %d %d %d %d %d %d %d %d finished after %.0f %.0f %.0f %.0f %.0f %.0f %.0f %.0f us\n",
                    round, us, e->geo.xcd_n[0], e->geo.xcd_n[1], e->geo.xcd_n[2], e->geo.xcd_n[3], e->geo.xcd_n[4], e->geo.xcd_n[5],
                    e->geo.xcd_n[6], e->geo.xcd_n[7], f[0] / 100, f[1] / 100, f[2] / 100, f[3] / 100, f[4] / 100, f[5] / 100,
                    f[6] / 100, f[7] / 100);
        if (round == rounds) break;
        // half of the correction the finish times ask for (an XCD that got less work also finishes the rest faster)
        double sum = 0.0;
        for (int x = 0; x < 8; ++x) {
            const double v = f[x] > 0.0 ? (double)w[x] * (0.5 + 0.5 * mean / f[x]) : (double)w[x];
            w[x] = (float)(v < 0.10 ? 0.10 : v > 0.15 ? 0.15 : v);
            sum += w[x];
        }
        for (int x = 0; x < 8; ++x) w[x] = (float)(w[x] / sum);
    }
    for (int x = 0; x < 8; ++x) e->xcd_w[x] = best_w[x];
    apply_xcd_shares(e);
    PGX_HIP(err);
    if (us_equal) *us_equal = first_us;
    if (us_tuned) *us_tuned = best_us;
    return PGX_OK;
}

int pgx_get_state(pgx_env* e, int32_t* agent_xy, int32_t* target_xy, uint8_t* is_active, int32_t* elapsed,
                  uint8_t* occupancy, void* stream) {
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_get_state", true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const pgx_config& c = e->cfg;
    const size_t B = (size_t)c.batch, BA = B * c.num_agents;
    if (agent_xy || target_xy || is_active)
        PGX_HIP(pgx::launch_unpack_state(e->pos, e->tgt, e->active, agent_xy, target_xy, is_active, BA, c.obs_radius, s));
    if (elapsed) PGX_HIP(hipMemcpyAsync(elapsed, e->elapsed, B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (occupancy) {
        PGX_HIP(hipMemsetAsync(occupancy, 0, B * e->PH * e->PW, s));
        PGX_HIP(pgx::launch_occupancy(e->pos, e->active, occupancy, BA, c.num_agents, e->PH, e->PW, s));
    }
    return PGX_OK;
}

// Diagnostic only (not part of include/pogema_amd.h): copies the per-workgroup clock stamps of the last
// launch to the host; needs PGX_FLAGS bit 2 at pgx_create.  Synchronises the device.
int pgx_xcd_shares(pgx_env* e, int32_t* shares) {
    if (!e || !shares) return fail_msg(PGX_E_INVALID, "pgx_xcd_shares: null argument");
    for (int x = 0; x < 8; ++x) shares[x] = e->geo.xcd_n[x];
    return PGX_OK;
}

int pgx_get_geometry(const pgx_env* e, int32_t for_rollout, pgx_geometry* out) {
    if (!e || !out) return fail_msg(PGX_E_INVALID, "pgx_get_geometry: null argument");
    const pgx::StepGeometry& g = for_rollout ? e->geo_roll : e->geo;
    out->lanes_per_env = g.G;
    out->waves = g.waves * (g.pc ? 2 : 1);
    out->envs_per_wave = g.epw;
    out->multi_wave = g.big ? 2 : g.multi_wave ? 1 : 0;
    out->p16 = g.p16 ? 1 : 0;
    out->stagger = g.stagger;
    // the EFFECTIVE store flavour: the generic funnels of the lighter formats (uint8; bfloat16 / float16 with a
    // window below 7 cells or beyond the 16-bit row masks) know plain and nontemporal stores only -- sc1 runs as plain there
    {
        const int W = 2 * e->cfg.obs_radius + 1;
        const bool h16 = e->cfg.obs_dtype == PGX_OBS_BF16 || e->cfg.obs_dtype == PGX_OBS_F16;
        const bool all_flavours = e->cfg.obs_dtype == PGX_OBS_F32 || (h16 && g.p16 && W >= 7);
        out->store_policy = all_flavours ? g.store_policy : (g.store_policy == 1 ? 1 : 0);
    }
    out->state_stores = g.state_stores;
    out->grid = g.grid;
    out->lds_bytes = (int32_t)g.lds_bytes;
    out->for_rollout = for_rollout ? 1 : 0;
    out->xcd_aware = e->xcd_aware ? 1 : 0;
    return PGX_OK;
}

int pgx_debug_timestamps(pgx_env* e, unsigned long long* host_out, int64_t max_elems) {
    if (!e || !host_out) return fail_msg(PGX_E_INVALID, "pgx_debug_timestamps: null argument");
    if (!e->dbg) return fail_msg(PGX_E_STATE, "diagnostic stamps not enabled (PGX_FLAGS bit 2)");
    DeviceGuard guard;
    if (const int rc = enter(guard, e, "pgx_debug_timestamps", false)) return rc;
    PGX_HIP(hipDeviceSynchronize());
    const size_t n = std::min<size_t>(e->dbg_elems, (size_t)max_elems);
    PGX_HIP(hipMemcpy(host_out, e->dbg, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return (int)PGX_OK;
}

}  // extern "C"
