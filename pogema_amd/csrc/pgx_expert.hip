// pgx_expert.hip -- shortest-path expert (pgx_expert_actions, docs/SPEC.md "Shortest-path expert").
//
// For every agent: the 4-connected BFS distance from its cell to its target over the free cells of the H x W map
// (never the padding), and the first action (up, down, left, right order) that lowers it.  The search is bit-parallel
// and runs FROM the target: the visited set is a bitmap grown once per iteration by
//     v' = (v | v << 1 | v >> 1 | row above | row below) & free
// so after d iterations it holds exactly the cells at distance <= d.  The agent's bit appears in iteration d = its
// distance; its neighbours already in the previous set are the ones at distance d - 1 (the action).  A set that stops
// growing before the agent's bit appears means "no path".
//
// Two layouts, picked per configuration:
//   small  (H <= 64 and W <= 64): one workgroup per environment.  The free bitmap (and, with agents as obstacles, the
//          occupancy bitmap) is built in LDS once, one u64 row per map row.  A wave runs floor(64 / H) searches side by
//          side, one lane per map row; the rows above and below are a cross-lane shift.
//   large  (any other legal map, up to 1024 x 1024): one workgroup per (environment, agent).  The visited set lives in
//          LDS as rows of ceil(W / 32) words (128 KB at 1024 x 1024).  The search's free bitmap is staged next to it in
//          LDS once when both fit (up to ~1024 x 640); larger maps read obstacles through the L2 from the engine's
//          padded bitmap every iteration.  Each iteration only touches the visited set's bounding box grown by one
//          row / word.
// Both only read the engine state; nothing the next pgx_step reads is written.
#include "pgx_internal.h"

namespace pgx {
namespace {

// large layout: visited-set words one thread stages in VGPRs per iteration (every read of the old set precedes the first
// write).  8 covers maps up to 8192 words (1024 threads), e.g. 256 x 256; 32 every legal map (1024 x 1024 = 32768 words)
// at the price of a few spilled registers.
constexpr int EXPERT_WORDS_SMALL = 8, EXPERT_WORDS_BIG = 32;
// workgroups of one large-layout launch: 2^20 x 1024 lanes stays below 2^32 work-items; more slots loop in the kernel
constexpr size_t EXPERT_MAX_GRID = size_t(1) << 20;

__device__ __forceinline__ void store_action(void* actions, int action_dtype, size_t i, int a) {
    if (action_dtype == 0) static_cast<int8_t*>(actions)[i] = (int8_t)a;
    else if (action_dtype == 1) static_cast<int32_t*>(actions)[i] = a;
    else static_cast<int64_t*>(actions)[i] = a;
}

// 32 free-of-obstacle bits of unpadded row x, unpadded columns [32 c, 32 c + 32), from the padded bitmap of one env.
// Bits at or beyond W are cleared: the padding (border ring, `empty_outside=False` obstacles) is never traversed.
__device__ __forceinline__ uint32_t free_word(const uint32_t* __restrict__ bm, int x, int c, int r, int wpr, int W) {
    const uint32_t* row = bm + (size_t)(x + r) * wpr;
    const int col = 32 * c + r;              // padded column of bit 0
    const int w0 = col >> 5, sh = col & 31;
    uint32_t lo = row[w0];
    uint32_t obst = lo >> sh;
    if (sh && (w0 + 1) * 32 < W + r) obst |= row[w0 + 1] << (32 - sh);  // the next word holds map bits too
    const int n = W - 32 * c;                // map columns in this word
    const uint32_t mask = n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u);
    return ~obst & mask;
}

__device__ __forceinline__ bool padded_obstacle(const uint32_t* __restrict__ bm, int px, int py, int wpr) {
    return (bm[(size_t)px * wpr + (py >> 5)] >> (py & 31)) & 1u;
}

// ---------------------------------------------------------------------------------------------------------------
// small layout: H <= 64, W <= 64
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) expert_small_kernel(const uint32_t* __restrict__ obst,
                                                           const uint32_t* __restrict__ pos,
                                                           const uint32_t* __restrict__ tgt,
                                                           const uint8_t* __restrict__ active, int A, int H, int W,
                                                           int r, int wpr, int bmw, int with_agents,
                                                           void* __restrict__ actions, int action_dtype,
                                                           int32_t* __restrict__ distance) {
    __shared__ unsigned long long s_free[64];
    __shared__ unsigned long long s_occ[64];
    const int env = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t* bm = obst + (size_t)env * bmw;
    const size_t abase = (size_t)env * A;
    if (tid < 64) {
        unsigned long long f = 0ull;
        if (tid < H) {
            f = free_word(bm, tid, 0, r, wpr, W);
            if (W > 32) f |= (unsigned long long)free_word(bm, tid, 1, r, wpr, W) << 32;
        }
        s_free[tid] = f;
        s_occ[tid] = 0ull;
    }
    __syncthreads();
    if (with_agents) {
        for (int a = tid; a < A; a += blockDim.x) {
            if (!(active[abase + a] & ACTIVE_BIT)) continue;
            const uint32_t p = pos[abase + a];
            atomicOr(&s_occ[(int)(p >> 16) - r], 1ull << ((int)(p & 0xFFFFu) - r));
        }
        __syncthreads();
    }
    const int lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const int segs = 64 / H;                 // searches per wave
    const int seg = lane / H, row = lane - seg * H;
    const bool valid_lane = seg < segs;
    const unsigned long long seg_mask =
        H == 64 ? ~0ull : (valid_lane ? (((1ull << H) - 1ull) << (seg * H)) : 0ull);
    const unsigned long long free_row = valid_lane ? s_free[row] : 0ull;
    const unsigned long long occ_row = valid_lane ? s_occ[row] : 0ull;

    for (int first = wave * segs; first < A; first += waves * segs) {
        const int a = first + seg;
        const bool have = valid_lane && a < A;
        int ax = 0, ay = 0, tx = 0, ty = 0;
        bool act = false;
        if (have) {
            const uint32_t p = pos[abase + a], t = tgt[abase + a];
            ax = (int)(p >> 16) - r;
            ay = (int)(p & 0xFFFFu) - r;
            tx = (int)(t >> 16) - r;
            ty = (int)(t & 0xFFFFu) - r;
            act = (active[abase + a] & ACTIVE_BIT) != 0;
        }
        // the agent's own cell and its own target are never blocked by agents; obstacles still block them
        unsigned long long own = 0ull;
        if (row == ax) own |= 1ull << ay;
        if (row == tx) own |= 1ull << ty;
        const unsigned long long fr = free_row & ~(occ_row & ~own);
        unsigned long long v = (have && row == tx) ? ((1ull << ty) & fr) : 0ull;
        const bool agent_lane = have && row == ax;
        int dist = -1, action = 0;
        bool done = !have || !act;
        if (have && act && ax == tx && ay == ty) {
            dist = 0;
            done = true;
        }
        for (int d = 1; __ballot(!done) != 0ull; ++d) {
            unsigned long long up = __shfl(v, lane - 1);
            unsigned long long dn = __shfl(v, lane + 1);
            if (row == 0) up = 0ull;
            if (row == H - 1 || lane == 63) dn = 0ull;
            unsigned long long nv = (v | (v << 1) | (v >> 1) | up | dn) & fr;
            if (done) nv = v;
            const bool found_here = agent_lane && ((nv >> ay) & 1ull);
            const bool found = (__ballot(found_here) & seg_mask) != 0ull;
            const bool grew = (__ballot(nv != v) & seg_mask) != 0ull;
            if (!done && found && agent_lane) {
                dist = d;
                // neighbours in the previous set are at distance d - 1; the lowest action index wins
                if ((up >> ay) & 1ull) action = 1;
                else if ((dn >> ay) & 1ull) action = 2;
                else if (ay > 0 && ((v >> (ay - 1)) & 1ull)) action = 3;
                else action = 4;
            }
            if (found || !grew) done = true;
            v = nv;
        }
        if (agent_lane) {
            store_action(actions, action_dtype, abase + a, action);
            if (distance) distance[abase + a] = dist;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// large layout: one search per workgroup at a time, over the (environment, agent) slots
// ---------------------------------------------------------------------------------------------------------------
__global__ void occupancy_bits_kernel(const uint32_t* __restrict__ pos, const uint8_t* __restrict__ active,
                                      uint32_t* __restrict__ occ, int batch, int A, int H, int wn, int r) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)batch * A) return;
    if (!(active[i] & ACTIVE_BIT)) return;
    const size_t env = i / A;
    const uint32_t p = pos[i];
    const int x = (int)(p >> 16) - r, y = (int)(p & 0xFFFFu) - r;
    atomicOr(&occ[(env * H + x) * wn + (y >> 5)], 1u << (y & 31));
}

template <int K>
__global__ void __launch_bounds__(1024) expert_large_kernel(const uint32_t* __restrict__ obst,
                                                            const uint32_t* __restrict__ pos,
                                                            const uint32_t* __restrict__ tgt,
                                                            const uint8_t* __restrict__ active,
                                                            const uint32_t* __restrict__ occ, size_t total, int A,
                                                            int H, int W, int r, int wpr, int bmw, int wn, int staged,
                                                            void* __restrict__ actions, int action_dtype,
                                                            int32_t* __restrict__ distance) {
    extern __shared__ uint32_t s_vis[];      // [H][wn] visited set, then (staged) [H][wn] free cells of this search
    __shared__ int s_found, s_action;
    const int tid = threadIdx.x, nt = blockDim.x;
    // workgroups loop over the (env, agent) slots: batch * agents workgroups of up to 1024 lanes could pass the 2^32
    // work-items of one launch
    for (size_t slot = blockIdx.x; slot < total; slot += gridDim.x) {
        __syncthreads();                     // the previous slot's last reads of s_vis / s_found are done
        const size_t env = slot / A;
        const uint32_t* bm = obst + env * bmw;
        const uint32_t* oc = occ ? occ + env * (size_t)H * wn : nullptr;
        const uint32_t p = pos[slot], t = tgt[slot];
        const int ax = (int)(p >> 16) - r, ay = (int)(p & 0xFFFFu) - r;
        const int tx = (int)(t >> 16) - r, ty = (int)(t & 0xFFFFu) - r;
        const bool act = (active[slot] & ACTIVE_BIT) != 0;
        int dist = -1, action = 0;
        if (act && ax == tx && ay == ty) dist = 0;
        if (act && dist != 0) {
            uint32_t* s_free = s_vis + H * wn;
            // free cells of this search: obstacles from the padded bitmap, with the flag the other agents' cells
            const int awc = ay >> 5, twc = ty >> 5;
            const uint32_t abit = 1u << (ay & 31), tbit = 1u << (ty & 31);
            auto free_at = [&](int x, int c) {
                uint32_t f = free_word(bm, x, c, r, wpr, W);
                if (oc) {
                    uint32_t own = 0u;
                    if (x == ax && c == awc) own |= abit;
                    if (x == tx && c == twc) own |= tbit;
                    f &= ~(oc[x * wn + c] & ~own);
                }
                return f;
            };
            for (int i = tid; i < H * wn; i += nt) {
                s_vis[i] = 0u;
                if (staged) s_free[i] = free_at(i / wn, i % wn);
            }
            if (tid == 0) s_found = 0;
            __syncthreads();
            // seed: the target, unless an obstacle stands there (agents never block one's own target)
            if (tid == 0 && !padded_obstacle(bm, tx + r, ty + r, wpr)) s_vis[tx * wn + twc] = tbit;
            int r0 = tx, r1 = tx, c0 = twc, c1 = twc;  // bounding box of the visited set (rows, words)
            for (int d = 1;; ++d) {
                r0 = max(r0 - 1, 0);
                r1 = min(r1 + 1, H - 1);
                c0 = max(c0 - 1, 0);
                c1 = min(c1 + 1, wn - 1);
                const int bw = c1 - c0 + 1;
                const int n = (r1 - r0 + 1) * bw;
                __syncthreads();                 // the previous iteration's writes (and the seed) are visible
                uint32_t nw[K];
                bool changed = false;
    #pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int idx = tid + k * nt;
                    nw[k] = 0u;
                    if (idx < n) {
                        const int x = r0 + idx / bw, c = c0 + idx % bw;
                        const uint32_t* vr = s_vis + x * wn;
                        const uint32_t v = vr[c];
                        uint32_t g = v | (v << 1) | (v >> 1);
                        if (c > 0) g |= vr[c - 1] >> 31;
                        if (c + 1 < wn) g |= vr[c + 1] << 31;
                        if (x > 0) g |= vr[c - wn];
                        if (x + 1 < H) g |= vr[c + wn];
                        g &= staged ? s_free[x * wn + c] : free_at(x, c);
                        nw[k] = g;
                        changed |= g != v;
                        if (x == ax && c == awc && (g & abit)) {
                            // neighbours in the previous set are at distance d - 1; the lowest action index wins
                            int a;
                            if (ax > 0 && (s_vis[(ax - 1) * wn + awc] & abit)) a = 1;
                            else if (ax + 1 < H && (s_vis[(ax + 1) * wn + awc] & abit)) a = 2;
                            else if (ay > 0 && (s_vis[ax * wn + ((ay - 1) >> 5)] >> ((ay - 1) & 31) & 1u)) a = 3;
                            else a = 4;
                            s_action = a;
                            s_found = d;
                        }
                    }
                }
                const int any_changed = __syncthreads_or(changed ? 1 : 0);  // every read of the previous set is done
                if (s_found) {
                    dist = s_found;
                    action = s_action;
                    break;
                }
                if (!any_changed) break;
    #pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int idx = tid + k * nt;
                    if (idx < n) s_vis[(r0 + idx / bw) * wn + c0 + idx % bw] = nw[k];
                }
            }
        }
        if (tid == 0) {
            store_action(actions, action_dtype, slot, action);
            if (distance) distance[slot] = dist;
        }
    }
}

}  // namespace

bool expert_large_layout(int H, int W) { return H > 64 || W > 64; }

size_t expert_occupancy_words(int batch, int H, int W) {
    return expert_large_layout(H, W) ? (size_t)batch * H * ((W + 31) / 32) : 0;
}

// the free bitmap of a search is staged in LDS next to the visited set when both fit (maps up to ~1024 x 640)
bool expert_large_staged(int H, int W) { return (size_t)H * ((W + 31) / 32) * 8 <= 156 * 1024; }

size_t expert_large_lds(int H, int W) {
    return (size_t)H * ((W + 31) / 32) * sizeof(uint32_t) * (expert_large_staged(H, W) ? 2 : 1);
}

int expert_large_words(int H, int W) { return H * ((W + 31) / 32) <= 1024 * EXPERT_WORDS_SMALL ? EXPERT_WORDS_SMALL : EXPERT_WORDS_BIG; }

int expert_large_threads(int H, int W) {
    const int words = H * ((W + 31) / 32), k = expert_large_words(H, W);
    int nt = (words + k - 1) / k;
    nt = (nt + 63) / 64 * 64;
    return nt < 256 ? 256 : nt;              // <= 1024: H * ceil(W / 32) <= 32768 words
}

hipError_t launch_expert(const ExpertParams& e, hipStream_t stream) {
    const int wn = (e.W + 31) / 32;
    if (!expert_large_layout(e.H, e.W)) {
        // 4 waves per environment; a wave runs floor(64 / H) searches side by side
        const int waves = 4;
        hipLaunchKernelGGL(expert_small_kernel, dim3(e.batch), dim3(64 * waves), 0, stream, e.obst, e.pos, e.tgt,
                           e.active, e.A, e.H, e.W, e.r, e.wpr, e.bmw, e.with_agents, e.actions, e.action_dtype,
                           e.distance);
        return hipGetLastError();
    }
    if (e.with_agents) {
        const size_t words = (size_t)e.batch * e.H * wn;
        hipError_t err = hipMemsetAsync(e.occ, 0, words * sizeof(uint32_t), stream);
        if (err != hipSuccess) return err;
        const size_t n = (size_t)e.batch * e.A;
        hipLaunchKernelGGL(occupancy_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, e.pos,
                           e.active, e.occ, e.batch, e.A, e.H, wn, e.r);
        err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    const size_t lds = expert_large_lds(e.H, e.W);
    const int nt = expert_large_threads(e.H, e.W);
    auto kernel = expert_large_words(e.H, e.W) == EXPERT_WORDS_SMALL ? expert_large_kernel<EXPERT_WORDS_SMALL>
                                                                      : expert_large_kernel<EXPERT_WORDS_BIG>;
    const size_t total = (size_t)e.batch * e.A;
    const unsigned grid = (unsigned)(total < EXPERT_MAX_GRID ? total : EXPERT_MAX_GRID);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(nt), lds, stream, e.obst,
                       e.pos, e.tgt, e.active, e.with_agents ? e.occ : nullptr, total, e.A, e.H, e.W, e.r, e.wpr, e.bmw, wn,
                       expert_large_staged(e.H, e.W) ? 1 : 0, e.actions, e.action_dtype, e.distance);
    return hipGetLastError();
}

hipError_t prepare_expert(int H, int W) {
    if (!expert_large_layout(H, W)) return hipSuccess;
    // an attribute of the kernel function, shared by every handle: raise_lds_limit only ever raises it
    const void* fn = expert_large_words(H, W) == EXPERT_WORDS_SMALL
                         ? reinterpret_cast<const void*>(&expert_large_kernel<EXPERT_WORDS_SMALL>)
                         : reinterpret_cast<const void*>(&expert_large_kernel<EXPERT_WORDS_BIG>);
    return raise_lds_limit(fn, expert_large_lds(H, W));
}

}  // namespace pgx
