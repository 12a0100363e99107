// pgx_blocking.hip -- blocking counts (pgx_blocking, docs/SPEC.md S25).
//
// For every ordered pair (i, j) of active agents of one env with j in i's window: does i, where it stands, lengthen j's
// way to its target by at least `inflation` steps (or cut it off)?  With c = cell of i, s = cell of j, t = target of j and
// d0 = F_j[s] (pgx_cost2go.hip's cached field of j), i blocks j iff d0 is defined, s != c and no path from s to t of at
// most d0 + inflation - 1 steps exists on the map with c blocked.  The call refreshes the stale fields
// (launch_cost_to_go_refresh) and then counts:
//   1. the filter, exact: F_j[c] undefined or F_j[c] + |c - s|_1 > d0 means c is on no shortest path of j, a path of d0
//      steps avoids it and the pair is not blocked -- two field reads, no search;
//   2. every other eligible pair takes one bit-parallel BFS from s on a private free mask with the bit of c cleared (the
//      shared obstacle bitmap is only read), at most d0 + inflation - 1 levels, ended as soon as t is reached or a level
//      adds nothing.  Every loop is bounded by that level count or by an empty frontier, whatever a field holds.
// The two search layouts of pgx_expert.hip / pgx_cost2go.hip, with own copies of the helpers (those files stay untouched):
//   small (H <= 64 and W <= 64): one workgroup per env, one lane per map row and a 64-bit word per row, floor(64 / H)
//         searches per wave.  A wave owns the agents j = wave, wave + 4, ...; per j its lanes test 64 blockers i at a time
//         with the filter, and the survivors of the ballot are searched floor(64 / H) at a time.  No wave waits on another.
//   large (any other legal map): workgroups own contiguous ranges of (env, j) slots, scan each slot's blockers for
//         survivors of the filter and run one search at a time; the visited set lives in LDS, its bounding box grows one
//         row / word per level (the field build's band scheme).  Both field widths are read.
// The launch shape never depends on device data, so the call is capturable once the cache exists.
// How the counts are accumulated, by layout:
//   small: the workgroup holds the whole env, so count[] is summed in LDS (integer LDS atomics, order-independent) and both
//          outputs leave in plain stores: no global atomic, no zeroing launch.
//   large: the owner of slot (env, j) knows blocked_by[j] alone and stores it plainly; count[i] collects from the owners
//          of different j with integer atomicAdd into an output an earlier launch of the same call zeroed.  A second
//          gather pass in its place would repeat every search with the roles swapped.  Chosen by construction, not by a
//          comparison of two builds: docs/EXPERIMENTS.md has tools/time_blocking.py's figures and says what was not timed.
// The engine state the next pgx_step reads is only read; the cache and the two outputs are all that is written.
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr int BLK_SMALL_WAVES = 4;
constexpr int BLK_WORDS = 8;                    // large layout: visited-set words a thread stages per band (as the field build)
constexpr size_t BLK_MAX_GRID = 4096;           // large layout: workgroups; each owns a contiguous range of slots

// 32 free bits of unpadded row x, unpadded columns [32 c, 32 c + 32), bits at or beyond W cleared.  The same function as
// pgx_cost2go.hip's, which keeps its own copy too.
__device__ __forceinline__ uint32_t blk_free_word(const uint32_t* __restrict__ bm, int x, int c, int r, int wpr, int W) {
    const uint32_t* row = bm + (size_t)(x + r) * wpr;
    const int col = 32 * c + r;
    const int w0 = col >> 5, sh = col & 31;
    uint32_t obst = row[w0] >> sh;
    if (sh && (w0 + 1) * 32 < W + r) obst |= row[w0 + 1] << (32 - sh);
    const int n = W - 32 * c;
    const uint32_t mask = n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u);
    return ~obst & mask;
}

// ---------------------------------------------------------------------------------------------------------------
// small layout: H <= 64, W <= 64, u16 fields
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * BLK_SMALL_WAVES) blocking_small_kernel(BlockingParams p) {
    __shared__ unsigned long long s_free[64];
    __shared__ uint32_t s_pos[1024];         // the env's packed padded positions
    __shared__ uint8_t s_flag[1024];         // bit 0: active; bit 1: may block (active and, with on_target, on its target)
    __shared__ int s_count[1024];
    const int env = blockIdx.x, tid = threadIdx.x;
    const int H = p.H, W = p.W, HW = H * W, A = p.A, r = p.r;
    const uint32_t* bm = p.obst + (size_t)env * p.bmw;
    const size_t abase = (size_t)env * A;
    if (tid < 64) {
        unsigned long long f = 0ull;
        if (tid < H) {
            f = blk_free_word(bm, tid, 0, r, p.wpr, W);
            if (W > 32) f |= (unsigned long long)blk_free_word(bm, tid, 1, r, p.wpr, W) << 32;
        }
        s_free[tid] = f;
    }
    for (int a = tid; a < A; a += blockDim.x) {
        const uint32_t pp = p.pos[abase + a];
        const bool act = p.active[abase + a] & ACTIVE_BIT;
        s_pos[a] = pp;
        s_flag[a] = act ? ((!p.on_target || pp == p.tgt[abase + a]) ? 3 : 1) : 0;
        s_count[a] = 0;
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int segs = 64 / H;                 // searches per wave
    const int seg = lane / H, row = lane - seg * H;
    const bool valid_lane = seg < segs;
    const unsigned long long seg_mask =
        H == 64 ? ~0ull : (valid_lane ? (((1ull << H) - 1ull) << (seg * H)) : 0ull);
    const unsigned long long fr0 = valid_lane ? s_free[row] : 0ull;
    const uint16_t* field = static_cast<const uint16_t*>(p.field);

    for (int j = wave; j < A; j += BLK_SMALL_WAVES) {   // (wave-uniform: the ballots and shuffles below are whole-wave)
        int by = 0;
        if (s_flag[j] & 1) {
            const uint32_t s = s_pos[j], t = p.tgt[abase + j];
            const int sx = (int)(s >> 16) - r, sy = (int)(s & 0xFFFFu) - r;
            const int tx = (int)(t >> 16) - r, ty = (int)(t & 0xFFFFu) - r;
            const uint16_t* f = field + (abase + j) * HW;
            const uint32_t d0 = f[sx * W + sy];
            if (d0 != 0xFFFFu && d0 != 0u) {
                const int levels = (int)d0 + p.inflation - 1;
                for (int i0 = 0; i0 < A; i0 += 64) {
                    const int i = i0 + lane;
                    bool cand = false;
                    uint32_t cpk = 0u;
                    if (i < A && i != j && (s_flag[i] & 2)) {
                        cpk = s_pos[i];
                        const int cx = (int)(cpk >> 16) - r, cy = (int)(cpk & 0xFFFFu) - r;
                        const int dx = abs(sx - cx), dy = abs(sy - cy);
                        if (dx <= r && dy <= r && cpk != s) {
                            const uint32_t fc = f[cx * W + cy];          // (an agent's cell lies inside the map)
                            cand = fc != 0xFFFFu && fc + (uint32_t)(dx + dy) <= d0;   // the filter
                        }
                    }
                    unsigned long long mask = __ballot(cand);
                    while (mask) {                     // the survivors, `segs` at a time
                        int mine = -1;
                        for (int q = 0; q < segs && mask; ++q) {
                            const int idx = __builtin_ctzll(mask);
                            mask &= mask - 1ull;
                            if (q == seg) mine = idx;
                        }
                        const bool have = valid_lane && mine >= 0;
                        const uint32_t cc = __shfl(cpk, mine < 0 ? 0 : mine);
                        const int cx = (int)(cc >> 16) - r, cy = (int)(cc & 0xFFFFu) - r;
                        unsigned long long fr = fr0;
                        if (have && row == cx) fr &= ~(1ull << cy);      // the blocker: one cleared bit of a private mask
                        unsigned long long v = (have && row == sx) ? ((1ull << sy) & fr) : 0ull;
                        bool done = !have, reached = false;
                        for (int d = 1; d <= levels; ++d) {              // bounded by the level count, whatever a field holds
                            unsigned long long up = __shfl(v, lane - 1);
                            unsigned long long dn = __shfl(v, lane + 1);
                            if (row == 0) up = 0ull;
                            if (row == H - 1 || lane == 63) dn = 0ull;
                            unsigned long long nv = (v | (v << 1) | (v >> 1) | up | dn) & fr;
                            if (done) nv = v;
                            const bool hit = (__ballot(row == tx && ((nv >> ty) & 1ull)) & seg_mask) != 0ull;
                            const bool grew = (__ballot(nv != v) & seg_mask) != 0ull;
                            v = nv;
                            if (!done && hit) reached = true;
                            if (hit || !grew) done = true;
                            if (__ballot(!done) == 0ull) break;
                        }
                        const bool rep = have && row == 0 && !reached;   // one lane per search reports a blocked pair
                        if (rep) atomicAdd(&s_count[i0 + mine], 1);
                        by += __popcll(__ballot(rep));
                    }
                }
            }
        }
        if (lane == 0 && p.blocked_by) p.blocked_by[abase + j] = by;
    }
    __syncthreads();
    if (p.count)
        for (int a = tid; a < A; a += blockDim.x) p.count[abase + a] = s_count[a];
}

// ---------------------------------------------------------------------------------------------------------------
// large layout: one search per workgroup at a time
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(1024) blocking_large_kernel(BlockingParams p, size_t per, int wn, int staged) {
    extern __shared__ uint32_t s_vis[];      // [H][wn] visited set, then (staged) [H][wn] free cells of the current env
    __shared__ uint16_t s_list[1024];        // survivors of the filter in the current chunk of blockers, relative to it
    __shared__ uint32_t s_edge[32];          // the last row of the previous band before it was overwritten
    __shared__ int s_n;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int H = p.H, W = p.W, A = p.A, r = p.r;
    const size_t HW = (size_t)H * W;
    const size_t total = (size_t)p.batch * A;
    const size_t begin = blockIdx.x * per, end = min(begin + per, total);
    uint32_t* s_free = s_vis + H * wn;
    const T* field = static_cast<const T*>(p.field);
    constexpr uint32_t UNDEF = (uint32_t)(T)~T(0);
    long long staged_env = -1;

    for (size_t slot = begin; slot < end; ++slot) {      // (everything below is uniform over the workgroup)
        const size_t env = slot / A;
        const int j = (int)(slot - env * A);
        const size_t abase = env * A;
        int by = 0;
        bool live = p.active[slot] & ACTIVE_BIT;
        uint32_t s = 0u, t = 0u, d0 = 0u;
        const T* f = field + slot * HW;
        if (live) {
            s = p.pos[slot];
            t = p.tgt[slot];
            d0 = f[(size_t)((int)(s >> 16) - r) * W + ((int)(s & 0xFFFFu) - r)];
            live = d0 != UNDEF && d0 != 0u;
        }
        if (live) {
            const int sx = (int)(s >> 16) - r, sy = (int)(s & 0xFFFFu) - r;
            const int tx = (int)(t >> 16) - r, ty = (int)(t & 0xFFFFu) - r;
            const int swc = sy >> 5, twc = ty >> 5;
            // (d0 < H * W <= 2^20 and inflation <= 64: no overflow)
            const int levels = (int)d0 + p.inflation - 1;
            const uint32_t* bm = p.obst + env * p.bmw;
            if (staged && staged_env != (long long)env) {
                __syncthreads();             // the previous env's last reads of s_free are done
                for (int i = tid; i < H * wn; i += nt) s_free[i] = blk_free_word(bm, i / wn, i % wn, r, p.wpr, W);
                staged_env = (long long)env; // (visible after the barriers below, before any search reads it)
            }
            for (int i0 = 0; i0 < A; i0 += nt) {
                __syncthreads();             // the previous chunk's last reads of s_list / s_n are done
                if (tid == 0) s_n = 0;
                __syncthreads();
                const int i = i0 + tid;
                if (i < A && i != j && (p.active[abase + i] & ACTIVE_BIT)) {
                    const uint32_t cpk = p.pos[abase + i];
                    const int cx = (int)(cpk >> 16) - r, cy = (int)(cpk & 0xFFFFu) - r;
                    const int dx = abs(sx - cx), dy = abs(sy - cy);
                    if (dx <= r && dy <= r && cpk != s && (!p.on_target || cpk == p.tgt[abase + i])) {
                        const uint32_t fc = f[(size_t)cx * W + cy];
                        if (fc != UNDEF && fc + (uint32_t)(dx + dy) <= d0)    // the filter
                            s_list[atomicAdd(&s_n, 1)] = (uint16_t)tid;      // (at most nt <= 1024 entries)
                    }
                }
                __syncthreads();
                const int n = s_n;
                for (int k = 0; k < n; ++k) {
                    const int ib = i0 + s_list[k];
                    const uint32_t cpk = p.pos[abase + ib];
                    const int cx = (int)(cpk >> 16) - r, cy = (int)(cpk & 0xFFFFu) - r;
                    const int cwc = cy >> 5;
                    const uint32_t cbit = 1u << (cy & 31);
                    __syncthreads();         // the previous search's last reads of s_vis are done
                    for (int q = tid; q < H * wn; q += nt) s_vis[q] = 0u;
                    __syncthreads();
                    if (tid == 0) s_vis[sx * wn + swc] = 1u << (sy & 31);   // (s != c, and an agent stands on a free cell)
                    int r0 = sx, r1 = sx, c0 = swc, c1 = swc;  // bounding box of the visited set (rows, words)
                    bool reached = false;
                    for (int d = 1; d <= levels; ++d) {        // bounded by the level count, whatever a field holds
                        r0 = max(r0 - 1, 0);
                        r1 = min(r1 + 1, H - 1);
                        c0 = max(c0 - 1, 0);
                        c1 = min(c1 + 1, wn - 1);
                        const int bw = c1 - c0 + 1;
                        // the box in bands of whole rows, at most nt * BLK_WORDS words each; a band reads the row above it
                        // from s_edge, the copy of that row from before the previous band overwrote it
                        const int band = max(1, nt * BLK_WORDS / bw);
                        bool any = false;
                        for (int b0 = r0; b0 <= r1; b0 += band) {
                            const int b1 = min(b0 + band, r1 + 1);
                            const int nb = (b1 - b0) * bw;
                            __syncthreads();     // the previous level's / band's writes (and the seed) are visible
                            uint32_t nw[BLK_WORDS];
                            bool changed = false;
                            const int rbw = __builtin_amdgcn_readfirstlane(bw);
#pragma unroll
                            for (int q = 0; q < BLK_WORDS; ++q) {
                                const int idx = tid + q * nt;
                                nw[q] = 0u;
                                if (idx < nb) {
                                    const int x = b0 + idx / rbw, c = c0 + idx % rbw;
                                    const uint32_t* vr = s_vis + x * wn;
                                    const uint32_t v = vr[c];
                                    uint32_t g = v | (v << 1) | (v >> 1);
                                    if (c > 0) g |= vr[c - 1] >> 31;
                                    if (c + 1 < wn) g |= vr[c + 1] << 31;
                                    if (x > 0) g |= (x == b0 && b0 > r0) ? s_edge[c] : vr[c - wn];
                                    if (x + 1 < H) g |= vr[c + wn];
                                    g &= staged ? s_free[x * wn + c] : blk_free_word(bm, x, c, r, p.wpr, W);
                                    if (x == cx && c == cwc) g &= ~cbit;   // the blocker: one cleared bit of a private mask
                                    nw[q] = g;
                                    changed |= g != v;
                                }
                            }
                            // every read of this band's previous set (and of s_edge) is done; the write-back runs even
                            // without a change, so that s_edge always holds the row above the next band
                            any |= __syncthreads_or(changed ? 1 : 0) != 0;
                            const int wb0 = __builtin_amdgcn_readfirstlane(b0), wc0 = __builtin_amdgcn_readfirstlane(c0);
                            const int wbw = __builtin_amdgcn_readfirstlane(bw);
#pragma unroll
                            for (int q = 0; q < BLK_WORDS; ++q) {
                                const int idx = tid + q * nt;
                                if (idx < nb) {
                                    const int x = wb0 + idx / wbw, c = wc0 + idx % wbw;
                                    uint32_t* w = s_vis + x * wn + c;
                                    if (x == b1 - 1) s_edge[c] = *w;  // the next band's row above, as it was
                                    *w = nw[q];
                                }
                            }
                        }
                        __syncthreads();         // the level's writes are visible
                        reached = (s_vis[tx * wn + twc] >> (ty & 31)) & 1u;
                        if (reached || !any) break;   // the target, or an exhausted search
                    }
                    if (!reached) {
                        ++by;
                        if (tid == 0 && p.count) atomicAdd(&p.count[abase + ib], 1);
                    }
                }
            }
        }
        if (tid == 0 && p.blocked_by) p.blocked_by[slot] = by;
    }
}

bool blk_large_layout(int H, int W) { return H > 64 || W > 64; }
// the search's free bitmap is staged in LDS next to the visited set when both fit (as the field build)
bool blk_large_staged(int H, int W) { return (size_t)H * ((W + 31) / 32) * 8 <= 156 * 1024; }
size_t blk_large_lds(int H, int W) {
    return (size_t)H * ((W + 31) / 32) * sizeof(uint32_t) * (blk_large_staged(H, W) ? 2 : 1);
}
int blk_large_threads(int H, int W) {
    const int words = H * ((W + 31) / 32);
    int nt = (words + BLK_WORDS - 1) / BLK_WORDS;
    nt = (nt + 63) / 64 * 64;
    return nt < 256 ? 256 : (nt > 1024 ? 1024 : nt);  // more words than 1024 * BLK_WORDS: several bands per level
}

template <typename T>
hipError_t blocking_large_launch(const BlockingParams& p, hipStream_t stream) {
    const size_t total = (size_t)p.batch * p.A;
    if (p.count) {
        const hipError_t err = launch_zero_i32(p.count, total, stream);
        if (err != hipSuccess) return err;
    }
    const size_t lds = blk_large_lds(p.H, p.W);
    // an attribute of the kernel function, shared by every handle: raise_lds_limit only ever raises it, and only the
    // first call that needs more touches the runtime
    const hipError_t err = raise_lds_limit(reinterpret_cast<const void*>(&blocking_large_kernel<T>), lds);
    if (err != hipSuccess) return err;
    const size_t per = (total + BLK_MAX_GRID - 1) / BLK_MAX_GRID;
    const unsigned grid = (unsigned)((total + per - 1) / per);
    const int wn = (p.W + 31) / 32;
    hipLaunchKernelGGL(blocking_large_kernel<T>, dim3(grid), dim3(blk_large_threads(p.H, p.W)), lds, stream, p, per, wn,
                       blk_large_staged(p.H, p.W) ? 1 : 0);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_blocking(const BlockingParams& p, hipStream_t stream) {
    const hipError_t err = launch_cost_to_go_refresh(p, stream);
    if (err != hipSuccess) return err;
    if (!blk_large_layout(p.H, p.W)) {
        hipLaunchKernelGGL(blocking_small_kernel, dim3(p.batch), dim3(64 * BLK_SMALL_WAVES), 0, stream, p);
        return hipGetLastError();
    }
    return p.cell_bytes == 4 ? blocking_large_launch<uint32_t>(p, stream) : blocking_large_launch<uint16_t>(p, stream);
}

}  // namespace pgx
