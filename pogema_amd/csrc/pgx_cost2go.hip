// pgx_cost2go.hip -- cost-to-go observation windows (pgx_cost_to_go, docs/SPEC.md S11).
//
// For every active agent: the 4-connected BFS distance to its current target of every cell of its (2r+1)^2 window.
// A distance field depends only on (map, target), so the handle caches one full H x W field per agent and rebuilds only
// the stale ones.  One call is three launches, so that no workgroup ever waits on another workgroup's stores:
//   1. invalidate: one workgroup per env compares the env's free bits (the engine's padded bitmap, padding masked out)
//      with the copy its fields were built on; on a difference it takes the new bits and clears every target tag of the
//      env.
//   2. build: a field is stale when its agent is active and its tag differs from the agent's target.  A stale field is
//      rebuilt by a bit-parallel BFS from the target, run to exhaustion (pgx_expert.hip's search without the early exit);
//      every cell is written once: its level when it is first visited, "unreachable" (all ones) for the cells never
//      visited.  pgx_expert.hip's two layouts:
//        small (H <= 64 and W <= 64): one workgroup per environment, one lane per map row, floor(64 / H) searches per
//              wave; the field is assembled in LDS and written out coalesced.
//        large (any other legal map): workgroups own contiguous ranges of (env, agent) slots, scan them for stale ones and
//              run one search at a time; the visited set lives in LDS, its bounding box grows one row / word per level.
//      Fresh slots cost one tag compare, so the launch shape never depends on device data and the call is capturable.
//   3. gather: the windows as a flat stream of 16-byte stores, -1 outside the map, on obstacles, for unreachable cells
//      and for inactive agents.
// The engine state the next pgx_step reads is only read; the cache is the only thing written besides `out`.
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr uint32_t C2G_NO_FIELD = 0xFFFFFFFFu;  // tag of a slot without a valid field (never a packed padded cell)
// large layout: visited-set words one thread stages in VGPRs per band of rows (larger maps take several bands per level)
constexpr int C2G_WORDS = 8;
constexpr size_t C2G_MAX_GRID = 4096;           // large-layout build: workgroups; each owns a contiguous range of slots
constexpr size_t C2G_GATHER_MAX_GRID = size_t(1) << 20;

// 32 free bits of unpadded row x, unpadded columns [32 c, 32 c + 32), bits at or beyond W cleared (the padding is never
// traversed).  The same function as pgx_expert.hip's, which keeps its own copy so that its code stays untouched.
__device__ __forceinline__ uint32_t c2g_free_word(const uint32_t* __restrict__ bm, int x, int c, int r, int wpr, int W) {
    const uint32_t* row = bm + (size_t)(x + r) * wpr;
    const int col = 32 * c + r;
    const int w0 = col >> 5, sh = col & 31;
    uint32_t obst = row[w0] >> sh;
    if (sh && (w0 + 1) * 32 < W + r) obst |= row[w0 + 1] << (32 - sh);
    const int n = W - 32 * c;
    const uint32_t mask = n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u);
    return ~obst & mask;
}

__device__ __forceinline__ bool c2g_target_free(const uint32_t* __restrict__ bm, int px, int py, int wpr) {
    return !((bm[(size_t)px * wpr + (py >> 5)] >> (py & 31)) & 1u);
}

__device__ __forceinline__ bool c2g_stale(const CostToGoParams& p, size_t slot) {
    return (p.active[slot] & ACTIVE_BIT) && p.tag[slot] != p.tgt[slot];
}

// ---------------------------------------------------------------------------------------------------------------
// 1. invalidate
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) c2g_invalidate_kernel(CostToGoParams p, int wn) {
    const int env = blockIdx.x, tid = threadIdx.x;
    const uint32_t* bm = p.obst + (size_t)env * p.bmw;
    uint32_t* mb = p.map_bits + (size_t)env * p.H * wn;
    bool diff = false;
    for (int i = tid; i < p.H * wn; i += blockDim.x) {  // every word is read and written by one thread only
        const int x = i / wn, c = i - x * wn;
        const uint32_t f = c2g_free_word(bm, x, c, p.r, p.wpr, p.W);
        if (mb[i] != f) {
            mb[i] = f;
            diff = true;
        }
    }
    if (__syncthreads_or(diff ? 1 : 0))
        for (int a = tid; a < p.A; a += blockDim.x) p.tag[(size_t)env * p.A + a] = C2G_NO_FIELD;
}

// ---------------------------------------------------------------------------------------------------------------
// 2a. build, small layout: H <= 64, W <= 64, u16 fields
// ---------------------------------------------------------------------------------------------------------------
constexpr int C2G_SMALL_WAVES = 4;

__global__ void __launch_bounds__(64 * C2G_SMALL_WAVES) c2g_build_small_kernel(CostToGoParams p) {
    __shared__ unsigned long long s_free[64];
    __shared__ uint16_t s_list[1024];                                        // stale agents of this env
    __shared__ __attribute__((aligned(16))) uint16_t s_field[C2G_SMALL_WAVES][64 * 64];  // one wave's fields
    __shared__ int s_n;
    const int env = blockIdx.x, tid = threadIdx.x;
    const int H = p.H, W = p.W, HW = H * W;
    const uint32_t* bm = p.obst + (size_t)env * p.bmw;
    const size_t abase = (size_t)env * p.A;
    if (tid < 64) {
        unsigned long long f = 0ull;
        if (tid < H) {
            f = c2g_free_word(bm, tid, 0, p.r, p.wpr, W);
            if (W > 32) f |= (unsigned long long)c2g_free_word(bm, tid, 1, p.r, p.wpr, W) << 32;
        }
        s_free[tid] = f;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int a = tid; a < p.A; a += blockDim.x)
        if (c2g_stale(p, abase + a)) s_list[atomicAdd(&s_n, 1)] = (uint16_t)a;
    __syncthreads();
    const int n = s_n;
    if (n == 0) return;
    if (tid == 0) atomicAdd(p.builds, (unsigned long long)n);

    const int lane = tid & 63, wave = tid >> 6;
    const int segs = 64 / H;                 // searches per wave
    const int seg = lane / H, row = lane - seg * H;
    const bool valid_lane = seg < segs;
    const unsigned long long seg_mask =
        H == 64 ? ~0ull : (valid_lane ? (((1ull << H) - 1ull) << (seg * H)) : 0ull);
    const unsigned long long fr = valid_lane ? s_free[row] : 0ull;
    uint16_t* wf = s_field[wave];            // the wave's segs fields, H * W cells each
    uint16_t* sf = wf + (valid_lane ? seg : 0) * HW;
    uint16_t* field = static_cast<uint16_t*>(p.field);

    // rounds are uniform over the workgroup, so that the barriers below are reached by every wave
    for (int base = 0; base < n; base += C2G_SMALL_WAVES * segs) {
        const int first = base + wave * segs;
        __syncthreads();                     // the previous round's write-out has read the LDS fields
        uint32_t* wf32 = reinterpret_cast<uint32_t*>(wf);
        for (int j = lane; j < (segs * HW + 1) / 2; j += 64) wf32[j] = 0xFFFFFFFFu;
        __syncthreads();
        const int k = first + seg;
        const bool have = valid_lane && k < n;
        int tx = -1, ty = 0;
        if (have) {
            const uint32_t t = p.tgt[abase + s_list[k]];
            tx = (int)(t >> 16) - p.r;
            ty = (int)(t & 0xFFFFu) - p.r;
        }
        unsigned long long v = (have && row == tx) ? ((1ull << ty) & fr) : 0ull;
        if (v) sf[row * W + ty] = 0;
        bool done = !have;
        for (int d = 1; __ballot(!done) != 0ull; ++d) {
            unsigned long long up = __shfl(v, lane - 1);
            unsigned long long dn = __shfl(v, lane + 1);
            if (row == 0) up = 0ull;
            if (row == H - 1 || lane == 63) dn = 0ull;
            unsigned long long nv = (v | (v << 1) | (v >> 1) | up | dn) & fr;
            if (done) nv = v;
            for (unsigned long long nb = nv & ~v; nb; nb &= nb - 1ull) sf[row * W + __builtin_ctzll(nb)] = (uint16_t)d;
            if ((__ballot(nv != v) & seg_mask) == 0ull) done = true;
            v = nv;
        }
        __syncthreads();
        // write-out: each of the wave's searches to its slot, 16-byte stores when the fields are 16-byte aligned
        const int mine = min(segs, n - first);
        for (int s = 0; s < mine; ++s) {
            const size_t slot = abase + s_list[first + s];
            uint16_t* g = field + slot * HW;
            const uint16_t* l = wf + s * HW;
            if ((HW & 7) == 0) {
                for (int j = lane; j < HW / 8; j += 64)
                    reinterpret_cast<uint4*>(g)[j] = reinterpret_cast<const uint4*>(l)[j];
            } else {
                for (int j = lane; j < HW; j += 64) g[j] = l[j];
            }
            if (lane == 0) p.tag[slot] = p.tgt[slot];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 2b. build, large layout: one search per workgroup at a time
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(1024) c2g_build_large_kernel(CostToGoParams p, size_t per, int wn, int staged) {
    extern __shared__ uint32_t s_vis[];      // [H][wn] visited set, then (staged) [H][wn] free cells
    __shared__ uint16_t s_list[1024];        // stale slots of the current chunk, relative to it
    __shared__ uint32_t s_edge[32];          // the last row of the previous band before it was overwritten
    __shared__ int s_n;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int H = p.H, W = p.W;
    const size_t HW = (size_t)H * W;
    const size_t total = (size_t)p.batch * p.A;
    const size_t begin = blockIdx.x * per, end = min(begin + per, total);
    uint32_t* s_free = s_vis + H * wn;
    T* field = static_cast<T*>(p.field);
    unsigned long long built = 0;
    for (size_t chunk = begin; chunk < end; chunk += nt) {
        __syncthreads();                     // the previous chunk's last reads of s_list / s_vis are done
        if (tid == 0) s_n = 0;
        __syncthreads();
        if (chunk + tid < end && c2g_stale(p, chunk + tid)) s_list[atomicAdd(&s_n, 1)] = (uint16_t)tid;
        __syncthreads();
        const int n = s_n;
        built += n;
        for (int k = 0; k < n; ++k) {
            const size_t slot = chunk + s_list[k];
            const uint32_t* bm = p.obst + (slot / p.A) * p.bmw;
            const uint32_t t = p.tgt[slot];
            const int tx = (int)(t >> 16) - p.r, ty = (int)(t & 0xFFFFu) - p.r;
            const int twc = ty >> 5;
            T* f = field + slot * HW;
            __syncthreads();                 // the previous search's last reads of s_vis are done
            for (int i = tid; i < H * wn; i += nt) {
                s_vis[i] = 0u;
                if (staged) s_free[i] = c2g_free_word(bm, i / wn, i % wn, p.r, p.wpr, W);
            }
            __syncthreads();
            if (tid == 0 && c2g_target_free(bm, tx + p.r, ty + p.r, p.wpr)) {
                s_vis[tx * wn + twc] = 1u << (ty & 31);
                f[(size_t)tx * W + ty] = 0;
            }
            int r0 = tx, r1 = tx, c0 = twc, c1 = twc;  // bounding box of the visited set (rows, words)
            for (int d = 1;; ++d) {
                r0 = max(r0 - 1, 0);
                r1 = min(r1 + 1, H - 1);
                c0 = max(c0 - 1, 0);
                c1 = min(c1 + 1, wn - 1);
                const int bw = c1 - c0 + 1;
                // the box in bands of whole rows, at most nt * C2G_WORDS words each; a band reads the row above it from
                // s_edge, the copy of that row from before the previous band overwrote it
                const int band = max(1, nt * C2G_WORDS / bw);
                bool any = false;
                for (int b0 = r0; b0 <= r1; b0 += band) {
                    const int b1 = min(b0 + band, r1 + 1);
                    const int nb = (b1 - b0) * bw;
                    __syncthreads();         // the previous level's / band's writes (and the seed) are visible
                    uint32_t nw[C2G_WORDS];
                    bool changed = false;
                    const int rbw = __builtin_amdgcn_readfirstlane(bw);  // per band: no division hoisted out of the loop
#pragma unroll
                    for (int q = 0; q < C2G_WORDS; ++q) {
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
                            g &= staged ? s_free[x * wn + c] : c2g_free_word(bm, x, c, p.r, p.wpr, W);
                            nw[q] = g;
                            changed |= g != v;
                        }
                    }
                    // every read of this band's previous set (and of s_edge) is done; the write-back runs even without a
                    // change, so that s_edge always holds the row above the next band
                    any |= __syncthreads_or(changed ? 1 : 0) != 0;
                    // the band again as fresh values: the compiler would otherwise keep every word's (x, c) of the first
                    // pass live across the barrier, and spill
                    const int wb0 = __builtin_amdgcn_readfirstlane(b0), wc0 = __builtin_amdgcn_readfirstlane(c0);
                    const int wbw = __builtin_amdgcn_readfirstlane(bw);
#pragma unroll
                    for (int q = 0; q < C2G_WORDS; ++q) {
                        const int idx = tid + q * nt;
                        if (idx < nb) {
                            const int x = wb0 + idx / wbw, c = wc0 + idx % wbw;
                            uint32_t* w = s_vis + x * wn + c;
                            if (x == b1 - 1) s_edge[c] = *w;  // the next band's row above, as it was
                            // cells first visited at this level: their distance is d (only this thread owns word w)
                            for (uint32_t m = nw[q] & ~*w; m; m &= m - 1u) f[(size_t)x * W + 32 * c + __builtin_ctz(m)] = (T)d;
                            *w = nw[q];
                        }
                    }
                }
                if (!any) break;             // nothing new anywhere: the search is exhausted
            }
            // every cell never visited (obstacle, unreachable, or all of them behind a blocked target): all ones
            for (size_t j = tid; j < HW; j += nt) {
                const int x = (int)(j / W), y = (int)(j - (size_t)x * W);
                if (!((s_vis[x * wn + (y >> 5)] >> (y & 31)) & 1u)) f[j] = (T)~T(0);
            }
            if (tid == 0) p.tag[slot] = t;
        }
    }
    if (tid == 0 && built) atomicAdd(p.builds, built);
}

// ---------------------------------------------------------------------------------------------------------------
// 3. gather
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) c2g_gather_kernel(CostToGoParams p, size_t n, int vec) {
    const int ws = 2 * p.r + 1, ww = ws * ws, off = 2 * p.r;  // padded position - 2r = window corner (unpadded)
    const size_t HW = (size_t)p.H * p.W;
    const T* field = static_cast<const T*>(p.field);
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    for (size_t q = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; q < n; q += stride) {
        size_t slot = q / ww;
        int rem = (int)(q - slot * ww);
        int u = rem / ws, v = rem - u * ws;
        int vals[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int val = -1;
            if (q + e < n) {
                const uint32_t pp = p.pos[slot];
                const int cx = (int)(pp >> 16) - off + u, cy = (int)(pp & 0xFFFFu) - off + v;
                if ((p.active[slot] & ACTIVE_BIT) && cx >= 0 && cx < p.H && cy >= 0 && cy < p.W) {
                    const T d = field[slot * HW + (size_t)cx * p.W + cy];
                    if (d != (T)~T(0)) val = (int)d;
                }
            }
            vals[e] = val;
            if (++v == ws) {
                v = 0;
                if (++u == ws) {
                    u = 0;
                    ++slot;
                }
            }
        }
        if (vec && q + 4 <= n) {
            *reinterpret_cast<int4*>(p.out + q) = make_int4(vals[0], vals[1], vals[2], vals[3]);
        } else {
            for (int e = 0; e < 4 && q + e < n; ++e) p.out[q + e] = vals[e];
        }
    }
}

bool c2g_large_layout(int H, int W) { return H > 64 || W > 64; }
bool c2g_wide_cells(int H, int W) { return (size_t)H * W > 65536; }
// the search's free bitmap is staged in LDS next to the visited set when both fit (as pgx_expert.hip)
bool c2g_large_staged(int H, int W) { return (size_t)H * ((W + 31) / 32) * 8 <= 156 * 1024; }
size_t c2g_large_lds(int H, int W) {
    return (size_t)H * ((W + 31) / 32) * sizeof(uint32_t) * (c2g_large_staged(H, W) ? 2 : 1);
}
int c2g_large_threads(int H, int W) {
    const int words = H * ((W + 31) / 32);
    int nt = (words + C2G_WORDS - 1) / C2G_WORDS;
    nt = (nt + 63) / 64 * 64;
    return nt < 256 ? 256 : (nt > 1024 ? 1024 : nt);  // more words than 1024 * C2G_WORDS: several bands per level
}

template <typename T>
const void* c2g_large_fn() { return reinterpret_cast<const void*>(&c2g_build_large_kernel<T>); }

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace

CostToGoLayout cost_to_go_layout(int batch, int A, int H, int W) {
    CostToGoLayout l;
    const size_t slots = (size_t)batch * A;
    l.cell_bytes = c2g_wide_cells(H, W) ? 4 : 2;
    l.builds_off = 0;
    l.field_off = 16;
    l.tag_off = l.field_off + round16(slots * H * W * l.cell_bytes);
    l.map_off = l.tag_off + slots * sizeof(uint32_t);
    l.bytes = l.map_off + (size_t)batch * H * ((W + 31) / 32) * sizeof(uint32_t);
    return l;
}

hipError_t prepare_cost_to_go(int H, int W) {
    if (!c2g_large_layout(H, W)) return hipSuccess;
    // an attribute of the kernel function, shared by every handle: raise_lds_limit only ever raises it
    const void* fn = c2g_wide_cells(H, W) ? c2g_large_fn<uint32_t>() : c2g_large_fn<uint16_t>();
    return raise_lds_limit(fn, c2g_large_lds(H, W));
}

hipError_t launch_cost_to_go_refresh(const CostToGoParams& p, hipStream_t stream) {
    const int wn = (p.W + 31) / 32;
    hipLaunchKernelGGL(c2g_invalidate_kernel, dim3(p.batch), dim3(256), 0, stream, p, wn);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const bool wide = c2g_wide_cells(p.H, p.W);
    const size_t total = (size_t)p.batch * p.A;
    if (!c2g_large_layout(p.H, p.W)) {
        hipLaunchKernelGGL(c2g_build_small_kernel, dim3(p.batch), dim3(64 * C2G_SMALL_WAVES), 0, stream, p);
    } else {
        const size_t per = (total + C2G_MAX_GRID - 1) / C2G_MAX_GRID;
        const unsigned grid = (unsigned)((total + per - 1) / per);
        const int nt = c2g_large_threads(p.H, p.W);
        const size_t lds = c2g_large_lds(p.H, p.W);
        const int staged = c2g_large_staged(p.H, p.W) ? 1 : 0;
        if (wide) hipLaunchKernelGGL(c2g_build_large_kernel<uint32_t>, dim3(grid), dim3(nt), lds, stream, p, per, wn, staged);
        else hipLaunchKernelGGL(c2g_build_large_kernel<uint16_t>, dim3(grid), dim3(nt), lds, stream, p, per, wn, staged);
    }
    return hipGetLastError();
}

hipError_t launch_cost_to_go(const CostToGoParams& p, hipStream_t stream) {
    const hipError_t err = launch_cost_to_go_refresh(p, stream);
    if (err != hipSuccess) return err;
    const bool wide = c2g_wide_cells(p.H, p.W);
    const size_t total = (size_t)p.batch * p.A;
    const int ws = 2 * p.r + 1;
    const size_t n = total * ws * ws;
    const size_t quads = (n + 3) / 4;
    const unsigned grid = (unsigned)std::min((quads + 255) / 256, C2G_GATHER_MAX_GRID);
    const int vec = (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 ? 1 : 0;
    if (wide) hipLaunchKernelGGL(c2g_gather_kernel<uint32_t>, dim3(grid), dim3(256), 0, stream, p, n, vec);
    else hipLaunchKernelGGL(c2g_gather_kernel<uint16_t>, dim3(grid), dim3(256), 0, stream, p, n, vec);
    return hipGetLastError();
}

}  // namespace pgx
