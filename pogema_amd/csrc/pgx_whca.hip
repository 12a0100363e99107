// pgx_whca.hip -- windowed cooperative A* against a reservation table (pgx_whca_plan, docs/SPEC.md S28): prioritized
// planning in space-time over `horizon` = K <= 31 steps, with the cached distance fields as the exact heuristic.
//
// One wave per env, serial over the env's planned agents in the order (-priority, index).  Within K steps an agent can
// only reach the (2K+1)^2 box around its cell -- at most 63 rows of 63 cells -- so a layer R_h of the search is one
// 64-bit row mask per lane: lane l holds row (row of the agent) - K + l, bit b column (column of the agent) - K + b.
// Lane 63 and bit 63 lie outside every box and stay 0, so the shifts and the lane exchanges need no guard.
//   per agent:
//     the served agents whose start lies within Chebyshev distance 2K are listed (only they can touch the box);
//     the lane's free mask: the obstacle bits of its row, cut to the map and the box;
//     per layer h: the listed agents' cells at h - 1 and h are scattered into five row masks in LDS (the vertex
//         reservations and, per action of the agent being served, the cells it cannot enter with that action: the edge
//         reservations), one listed agent per lane; R_h = free & ~vertex & (R_{h-1} | the four shifted R_{h-1} & ~edge);
//         R_h is kept in LDS for the backtrack.  Two barriers per layer (of a single wave).
//     the end: the target's layer under `finish`, else the cell of R_K with the smallest (distance, row-major index) --
//         the rows of R_K are read from the agent's field row-contiguously, one cell per lane, then a wave minimum;
//     the backtrack runs on wave-uniform values (the R_h rows are LDS broadcasts; the edge reservations at the current
//         cell are one pass over the listed agents and a ballot); lane h then stores step h of `actions` and `path_xy`.
// The served agents' cells stay in LDS, [K + 1][A] packed words (step-major: the lanes of a scatter read consecutive
// words).  LDS = 8 * 64 * (K + 1) + 2560 + 4 * A * (K + 1) + 9 * A bytes: 27.1 KB at 64 agents and K = 31, 155.5 KB at
// 1024 agents and K = 31 (one workgroup per CU there).  Nothing but the caller's outputs is written.
//
// The same kernel with REPAIR set is pgx_repair_plan (docs/SPEC.md S29): a prologue, one lane per agent, scans the
// caller's `paths` -- in the map, not an obstacle, one of the five moves from the cell before, the `finish` stop -- and
// enters every kept agent (a planned agent with `replan` 0 whose given path is a walk) into the [K + 1][A] cells with
// its last step, exactly as if it had been served: the listing rule above (start within 2K) holds for a kept agent
// because its path is a walk.  The others are ranked and served as ever.  Every `paths` row of the env is in LDS before
// the first output is stored, so `path_xy` may be the `paths` buffer itself.  No LDS beyond S28's formula: whether an
// agent is kept, to be served or not planned is the sign of its s_last.
#include <algorithm>
#include <type_traits>

#include "pgx_internal.h"

namespace pgx {
namespace {

typedef unsigned long long u64;

constexpr int8_t WHCA_UNSERVED = -1;   // s_last of a planned agent that has not been served yet
constexpr int8_t WHCA_UNPLANNED = -2;  // ... of an agent that is not planned: it never reserves anything

__device__ __forceinline__ int whca_dx(int a) { return (a == 2) - (a == 1); }  // MOVES: noop, up, down, left, right
__device__ __forceinline__ int whca_dy(int a) { return (a == 4) - (a == 3); }
// the action that leads from packed cell `from` to its neighbour (or itself) `to`
__device__ __forceinline__ int whca_action(uint32_t from, uint32_t to) {
    const int dr = (int)(to >> 16) - (int)(from >> 16), dc = (int)(to & 0xFFFFu) - (int)(from & 0xFFFFu);
    return dr < 0 ? 1 : dr > 0 ? 2 : dc < 0 ? 3 : dc > 0 ? 4 : 0;
}

__host__ __device__ inline size_t whca_lds_bytes(int A, int K) {
    const size_t n = (size_t)8 * 64 * (K + 1) + 8 * 5 * 64 + (size_t)4 * A * (K + 1) + (size_t)9 * A;
    return (n + 7) & ~(size_t)7;
}

template <typename F, bool REPAIR>
__global__ void __launch_bounds__(64) whca_kernel(const std::conditional_t<REPAIR, RepairParams, WhcaParams> p) {
    extern __shared__ u64 whca_lds[];
    const int lane = threadIdx.x;
    const int A = p.A, K = p.horizon, H = p.H, W = p.W, r = p.r;
    const int env = blockIdx.x;
    u64* s_R = whca_lds;                                          // [K + 1][64] the layers of the agent being served
    u64* s_M = s_R + (size_t)64 * (K + 1);                        // [5][64] vertex mask, then one edge mask per action 1..4
    uint32_t* s_cell = reinterpret_cast<uint32_t*>(s_M + 5 * 64); // [K + 1][A] unpadded (row << 16) | col
    int32_t* s_prio = reinterpret_cast<int32_t*>(s_cell + (size_t)A * (K + 1));
    uint16_t* s_order = reinterpret_cast<uint16_t*>(s_prio + A);  // the planned agents by (-prio, index)
    uint16_t* s_near = s_order + A;                               // the served agents that can touch the box
    int8_t* s_last = reinterpret_cast<int8_t*>(s_near + A);       // last step a served agent reserves

    const size_t e0 = (size_t)env * A;
    const size_t row = (size_t)p.batch * A;   // agents of one step of `actions` and `path_xy`
    const uint32_t ring = (uint32_t)r * 0x10001u;
    const uint32_t* bm = p.obst + (size_t)env * p.bmw;

    for (int j = lane; j < A; j += 64) {
        s_cell[j] = p.pos[e0 + j] - ring;
        s_prio[j] = p.priority ? p.priority[e0 + j] : 0;
        s_last[j] = (p.active[e0 + j] & ACTIVE_BIT) ? WHCA_UNSERVED : WHCA_UNPLANNED;
    }
    for (int q = lane; q < 5 * 64; q += 64) s_M[q] = 0ull;
    if constexpr (REPAIR) {
        // the given paths, one agent per lane: a kept agent's cells and last step go where a served agent's would; an
        // agent that is not planned holds its cell in every row, so that one loop below stores both
        for (int j = lane; j < A; j += 64) {
            uint32_t cur = s_cell[j];
            const bool planned = s_last[j] == WHCA_UNSERVED;
            bool walk = planned && !(p.replan && p.replan[e0 + j]);
            const uint32_t wt = p.tgt[e0 + j] - ring;
            int last = K;
            for (int h = 1; h <= K; ++h) {
                if (walk && h <= last) {
                    const int32_t* g = p.paths + 2 * ((size_t)(h - 1) * row + e0 + j);
                    const int gr = g[0], gc = g[1];
                    // the range check comes first: any int32 may stand there
                    if ((unsigned)gr < (unsigned)H && (unsigned)gc < (unsigned)W) {
                        const int dr = gr - (int)(cur >> 16), dc = gc - (int)(cur & 0xFFFFu);
                        const uint32_t word = bm[(size_t)(gr + r) * p.wpr + ((gc + r) >> 5)];
                        if (abs(dr) + abs(dc) > 1 || ((word >> ((gc + r) & 31)) & 1u)) walk = false;
                        cur = ((uint32_t)gr << 16) | (uint32_t)gc;
                        if (p.finish && cur == wt) last = h;
                    } else {
                        walk = false;
                    }
                }
                s_cell[(size_t)h * A + j] = cur;
            }
            if (walk) s_last[j] = (int8_t)last;
        }
    }
    __syncthreads();

    // the order of service; an agent that is not planned keeps its cell
    int n = 0;
    for (int i0 = 0; i0 < A; i0 += 64) {
        const int i = i0 + lane;
        const bool pl = i < A && s_last[i] == WHCA_UNSERVED;
        const int pi = pl ? s_prio[i] : 0;
        int rank = 0;
        for (int j = 0; j < A; ++j) {         // every lane reads the same words: LDS broadcasts
            const int pj = s_prio[j];
            rank += (s_last[j] == WHCA_UNSERVED && (pj > pi || (pj == pi && j < i))) ? 1 : 0;
        }
        if (pl) s_order[rank] = (uint16_t)i;
        n += __popcll(__ballot(pl));
        if (i < A && !pl) {
            int32_t arrival = -1;
            if constexpr (REPAIR) {
                if (s_last[i] >= 0) {         // a kept agent: S28's rule on its cells
                    const uint32_t wt = p.tgt[e0 + i] - ring;
                    for (int h = K; h >= 0; --h) arrival = s_cell[(size_t)h * A + i] == wt ? h : arrival;
                }
            }
            if (p.arrival) p.arrival[e0 + i] = arrival;
            if (p.failed) p.failed[e0 + i] = 0;
        }
        if constexpr (REPAIR) {
            if (i < A && p.replanned) p.replanned[e0 + i] = pl ? 1 : 0;
        }
    }
    if constexpr (REPAIR) {
        // the kept agents and the agents that are not planned: their rows of the cells are final
        for (int q = lane; q < K * A; q += 64) {
            const int h = q / A, j = q - h * A;
            if (s_last[j] == WHCA_UNSERVED) continue;
            const uint32_t here = s_cell[(size_t)h * A + j], next = s_cell[(size_t)(h + 1) * A + j];
            const int a = whca_action(here, next);
            const size_t o = (size_t)h * row + e0 + j;
            if (p.action_dtype == 0) static_cast<int8_t*>(p.actions)[o] = (int8_t)a;
            else if (p.action_dtype == 1) static_cast<int32_t*>(p.actions)[o] = a;
            else static_cast<long long*>(p.actions)[o] = a;
            if (p.path_xy) {
                p.path_xy[2 * o] = (int32_t)(next >> 16);
                p.path_xy[2 * o + 1] = (int32_t)(next & 0xFFFFu);
            }
        }
    } else {
        for (int q = lane; q < K * A; q += 64) {
            const int h = q / A, j = q - h * A;
            if (s_last[j] != WHCA_UNPLANNED) continue;
            const size_t o = (size_t)h * row + e0 + j;
            if (p.action_dtype == 0) static_cast<int8_t*>(p.actions)[o] = 0;
            else if (p.action_dtype == 1) static_cast<int32_t*>(p.actions)[o] = 0;
            else static_cast<long long*>(p.actions)[o] = 0;
            if (p.path_xy) {
                p.path_xy[2 * o] = (int32_t)(s_cell[j] >> 16);
                p.path_xy[2 * o + 1] = (int32_t)(s_cell[j] & 0xFFFFu);
            }
        }
    }
    __syncthreads();

    for (int k = 0; k < n; ++k) {
        const int i = __builtin_amdgcn_readfirstlane((int)s_order[k]);
        const uint32_t wp = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cell[i]);
        const uint32_t wt = (uint32_t)__builtin_amdgcn_readfirstlane((int)(p.tgt[e0 + i] - ring));
        const int pr = (int)(wp >> 16), pc = (int)(wp & 0xFFFFu);
        const int tr = (int)(wt >> 16) - pr + K, tc = (int)(wt & 0xFFFFu) - pc + K;   // the target in box coordinates
        const bool tgt_in = (unsigned)tr <= (unsigned)(2 * K) && (unsigned)tc <= (unsigned)(2 * K);

        // the served agents that can touch the box
        int nn = 0;
        for (int j0 = 0; j0 < A; j0 += 64) {
            const int j = j0 + lane;
            bool near = false;
            if (j < A && s_last[j] >= 0) {
                const uint32_t w = s_cell[j];
                const int dr = abs((int)(w >> 16) - pr), dc = abs((int)(w & 0xFFFFu) - pc);
                near = max(dr, dc) <= 2 * K;
            }
            const u64 m = __ballot(near);
            if (near) s_near[nn + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)j;
            nn += __popcll(m);
        }

        // the lane's row of the box: in the map, not an obstacle
        u64 free_row = 0ull;
        const int row_l = pr - K + lane;
        if (lane <= 2 * K && row_l >= 0 && row_l < H) {
            const int lo = max(0, K - pc), hi = min(2 * K, W - 1 - pc + K);   // the box's columns inside the map: lo <= K <= hi
            const u64 cols = ((1ull << (hi + 1)) - 1ull) & ~((1ull << lo) - 1ull);
            const int s = pc - K + r;                                         // padded column of bit 0 (may be negative)
            const int w0 = s >> 5, sh = s & 31;
            const uint32_t* rp = bm + (size_t)(row_l + r) * p.wpr;
            const uint32_t a0 = (w0 >= 0 && w0 < p.wpr) ? rp[w0] : 0xFFFFFFFFu;
            const uint32_t a1 = (w0 + 1 >= 0 && w0 + 1 < p.wpr) ? rp[w0 + 1] : 0xFFFFFFFFu;
            const uint32_t a2 = (w0 + 2 >= 0 && w0 + 2 < p.wpr) ? rp[w0 + 2] : 0xFFFFFFFFu;
            u64 obst = (((u64)a1 << 32) | a0) >> sh;
            if (sh) obst |= (u64)a2 << (64 - sh);
            free_row = ~obst & cols;
        }

        u64 prev = lane == K ? 1ull << K : 0ull;                  // R_0: the agent's own cell, the box's centre
        s_R[lane] = prev;
        __syncthreads();                                          // s_near is complete

        int h_end = K;
        bool fail = false, reached = false;
        for (int h = 1; h <= K; ++h) {
            for (int n0 = 0; n0 < nn; n0 += 64) {
                if (n0 + lane >= nn) continue;
                const int j = s_near[n0 + lane];
                if (h > s_last[j]) continue;
                const uint32_t c1 = s_cell[(size_t)h * A + j], c0 = s_cell[(size_t)(h - 1) * A + j];
                const int r1 = (int)(c1 >> 16) - pr + K, q1 = (int)(c1 & 0xFFFFu) - pc + K;
                if ((unsigned)r1 <= (unsigned)(2 * K) && (unsigned)q1 <= (unsigned)(2 * K)) atomicOr(&s_M[r1], 1ull << q1);
                if (c0 == c1) continue;
                // j goes c0 -> c1: the agent being served cannot enter c0 from c1, with the action that leads there
                const int r0 = (int)(c0 >> 16) - pr + K, q0 = (int)(c0 & 0xFFFFu) - pc + K;
                if ((unsigned)r0 <= (unsigned)(2 * K) && (unsigned)q0 <= (unsigned)(2 * K))
                    atomicOr(&s_M[64 * whca_action(c1, c0) + r0], 1ull << q0);
            }
            __syncthreads();
            const u64 v = s_M[lane], e1 = s_M[64 + lane], e2 = s_M[128 + lane], e3 = s_M[192 + lane], e4 = s_M[256 + lane];
            s_M[lane] = 0ull;
            s_M[64 + lane] = 0ull;
            s_M[128 + lane] = 0ull;
            s_M[192 + lane] = 0ull;
            s_M[256 + lane] = 0ull;
            const u64 below = __shfl_down(prev, 1);               // R_{h-1} of row + 1: entered with `up`; lane 63 holds 0
            u64 above = __shfl_up(prev, 1);                       // ... of row - 1: entered with `down`
            if (lane == 0) above = 0ull;
            const u64 cur = free_row & ~v & (prev | (below & ~e1) | (above & ~e2) | ((prev >> 1) & ~e3) | ((prev << 1) & ~e4));
            s_R[(size_t)64 * h + lane] = cur;
            prev = cur;
            __syncthreads();                                      // the masks are clear and R_h is stored
            if (__ballot(cur != 0ull) == 0ull) {
                fail = true;
                break;
            }
            if (p.finish && tgt_in && __ballot(lane == tr && ((cur >> tc) & 1ull)) != 0ull) {
                h_end = h;
                reached = true;
                break;
            }
        }

        int er = K, ec = K;                                       // the end cell in box coordinates
        if (reached) {
            er = tr;
            ec = tc;
        } else if (!fail) {
            const F* f = static_cast<const F*>(p.field) + (e0 + i) * ((size_t)H * W);
            const bool manhattan = f[(size_t)pr * W + pc] == (F)~F(0);   // no path to the target: S28's other key
            u64 best = ~0ull;
            const u64* last_layer = s_R + (size_t)64 * K;
            // no branch around the load -- a lane whose cell is not in R_K reads the agent's own cell instead -- so that
            // the loads of several rows are in flight at once
            const uint32_t own = (uint32_t)(pr * W + pc);
            if (!manhattan) {
#pragma unroll 8
                for (int y = 0; y <= 2 * K; ++y) {
                    const bool in = (last_layer[y] >> lane) & 1ull;
                    const uint32_t idx = (uint32_t)((pr - K + y) * W + (pc - K + lane));
                    const uint32_t d = (uint32_t)f[in ? idx : own];
                    const u64 key = in ? ((u64)d << 32) | idx : ~0ull;
                    best = key < best ? key : best;
                }
            } else {
                for (int y = 0; y <= 2 * K; ++y) {
                    const bool in = (last_layer[y] >> lane) & 1ull;
                    const uint32_t idx = (uint32_t)((pr - K + y) * W + (pc - K + lane));
                    const u64 key = in ? ((u64)(uint32_t)(abs(y - K) + abs(lane - K)) << 32) | idx : ~0ull;
                    best = key < best ? key : best;
                }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const u64 other = __shfl_xor(best, o);
                best = other < best ? other : best;
            }
            const int idx = (int)(uint32_t)best;
            er = idx / W - pr + K;
            ec = idx % W - pc + K;
        }

        if (!fail) {
            const uint32_t wend = ((uint32_t)(pr - K + er) << 16) | (uint32_t)(pc - K + ec);
            if (lane >= h_end && lane <= K) s_cell[(size_t)lane * A + i] = wend;
            int cr = er, cc = ec;
            for (int h = h_end; h >= 1; --h) {
                const uint32_t wcur = ((uint32_t)(pr - K + cr) << 16) | (uint32_t)(pc - K + cc);
                // the edge reservations at the current cell: a served agent that leaves it in step h bars the way back
                uint32_t mine = 0u;
                for (int n0 = 0; n0 < nn; n0 += 64) {
                    if (n0 + lane >= nn) continue;
                    const int j = s_near[n0 + lane];
                    if (h > s_last[j] || s_cell[(size_t)(h - 1) * A + j] != wcur) continue;
                    const uint32_t u = s_cell[(size_t)h * A + j];
                    if (u != wcur) mine |= 1u << whca_action(u, wcur);
                }
                uint32_t barred = 0u;
#pragma unroll
                for (int a = 1; a < 5; ++a) barred |= __ballot((mine >> a) & 1u) != 0ull ? 1u << a : 0u;
                const u64* layer = s_R + (size_t)64 * (h - 1);
                int a = 0;
                for (; a < 5; ++a) {
                    const int ur = cr - whca_dx(a), uc = cc - whca_dy(a);
                    if ((unsigned)ur > (unsigned)(2 * K) || (unsigned)uc > (unsigned)(2 * K)) continue;
                    if (!((layer[ur] >> uc) & 1ull) || ((barred >> a) & 1u)) continue;
                    break;
                }
                cr -= whca_dx(a);                                 // (one always exists: S28)
                cc -= whca_dy(a);
                if (lane == 0) s_cell[(size_t)(h - 1) * A + i] = ((uint32_t)(pr - K + cr) << 16) | (uint32_t)(pc - K + cc);
            }
        } else if (lane <= K) {
            s_cell[(size_t)lane * A + i] = wp;                    // failed: the agent holds its cell for the whole window
        }
        __syncthreads();

        // lane h stores step h
        const uint32_t here = lane <= K ? s_cell[(size_t)lane * A + i] : ~0u;
        if (lane < K) {
            const uint32_t next = s_cell[(size_t)(lane + 1) * A + i];
            const int a = whca_action(here, next);
            const size_t o = (size_t)lane * row + e0 + i;
            if (p.action_dtype == 0) static_cast<int8_t*>(p.actions)[o] = (int8_t)a;
            else if (p.action_dtype == 1) static_cast<int32_t*>(p.actions)[o] = a;
            else static_cast<long long*>(p.actions)[o] = a;
            if (p.path_xy) {
                p.path_xy[2 * o] = (int32_t)(next >> 16);
                p.path_xy[2 * o + 1] = (int32_t)(next & 0xFFFFu);
            }
        }
        const u64 on = __ballot(lane <= K && here == wt);
        if (lane == 0) {
            if (p.arrival) p.arrival[e0 + i] = on ? (int32_t)__builtin_ctzll(on) : -1;
            if (p.failed) p.failed[e0 + i] = fail ? 1 : 0;
            s_last[i] = (int8_t)(fail ? K : h_end);
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_whca(const WhcaParams& p, hipStream_t stream) {
    const size_t lds = whca_lds_bytes(p.A, p.horizon);
    const void* fn = p.cell_bytes == 4 ? reinterpret_cast<const void*>(&whca_kernel<uint32_t, false>)
                                       : reinterpret_cast<const void*>(&whca_kernel<uint16_t, false>);
    // an attribute of the kernel function, shared by every handle: raise_lds_limit only ever raises it, and only the
    // first call that needs more touches the runtime
    if (const hipError_t err = raise_lds_limit(fn, lds)) return err;
    if (p.cell_bytes == 4)
        hipLaunchKernelGGL((whca_kernel<uint32_t, false>), dim3((unsigned)p.batch), dim3(64), lds, stream, p);
    else
        hipLaunchKernelGGL((whca_kernel<uint16_t, false>), dim3((unsigned)p.batch), dim3(64), lds, stream, p);
    return hipGetLastError();
}

// LDS of the repair: S28's formula, nothing more (the kept agents' cells and last steps lie where a served agent's do)
size_t repair_lds_bytes(int A, int K) { return whca_lds_bytes(A, K); }

hipError_t launch_repair(const RepairParams& p, hipStream_t stream) {
    const size_t lds = repair_lds_bytes(p.A, p.horizon);
    const void* fn = p.cell_bytes == 4 ? reinterpret_cast<const void*>(&whca_kernel<uint32_t, true>)
                                       : reinterpret_cast<const void*>(&whca_kernel<uint16_t, true>);
    if (const hipError_t err = raise_lds_limit(fn, lds)) return err;
    if (p.cell_bytes == 4)
        hipLaunchKernelGGL((whca_kernel<uint32_t, true>), dim3((unsigned)p.batch), dim3(64), lds, stream, p);
    else
        hipLaunchKernelGGL((whca_kernel<uint16_t, true>), dim3((unsigned)p.batch), dim3(64), lds, stream, p);
    return hipGetLastError();
}

}  // namespace pgx
