// pgx_pibt.hip -- cooperative one-step planner (pgx_pibt_actions, docs/SPEC.md S13): PIBT, priority inheritance with
// backtracking, on the distance fields pgx_cost2go.hip caches.
//
// One launch after the cache refresh (launch_cost_to_go_refresh).  One lane per agent; a workgroup holds
// min(64, floor(T / A)) whole envs (T = 256 lanes while A <= 256, 1024 above), so that the serial phase of all its envs
// runs side by side in the lanes of ONE wave.
//   phase 1 (parallel, every lane): the agent's five candidate cells -- in-map and obstacle tests against the padded
//       bitmap, their distances D_i from the agent's field (the only global-memory latency of the kernel: five
//       independent loads per lane, issued before anything depends on them), and one sweep over the env's staged
//       positions that finds `now` of the five cells (the lowest planned agent standing there) and the agent's rank in
//       the order (-prio, index).  A candidate's place in the agent's list depends only on the state, never on the
//       recursion, so the list is sorted here (a 9-comparator network over 64-bit keys in registers) and stored packed:
//       16 bits per candidate = action | occupied << 3 | occupant << 4, all ones = end of list.
//   phase 2 (serial per env, lane e of wave 0 = env e of the workgroup): the recursion as a loop.  An agent is on the
//       call stack at most once, so the stack is two per-agent fields: its caller and its position in its candidate
//       list.  `res` is only ever asked "is this cell reserved?", and the reserved cells are exactly the current `next`
//       cells (a reservation whose branch failed is the failed agent's own cell), so it is a set: open addressing,
//       linear probing, 2^ceil(log2(2A)) words per env keyed by the packed cell, never more than half full, nothing is
//       ever deleted.  The same table serves every legal map size (a dense H x W table would be 2 MB at 1024 x 1024).
//       Phase 2 touches LDS only.  It, the reservation set and the packed formats live in pgx_pibt_plan.h, shared
//       with the collision shield (pgx_shield.hip), whose lanes order their candidates by the caller's scores.
//   stores (parallel, every lane): action and next cell; unplanned agents get action 0 and their own cell.
// LDS: 40 bytes per lane + 256 (10.25 KB / 40.25 KB), static.  The grid depends on batch and A only; nothing but the caller's
// outputs is written.
#include "pgx_pibt_plan.h"

namespace pgx {
namespace {

template <int T, typename F>
__global__ void __launch_bounds__(T) pibt_kernel(const PibtParams p, int epb, int log2n) {
    __shared__ uint32_t s_pos[T];             // packed padded cell of a planned agent, PIBT_FAR otherwise
    __shared__ int32_t s_prio[T];
    __shared__ uint32_t s_set[4 * T];         // the envs' reservation sets
    __shared__ uint16_t s_cand[5 * T];        // sorted candidate lists
    __shared__ uint16_t s_order[T];           // the env's planned agents by (-prio, index)
    __shared__ uint16_t s_par[T];             // phase 2: the agent's caller
    __shared__ uint8_t s_ci[T];               // phase 2: candidates of the agent already tried
    __shared__ uint8_t s_act[T];              // the agent's action; PIBT_UNSET: `next` unset
    __shared__ uint32_t s_n[64];              // planned agents per env

    const int t = threadIdx.x;
    const int A = p.A, r = p.r;
    const int env0 = blockIdx.x * epb;
    const int nenv = min(epb, p.batch - env0);
    const int el = t / A, i = t - el * A, base = el * A;
    const bool have = el < nenv;
    const size_t slot = (size_t)(env0 + el) * A + i;

    uint32_t w = PIBT_FAR;
    bool planned = false;
    int prio = 0;
    if (have) {
        w = p.pos[slot];
        planned = (p.active[slot] & ACTIVE_BIT) != 0;
        if (p.priority) prio = p.priority[slot];
    }
    s_pos[t] = planned ? w : PIBT_FAR;
    s_prio[t] = prio;
    s_act[t] = planned ? PIBT_UNSET : (uint8_t)0;
    if (t < 64) s_n[t] = 0u;
    for (int q = t; q < (epb << log2n); q += T) s_set[q] = PIBT_EMPTY;

    // the five candidate cells and their distances: loads first, the sweep below hides them
    const int px = (int)(w >> 16), py = (int)(w & 0xFFFFu);
    uint32_t cell[5], dist[5];
    if (planned) {
        const uint32_t* bm = p.obst + (size_t)(env0 + el) * p.bmw;
        const F* f = static_cast<const F*>(p.field) + slot * ((size_t)p.H * p.W);
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            const int vx = px + pibt_dx(a), vy = py + pibt_dy(a);
            const int ux = vx - r, uy = vy - r;
            bool ok = ux >= 0 && ux < p.H && uy >= 0 && uy < p.W;
            if (ok) ok = !((bm[(size_t)vx * p.wpr + (vy >> 5)] >> (vy & 31)) & 1u);
            cell[a] = ok ? (((uint32_t)vx << 16) | (uint32_t)vy) : PIBT_NO_CELL;
            F d = (F)~F(0);
            if (ok) d = f[(size_t)ux * p.W + uy];
            dist[a] = d == (F)~F(0) ? PIBT_INF : (uint32_t)d;
        }
    } else {
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            cell[a] = PIBT_NO_CELL;
            dist[a] = PIBT_INF;
        }
    }
    __syncthreads();

    if (planned) {
        uint32_t occ[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) occ[a] = 0xFFFFu;
        int rank = 0;
        for (int j = 0; j < A; ++j) {         // lanes of one env read the same word: an LDS broadcast
            const uint32_t wj = s_pos[base + j];
            const int pj = s_prio[base + j];
#pragma unroll
            for (int a = 0; a < 5; ++a)
                if (wj == cell[a] && occ[a] == 0xFFFFu) occ[a] = (uint32_t)j;
            rank += (wj != PIBT_FAR && (pj > prio || (pj == prio && j < i))) ? 1 : 0;
        }
        // key: D, then unoccupied first, then the action; the occupant rides along below them
        unsigned long long key[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            const bool other = occ[a] != 0xFFFFu && occ[a] != (uint32_t)i;
            key[a] = cell[a] == PIBT_NO_CELL
                         ? PIBT_DROP
                         : ((unsigned long long)dist[a] << 16) | ((other ? 1ull : 0ull) << 15) | ((unsigned long long)a << 12) |
                               (other ? occ[a] : 0u);
        }
        pibt_cswap(key[0], key[1]);
        pibt_cswap(key[3], key[4]);
        pibt_cswap(key[2], key[4]);
        pibt_cswap(key[2], key[3]);
        pibt_cswap(key[1], key[4]);
        pibt_cswap(key[0], key[3]);
        pibt_cswap(key[0], key[2]);
        pibt_cswap(key[1], key[3]);
        pibt_cswap(key[1], key[2]);
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const uint32_t k = (uint32_t)key[q];
            s_cand[5 * t + q] = key[q] == PIBT_DROP
                                    ? PIBT_END
                                    : (uint16_t)(((k >> 12) & 7u) | (((k >> 15) & 1u) << 3) | ((k & 0x3FFu) << 4));
        }
        s_order[base + rank] = (uint16_t)i;
        atomicAdd(&s_n[el], 1u);
    }
    __syncthreads();

    pibt_serial(PibtLds{s_pos, s_prio, s_set, s_cand, s_order, s_par, s_ci, s_act, s_n}, nenv, A, log2n);
    __syncthreads();

    if (have) {
        const int a = s_act[t];
        if (p.action_dtype == 0) static_cast<int8_t*>(p.actions)[slot] = (int8_t)a;
        else if (p.action_dtype == 1) static_cast<int32_t*>(p.actions)[slot] = a;
        else static_cast<long long*>(p.actions)[slot] = a;
        if (p.next_xy) {
            p.next_xy[2 * slot] = px - r + pibt_dx(a);
            p.next_xy[2 * slot + 1] = py - r + pibt_dy(a);
        }
    }
}

template <int T>
hipError_t pibt_launch(const PibtParams& p, hipStream_t stream) {
    const int epb = std::min(64, T / p.A);
    int log2n = 1;
    while ((1 << log2n) < 2 * p.A) ++log2n;   // epb << log2n < epb * 4A <= 4T words
    const unsigned grid = (unsigned)((p.batch + epb - 1) / epb);
    if (p.cell_bytes == 4) hipLaunchKernelGGL((pibt_kernel<T, uint32_t>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    else hipLaunchKernelGGL((pibt_kernel<T, uint16_t>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pibt(const PibtParams& p, hipStream_t stream) {
    return p.A <= 256 ? pibt_launch<256>(p, stream) : pibt_launch<1024>(p, stream);
}

}  // namespace pgx
