// pgx_pibt_horizon.hip -- multi-step planner (pgx_pibt_plan, docs/SPEC.md S16): the one-step planner of pgx_pibt.hip
// iterated `horizon` times inside one launch, on a private copy of the positions, with the textbook growing priorities.
//
// The sibling of pibt_kernel: the same lane layout (one lane per agent, min(64, floor(T / A)) whole envs per workgroup,
// T = 256 lanes while A <= 256, 1024 above), the same LDS arrays and packed candidate lists, the same serial phase
// (pgx_pibt_plan.h); its body is wrapped in the loop over the steps h of the lookahead.
//   across the steps a lane keeps in registers: its agent's packed padded cell, planned flag, priority, the packed
//       target word (the targets, and with them the distance fields, are held for the whole lookahead) and the first
//       step at which the agent stood on its target.
//   every step: the lane re-stages its cell, priority and action and the workgroup clears the reservation sets and the
//       per-env counts (all readers of the previous step are behind its last barrier); the five field loads at the new
//       cell are issued, then the barrier, the sweep and the sort of pibt_kernel's phase 1, the barrier, phase 2, the
//       barrier; the lane stores row h of `actions` and `path_xy`, moves, and applies S16's planned / priority rules.
//   after the last step: `arrival` and `priority_out`.
// Three barriers per step; every lane of the workgroup runs all `horizon` steps, planned or not.
// LDS: 40 bytes per lane + 256 (10.25 KB / 40.25 KB), static, as pibt_kernel.  The grid depends on batch and A only;
// nothing but the caller's outputs is written.
#include "pgx_pibt_plan.h"

namespace pgx {
namespace {

template <int T, typename F>
__global__ void __launch_bounds__(T) pibt_horizon_kernel(const PibtPlanParams p, int epb, int log2n) {
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
    const size_t row = (size_t)p.batch * A;   // agents of one step of `actions` and `path_xy`

    uint32_t w = PIBT_FAR, tgt = PIBT_FAR;
    bool planned = false;
    int prio = 0;
    if (have) {
        w = p.pos[slot];
        tgt = p.tgt[slot];
        planned = (p.active[slot] & ACTIVE_BIT) != 0;
        if (p.priority) prio = p.priority[slot];
    }
    const bool planned0 = planned;
    int arrived_at = (planned0 && w == tgt) ? 0 : -1;
    const uint32_t* bm = p.obst + (size_t)(env0 + el) * p.bmw;
    const F* f = static_cast<const F*>(p.field) + slot * ((size_t)p.H * p.W);

    for (int h = 0; h < p.horizon; ++h) {
        s_pos[t] = planned ? w : PIBT_FAR;
        s_prio[t] = prio;
        s_act[t] = planned ? PIBT_UNSET : (uint8_t)0;
        if (t < 64) s_n[t] = 0u;
        for (int q = t; q < (epb << log2n); q += T) s_set[q] = PIBT_EMPTY;

        // the five candidate cells and their distances: loads first, the sweep below hides them
        const int px = (int)(w >> 16), py = (int)(w & 0xFFFFu);
        uint32_t cell[5], dist[5];
        if (planned) {
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
            for (int a = 0; a < 5; ++a) occ[a] = PIBT_NOBODY;
            int rank = 0;
            for (int j = 0; j < A; ++j) {     // lanes of one env read the same word: an LDS broadcast
                const uint32_t wj = s_pos[base + j];
                const int pj = s_prio[base + j];
#pragma unroll
                for (int a = 0; a < 5; ++a)
                    if (wj == cell[a] && occ[a] == PIBT_NOBODY) occ[a] = (uint32_t)j;
                rank += (wj != PIBT_FAR && (pj > prio || (pj == prio && j < i))) ? 1 : 0;
            }
            // key: D, then unoccupied first, then the action; the occupant rides along below them
            unsigned long long key[5];
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                const bool other = occ[a] != PIBT_NOBODY && occ[a] != (uint32_t)i;
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

        // row h of the outputs, then S16's dynamics; the next step's staging overwrites only what this lane owns
        // (s_pos[t], s_prio[t], s_act[t]) or what nobody reads any more (the sets, the counts)
        if (have) {
            const int a = s_act[t];
            const size_t o = (size_t)h * row + slot;
            if (p.action_dtype == 0) static_cast<int8_t*>(p.actions)[o] = (int8_t)a;
            else if (p.action_dtype == 1) static_cast<int32_t*>(p.actions)[o] = a;
            else static_cast<long long*>(p.actions)[o] = a;
            const int nx = px + pibt_dx(a), ny = py + pibt_dy(a);
            if (p.path_xy) {
                p.path_xy[2 * o] = nx - r;
                p.path_xy[2 * o + 1] = ny - r;
            }
            w = ((uint32_t)nx << 16) | (uint32_t)ny;
            const bool on_target = w == tgt;
            if (planned0 && on_target && arrived_at < 0) arrived_at = h + 1;
            if (p.finish && on_target) planned = false;
            if (!p.fixed_priority) prio = (!planned || on_target) ? 0 : (int)((uint32_t)prio + 1u);
        }
    }

    if (have) {
        if (p.arrival) p.arrival[slot] = arrived_at;
        if (p.priority_out) p.priority_out[slot] = prio;
    }
}

template <int T>
hipError_t pibt_horizon_launch(const PibtPlanParams& p, hipStream_t stream) {
    const int epb = std::min(64, T / p.A);
    int log2n = 1;
    while ((1 << log2n) < 2 * p.A) ++log2n;   // epb << log2n < epb * 4A <= 4T words
    const unsigned grid = (unsigned)((p.batch + epb - 1) / epb);
    if (p.cell_bytes == 4)
        hipLaunchKernelGGL((pibt_horizon_kernel<T, uint32_t>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    else
        hipLaunchKernelGGL((pibt_horizon_kernel<T, uint16_t>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pibt_plan(const PibtPlanParams& p, hipStream_t stream) {
    return p.A <= 256 ? pibt_horizon_launch<256>(p, stream) : pibt_horizon_launch<1024>(p, stream);
}

}  // namespace pgx
