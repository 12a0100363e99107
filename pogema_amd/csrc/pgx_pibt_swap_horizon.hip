// pgx_pibt_swap_horizon.hip -- multi-step planner with the swap operation (pgx_pibt_swap_plan, docs/SPEC.md S27): the
// one-step planner of pgx_pibt_swap.hip (S23) iterated `horizon` times inside one launch, on a private copy of the
// positions, with S16's planned / arrived / priority rules -- pibt_swap_kernel's body inside pibt_horizon_kernel's loop.
//
// Lane layout and launch shape are those of the other planners: one lane per agent, min(64, floor(T / A)) whole envs
// per workgroup, T = 256 lanes while A <= 256, 1024 above, the serial phase of all envs side by side in wave 0.
//   across the steps a lane keeps in registers: its agent's packed padded cell, planned flag, priority, the packed
//       target word and the first step at which the agent stood on its target (as pibt_horizon_kernel).  The env's
//       packed targets are staged in LDS once, before the loop: parked() of S23 asks for other agents' targets, and the
//       targets, with them the distance fields, are held for the whole lookahead.
//   every step h, on pos_h and planned_h:
//       1. the lane re-stages its cell, priority and action and clears its partner word and list length; the workgroup
//          clears the table words and the per-env counts;
//       2. the five field loads at the new cell are issued;                                           -- barrier A
//       3. every planned lane inserts its cell into its env's table cell -> lowest planned agent;      -- barrier B
//       4. sweep, sort, and S23's walks from the new cell (a lane with no planned neighbour walks nowhere; the walks
//          are dependent loads from the lane's own and a neighbour's field, at most PGX_SWAP_MAX_WALK + 1 trips);
//                                                                                                     -- barrier C
//       5. the table's words are cleared: they become the reservation sets;                            -- barrier D
//       6. pibt_swap_serial (pgx_pibt_swap.h);                                                         -- barrier E
//       7. the lane stores row h of `actions` and `path_xy`, moves, and applies S16's rules.
//   after the last step: `arrival` and `priority_out`.
// An agent that stopped being planned under `finish` is staged as PIBT_FAR and is not inserted: it is in nobody's
// now(), is nobody's partner and parks nowhere.
//
// Five barriers per step; every lane of the workgroup runs all `horizon` steps, planned or not.  Which barrier protects
// which array from the next writer:
//   A  s_pos, s_prio, s_act, s_sw, s_len, s_n, s_set (staged in 1; before the loop also s_tgt)  ->  the inserts of 3
//      (s_set), the sweep of 4 (s_pos, s_prio), the atomic counts of 4 (s_n)
//   B  s_set as the table (filled in 3)  ->  the walks of 4 that read it
//   C  the walks' reads of s_set  ->  the clear of 5;  s_cand, s_order, s_len, s_sw, s_n (written in 4)  ->  6
//   D  s_set cleared  ->  6, which fills it as the reservation set
//   E  everything 6 reads or writes (s_pos, s_act, s_sw, s_len, s_n, s_set, s_cand, s_order, s_par, s_ci, s_swc)  ->
//      the lane's read of s_act[t] in 7, and step h + 1's staging, which overwrites s_pos[t], s_prio[t], s_act[t],
//      s_sw[t], s_len[t] (the lane's own words, s_act[t] after its own read in program order), s_n and s_set (which
//      nobody reads any more).  s_cand, s_order, s_par, s_ci and s_swc are next written behind barrier B of step h + 1.
// Every loop is bounded by a host argument or the cap: probe sequences by the table's size, walks by
// PGX_SWAP_MAX_WALK + 1, the serial loop by 7 A + 2, the steps by `horizon`.
// Measured against pibt_plan() on the same states (docs/EXPERIMENTS.md): 2.4x to 2.5x per call at 8192 envs x 64 agents,
// 2.9x to 3.1x at 1024 envs x 8 agents; per step of the lookahead the walks are 50 to 77 us at the larger shape, the
// table 3 to 6 us and the heavier serial loop about 145 us.
// LDS: 51 bytes per lane + 256 (13312 B / 52480 B), static, as pibt_swap_kernel.  The grid depends on batch and A only;
// nothing but the caller's outputs is written.
#include "pgx_pibt_swap.h"

namespace pgx {
namespace {

enum : uint32_t { LANE_HAVE = 1u, LANE_PLANNED = 2u, LANE_FINISH = 4u, LANE_GROW = 8u, LANE_PATH = 16u };

template <int T, typename F>
__global__ void __launch_bounds__(T) pibt_swap_horizon_kernel(const PibtPlanParams p, int epb, int log2n) {
    __shared__ uint32_t s_pos[T];             // packed padded cell of a planned agent, PIBT_FAR otherwise
    __shared__ uint32_t s_tgt[T];             // packed padded target, staged once
    __shared__ int32_t s_prio[T];
    __shared__ uint32_t s_set[4 * T];         // phase 1: the envs' cell -> agent tables; phase 2: their reservation sets
    __shared__ uint32_t s_sw[T];              // the agent's partners
    __shared__ uint16_t s_cand[5 * T];        // sorted candidate lists
    __shared__ uint16_t s_order[T];           // the env's planned agents by (-prio, index)
    __shared__ uint16_t s_par[T];             // phase 2: the agent's caller
    __shared__ uint16_t s_swc[T];             // phase 2: the partner the agent's call chose
    __shared__ uint8_t s_ci[T];               // phase 2: candidates of the agent already tried
    __shared__ uint8_t s_len[T];              // candidates in the agent's list
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
    size_t o = slot;                          // the lane's element of row h
    const size_t cells = (size_t)p.H * p.W;

    uint32_t w = PIBT_FAR, tgt = PIBT_FAR;
    bool planned0 = false;
    int prio = 0;
    if (have) {
        w = p.pos[slot];
        tgt = p.tgt[slot];
        planned0 = (p.active[slot] & ACTIVE_BIT) != 0;
        if (p.priority) prio = p.priority[slot];
    }
    // -1: not arrived yet, -2: not planned at the start, never reported as arrived
    int arrived_at = !planned0 ? -2 : w == tgt ? 0 : -1;
    // What a lane decides by in every step, as bits of one vector register.  As booleans they are lane masks in pairs of
    // scalar registers for the whole loop, the uniform ones too, and with them the kernel runs out of scalar registers
    // (measured: 9 spilled); the empty asm at the head of a step keeps the word where it is and its tests inside the step.
    uint32_t lane = (have ? LANE_HAVE : 0u) | (planned0 ? LANE_PLANNED : 0u) | (p.finish ? LANE_FINISH : 0u) |
                    (p.fixed_priority ? 0u : LANE_GROW) | (p.path_xy ? LANE_PATH : 0u);
    const uint32_t* bm = p.obst + (size_t)(env0 + el) * p.bmw;
    s_tgt[t] = tgt;

    for (int h = 0; h < p.horizon; ++h) {
        asm volatile("" : "+v"(lane));
        const bool planned = (lane & LANE_PLANNED) != 0u;
        s_pos[t] = planned ? w : PIBT_FAR;
        s_prio[t] = prio;
        s_act[t] = planned ? PIBT_UNSET : (uint8_t)0;
        s_sw[t] = SWAP_NONE | (SWAP_NONE << 16);
        s_len[t] = 0;
        if (t < 64) s_n[t] = 0u;
        for (int q = t; q < (epb << log2n); q += T) s_set[q] = PIBT_EMPTY;

        // the five candidate cells and their distances: loads first, the table and the sweep below hide them
        const int px = (int)(w >> 16), py = (int)(w & 0xFFFFu);
        uint32_t cell[5], dist[5];
        if (planned) {
            const F* f = static_cast<const F*>(p.field) + slot * cells;
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
        __syncthreads();                      // A
        if (planned) swap_now_insert(s_set + ((size_t)el << log2n), log2n, w, i);
        __syncthreads();                      // B

        if (planned) {
            uint32_t occ[5];
#pragma unroll
            for (int a = 0; a < 5; ++a) occ[a] = 0xFFFFu;
            int rank = 0;
            for (int j = 0; j < A; ++j) {     // lanes of one env read the same word: an LDS broadcast
                const uint32_t wj = s_pos[base + j];
                const int pj = s_prio[base + j];
#pragma unroll
                for (int a = 0; a < 5; ++a)
                    if (wj == cell[a] && occ[a] == 0xFFFFu) occ[a] = (uint32_t)j;
                rank += (wj != PIBT_FAR && (pj > prio || (pj == prio && j < i))) ? 1 : 0;
            }
            unsigned long long beside = 0ull; // now() of the four neighbour cells, 16 bits each
#pragma unroll
            for (int a = 1; a < 5; ++a) beside |= (unsigned long long)occ[a] << (16 * (a - 1));
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
            int len = 0;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const uint32_t k = (uint32_t)key[q];
                s_cand[5 * t + q] = key[q] == PIBT_DROP
                                        ? PIBT_END
                                        : (uint16_t)(((k >> 12) & 7u) | (((k >> 15) & 1u) << 3) | ((k & 0x3FFu) << 4));
                len += key[q] == PIBT_DROP ? 0 : 1;
            }
            s_len[t] = (uint8_t)len;
            s_order[base + rank] = (uint16_t)i;
            atomicAdd(&s_n[el], 1u);

            // partners(i) on pos_h: the walks of S23 from the agent's best cell.  Both partners stand beside the agent, so
            // a lane with no planned agent on its four neighbour cells walks nowhere.
            const uint32_t k0 = (uint32_t)key[0];
            const int a0 = (int)((k0 >> 12) & 7u);
            if (key[0] != PIBT_DROP && a0 != 0 && beside != ~0ull) {
                const F* fields = static_cast<const F*>(p.field) + (size_t)(env0 + el) * A * cells;
                const SwapView<F> sv{bm, fields, s_tgt + base, s_set + ((size_t)el << log2n), cells, p.H, p.W, r, p.wpr, log2n};
                const uint32_t best = sv.step(w, a0);
                if (sv.possible(best, w)) {
                    uint32_t usual = SWAP_NONE, clear = SWAP_NONE;
                    for (int q = 0; q < 5; ++q) {  // q = 0: the agent on `best`; 1..4: the neighbours in MOVES order
                        int pusher = i, puller = i;
                        if (q == 0) {
                            if (!((k0 >> 15) & 1u)) continue;
                            puller = (int)(k0 & 0x3FFu);
                        } else {
                            const uint32_t k = (uint32_t)(beside >> (16 * (q - 1))) & 0xFFFFu;
                            if (k == 0xFFFFu || sv.step(w, q) == best) continue;
                            pusher = (int)k;
                        }
                        if (!sv.required(pusher, puller, w, best)) continue;
                        if (q == 0) {
                            usual = (uint32_t)puller;
                        } else {
                            clear = (uint32_t)pusher;
                            break;
                        }
                    }
                    s_sw[t] = usual | (clear << 16);
                }
            }
        }
        __syncthreads();                      // C
        for (int q = t; q < (epb << log2n); q += T) s_set[q] = PIBT_EMPTY;
        __syncthreads();                      // D

        pibt_swap_serial(PibtLds{s_pos, s_prio, s_set, s_cand, s_order, s_par, s_ci, s_act, s_n},
                         SwapLds{s_sw, s_len, s_swc}, nenv, A, log2n);
        __syncthreads();                      // E

        // row h of the outputs, then S16's dynamics
        if (lane & LANE_HAVE) {
            const int a = s_act[t];
            if (p.action_dtype == 0) static_cast<int8_t*>(p.actions)[o] = (int8_t)a;
            else if (p.action_dtype == 1) static_cast<int32_t*>(p.actions)[o] = a;
            else static_cast<long long*>(p.actions)[o] = a;
            const int nx = px + pibt_dx(a), ny = py + pibt_dy(a);
            if (lane & LANE_PATH) {
                p.path_xy[2 * o] = nx - r;
                p.path_xy[2 * o + 1] = ny - r;
            }
            w = ((uint32_t)nx << 16) | (uint32_t)ny;
            const bool on_target = w == tgt;
            if (on_target && arrived_at == -1) arrived_at = h + 1;
            if ((lane & LANE_FINISH) && on_target) lane &= ~LANE_PLANNED;
            if (lane & LANE_GROW) prio = (!(lane & LANE_PLANNED) || on_target) ? 0 : (int)((uint32_t)prio + 1u);
            o += row;
        }
    }

    if (lane & LANE_HAVE) {
        if (p.arrival) p.arrival[slot] = max(arrived_at, -1);
        if (p.priority_out) p.priority_out[slot] = prio;
    }
}

template <int T>
hipError_t pibt_swap_horizon_launch(const PibtPlanParams& p, hipStream_t stream) {
    const int epb = std::min(64, T / p.A);
    int log2n = 1;
    while ((1 << log2n) < 2 * p.A) ++log2n;   // epb << log2n < epb * 4A <= 4T words
    const unsigned grid = (unsigned)((p.batch + epb - 1) / epb);
    if (p.cell_bytes == 4)
        hipLaunchKernelGGL((pibt_swap_horizon_kernel<T, uint32_t>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    else
        hipLaunchKernelGGL((pibt_swap_horizon_kernel<T, uint16_t>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pibt_swap_plan(const PibtPlanParams& p, hipStream_t stream) {
    return p.A <= 256 ? pibt_swap_horizon_launch<256>(p, stream) : pibt_swap_horizon_launch<1024>(p, stream);
}

}  // namespace pgx
