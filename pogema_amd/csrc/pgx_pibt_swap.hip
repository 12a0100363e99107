// pgx_pibt_swap.hip -- cooperative one-step planner with the swap operation (pgx_pibt_swap_actions, docs/SPEC.md S23):
// pgx_pibt.hip's planner plus the rule that lets two agents change places in a corridor or a dead end -- an agent whose
// best cell leads into a corridor behind an agent that wants out tries its candidates back to front and pulls that
// agent into the cell it leaves.
//
// Lane layout and launch shape are pgx_pibt.hip's: one lane per agent, min(64, floor(T / A)) whole envs per workgroup,
// the serial phase of all envs side by side in wave 0.  What is added:
//   phase 1 (parallel, every lane): partners(i) of S23 depends on the state only, never on the recursion, so both
//       corridor walks (swap_required, swap_possible) run here, one lane per agent, and leave two agent indices per
//       lane (`usual`, `clear`; 16 bits each).  Both partners stand on a neighbour cell, so a lane whose sweep found
//       no planned agent there walks nowhere.  The walks read the padded obstacle bitmap and distance fields -- the
//       lane's own, and for a `clear` partner that neighbour's -- and ask `now(c)` of arbitrary cells.  That is answered
//       by a per-env hash table cell -> lowest planned agent: open addressing over 2^ceil(log2(2A)) words, one word per
//       cell = x : 11 | y : 11 | agent : 10 (padded coordinates are below 2048, agents below 1024), filled by every
//       planned lane with one atomicCAS (free word) or atomicMin (the cell's word) -- whatever the order of arrival the
//       table answers the same.  It lives in the words of the reservation set, which phase 2 only needs afterwards and
//       which are cleared again in between: no LDS is added for it.  (The alternative, a sweep over the env's staged
//       positions per query, was not built: a walk step asks up to three cells, each a sweep of A LDS reads against a
//       probe sequence of a table that is at most half full, and a walk may take PGX_SWAP_MAX_WALK steps.)
//       Every walk has the trip count PGX_SWAP_MAX_WALK + 1 whatever a field holds, every probe sequence the table's size.
//   phase 2 (serial per env, LDS only): pibt_swap_serial (pgx_pibt_swap.h, as the table and the walks: the
//       lookahead of pgx_pibt_swap_horizon.hip uses them too), pgx_pibt_plan.h's recursion-as-a-loop with three more
//       pieces of work per call: it chooses `sw` (one read of act[usual]), walks the packed candidate list from its end
//       when `sw` exists, and after a success whose first-tried candidate held, pulls `sw` -- for every caller up the
//       chain, innermost first, as the recursion returns (a chain none of whose calls chose a partner is not walked).
// Measured against pibt_actions() on the same states (docs/EXPERIMENTS.md): 1.8x to 1.9x per call at 8192 envs x 64
// agents, of which the walks are about 50 us, the table 5 us and the heavier serial loop about 105 us.
// LDS: 51 bytes per lane + 256 (13 KB / 51.25 KB), static.  The grid depends on batch and A only; nothing but the
// caller's outputs is written.
#include "pgx_pibt_swap.h"

namespace pgx {
namespace {

template <int T, typename F>
__global__ void __launch_bounds__(T) pibt_swap_kernel(const PibtParams p, int epb, int log2n) {
    __shared__ uint32_t s_pos[T];             // packed padded cell of a planned agent, PIBT_FAR otherwise
    __shared__ uint32_t s_tgt[T];             // packed padded target
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

    uint32_t w = PIBT_FAR, tgt = PIBT_FAR;
    bool planned = false;
    int prio = 0;
    if (have) {
        w = p.pos[slot];
        tgt = p.tgt[slot];
        planned = (p.active[slot] & ACTIVE_BIT) != 0;
        if (p.priority) prio = p.priority[slot];
    }
    s_pos[t] = planned ? w : PIBT_FAR;
    s_tgt[t] = tgt;
    s_prio[t] = prio;
    s_act[t] = planned ? PIBT_UNSET : (uint8_t)0;
    s_sw[t] = SWAP_NONE | (SWAP_NONE << 16);
    s_len[t] = 0;
    if (t < 64) s_n[t] = 0u;
    for (int q = t; q < (epb << log2n); q += T) s_set[q] = PIBT_EMPTY;

    // the five candidate cells and their distances: loads first, the table and the sweep below hide them
    const int px = (int)(w >> 16), py = (int)(w & 0xFFFFu);
    const uint32_t* bm = p.obst + (size_t)(env0 + el) * p.bmw;
    const size_t cells = (size_t)p.H * p.W;
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
    __syncthreads();
    if (planned) swap_now_insert(s_set + ((size_t)el << log2n), log2n, w, i);
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
        unsigned long long beside = 0ull;     // now() of the four neighbour cells, 16 bits each
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

        // partners(i): the walks of S23 from the agent's best cell.  Both partners stand beside the agent, so a lane with
        // no planned agent on its four neighbour cells -- most lanes of a sparse map -- walks nowhere.
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
    __syncthreads();
    for (int q = t; q < (epb << log2n); q += T) s_set[q] = PIBT_EMPTY;
    __syncthreads();

    pibt_swap_serial(PibtLds{s_pos, s_prio, s_set, s_cand, s_order, s_par, s_ci, s_act, s_n}, SwapLds{s_sw, s_len, s_swc},
                     nenv, A, log2n);
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
hipError_t pibt_swap_launch(const PibtParams& p, hipStream_t stream) {
    const int epb = std::min(64, T / p.A);
    int log2n = 1;
    while ((1 << log2n) < 2 * p.A) ++log2n;   // epb << log2n < epb * 4A <= 4T words
    const unsigned grid = (unsigned)((p.batch + epb - 1) / epb);
    if (p.cell_bytes == 4) hipLaunchKernelGGL((pibt_swap_kernel<T, uint32_t>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    else hipLaunchKernelGGL((pibt_swap_kernel<T, uint16_t>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pibt_swap(const PibtParams& p, hipStream_t stream) {
    return p.A <= 256 ? pibt_swap_launch<256>(p, stream) : pibt_swap_launch<1024>(p, stream);
}

}  // namespace pgx
