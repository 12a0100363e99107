// pgx_shield.hip -- collision shielding (pgx_shield_actions, docs/SPEC.md S15): the cooperative planner of pgx_pibt.hip
// with every agent's candidate cells ordered by the caller's action scores instead of by the distance to its target.
//
// The sibling of pibt_kernel: the same lane layout, LDS, packed candidate lists, serial phase and stores
// (pgx_pibt_plan.h); only a lane's sort key differs.
//   phase 1: each planned lane issues its five score loads (f32 / f16 / bf16, [B][A][5] contiguous), the bitmap tests of
//       its five cells and, with TIE only, the five loads from its distance field, all before the sweep over the env's
//       staged positions that hides them.  A score becomes a 32-bit rank that ascends as the score descends: -0.0 is
//       +0.0, every NaN is the last rank, below -inf.  The sort key is rank << 25 | D << 4 | occupied << 3 | action
//       (57 bits; D and occupied are 0 without TIE); the occupant no longer fits and is picked by the action after the
//       sort, with compile-time indices only, so that nothing leaves the registers.
//       overridden = the planned action is not the lowest (rank, action) over all five actions, kept or not.
//   Without TIE the kernel reads no distance field: the call needs no cache, allocates nothing and is one launch.
// LDS: 40 bytes per lane + 256 (10.25 KB / 40.25 KB), static, as pibt_kernel.  The grid depends on batch and A only;
// nothing but the caller's outputs is written.
#include "pgx_pibt_plan.h"

namespace pgx {
namespace {

// ---- phase 1 and the stores, as pibt_kernel has them inline ----
// five keys ascending: a 9-comparator network, registers only
__device__ __forceinline__ void pibt_sort5(unsigned long long (&key)[5]) {
    pibt_cswap(key[0], key[1]);
    pibt_cswap(key[3], key[4]);
    pibt_cswap(key[2], key[4]);
    pibt_cswap(key[2], key[3]);
    pibt_cswap(key[1], key[4]);
    pibt_cswap(key[0], key[3]);
    pibt_cswap(key[0], key[2]);
    pibt_cswap(key[1], key[3]);
    pibt_cswap(key[1], key[2]);
}
// one entry of a candidate list: action | occupied << 3 | occupant << 4 (all ones, PIBT_END, is no entry: a <= 4);
// `occupied` is 0 or 1, `occupant` is 0 unless occupied
__device__ __forceinline__ uint16_t pibt_pack(uint32_t a, uint32_t occupied, uint32_t occupant) {
    return (uint16_t)(a | (occupied << 3) | ((occupant & 0x3FFu) << 4));
}

// the kernel's LDS arrays
template <int T>
__device__ __forceinline__ PibtLds pibt_lds() {
    __shared__ uint32_t s_pos[T];
    __shared__ int32_t s_prio[T];
    __shared__ uint32_t s_set[4 * T];
    __shared__ uint16_t s_cand[5 * T];
    __shared__ uint16_t s_order[T];
    __shared__ uint16_t s_par[T];
    __shared__ uint8_t s_ci[T];
    __shared__ uint8_t s_act[T];
    __shared__ uint32_t s_n[64];
    return PibtLds{s_pos, s_prio, s_set, s_cand, s_order, s_par, s_ci, s_act, s_n};
}

// a lane's agent
struct PibtLane {
    int nenv;                    // envs of this workgroup
    int el, i, base;             // env inside the workgroup, agent inside the env, first lane of the env
    int env;                     // env inside the batch
    bool have, planned;          // the lane has an agent; the agent is planned
    size_t slot;                 // [B][A] index of the agent
    uint32_t w;                  // its packed padded cell
    int prio;
};

// reads the lane's agent and stages it; clears the sets.  The caller's __syncthreads() publishes it.
template <int T>
__device__ __forceinline__ PibtLane pibt_stage(const PibtLds& s, const PibtParams& p, int epb, int log2n) {
    const int t = threadIdx.x;
    const int A = p.A;
    const int env0 = blockIdx.x * epb;
    PibtLane l;
    l.nenv = min(epb, p.batch - env0);
    l.el = t / A;
    l.i = t - l.el * A;
    l.base = l.el * A;
    l.env = env0 + l.el;
    l.have = l.el < l.nenv;
    l.slot = (size_t)l.env * A + l.i;
    l.w = PIBT_FAR;
    l.planned = false;
    l.prio = 0;
    if (l.have) {
        l.w = p.pos[l.slot];
        l.planned = (p.active[l.slot] & ACTIVE_BIT) != 0;
        if (p.priority) l.prio = p.priority[l.slot];
    }
    s.pos[t] = l.planned ? l.w : PIBT_FAR;
    s.prio[t] = l.prio;
    s.act[t] = l.planned ? PIBT_UNSET : (uint8_t)0;
    if (t < 64) s.n[t] = 0u;
    for (int q = t; q < (epb << log2n); q += T) s.set[q] = PIBT_EMPTY;
    return l;
}

// candidate a of an agent at padded (px, py) of env bitmap `bm`: whether it lies inside the map and off the obstacles;
// cell = its packed padded cell, or PIBT_NO_CELL when it does not; (ux, uy) = its unpadded coordinates
__device__ __forceinline__ bool pibt_cell(const PibtParams& p, const uint32_t* bm, int px, int py, int a, uint32_t& cell,
                                          int& ux, int& uy) {
    const int vx = px + pibt_dx(a), vy = py + pibt_dy(a);
    ux = vx - p.r;
    uy = vy - p.r;
    bool ok = ux >= 0 && ux < p.H && uy >= 0 && uy < p.W;
    if (ok) ok = !((bm[(size_t)vx * p.wpr + (vy >> 5)] >> (vy & 31)) & 1u);
    cell = ok ? (((uint32_t)vx << 16) | (uint32_t)vy) : PIBT_NO_CELL;
    return ok;
}

// one sweep over the env's staged agents: occ[a] = `now` of candidate cell a (PIBT_NOBODY: nobody), and the agent's
// rank in the order (-prio, index).  Lanes of one env read the same word: an LDS broadcast.
__device__ __forceinline__ int pibt_sweep(const PibtLds& s, const PibtLane& l, int A, const uint32_t (&cell)[5], uint32_t (&occ)[5]) {
#pragma unroll
    for (int a = 0; a < 5; ++a) occ[a] = PIBT_NOBODY;
    int rank = 0;
    for (int j = 0; j < A; ++j) {
        const uint32_t wj = s.pos[l.base + j];
        const int pj = s.prio[l.base + j];
#pragma unroll
        for (int a = 0; a < 5; ++a)
            if (wj == cell[a] && occ[a] == PIBT_NOBODY) occ[a] = (uint32_t)j;
        rank += (wj != PIBT_FAR && (pj > l.prio || (pj == l.prio && j < l.i))) ? 1 : 0;
    }
    return rank;
}

// the lane's outputs: action `a` and the cell it leads to from padded (px, py)
__device__ __forceinline__ void pibt_store(const PibtParams& p, const PibtLane& l, int px, int py, int a) {
    if (p.action_dtype == 0) static_cast<int8_t*>(p.actions)[l.slot] = (int8_t)a;
    else if (p.action_dtype == 1) static_cast<int32_t*>(p.actions)[l.slot] = a;
    else static_cast<long long*>(p.actions)[l.slot] = a;
    if (p.next_xy) {
        p.next_xy[2 * l.slot] = px - p.r + pibt_dx(a);
        p.next_xy[2 * l.slot + 1] = py - p.r + pibt_dy(a);
    }
}

// envs per workgroup of T lanes and log2 of the words of an env's reservation set: epb << log2n < epb * 4A <= 4T
template <int T>
inline void pibt_geometry(int batch, int A, int& epb, int& log2n, unsigned& grid) {
    epb = std::min(64, T / A);
    log2n = 1;
    while ((1 << log2n) < 2 * A) ++log2n;
    grid = (unsigned)((batch + epb - 1) / epb);
}

// ---- the scores ----
// the bits of score `idx` widened exactly to float32
template <int SD>
__device__ __forceinline__ uint32_t shield_score_bits(const void* scores, size_t idx) {
    if constexpr (SD == SCORES_F32) return static_cast<const uint32_t*>(scores)[idx];
    else if constexpr (SD == SCORES_F16) return __float_as_uint((float)static_cast<const _Float16*>(scores)[idx]);
    else return (uint32_t)static_cast<const uint16_t*>(scores)[idx] << 16;
}

// float32 bits -> a rank that ascends as the score descends; NaN last
__device__ __forceinline__ uint32_t shield_rank(uint32_t u) {
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;    // NaN: above the rank of -inf, 0xFF800000
    if (u == 0x80000000u) u = 0u;                               // -0.0 == +0.0
    return (u & 0x80000000u) ? u : ~(u | 0x80000000u);          // = ~(the usual ascending order-preserving map)
}

template <int T, int SD, typename F, bool TIE>
__global__ void __launch_bounds__(T) shield_kernel(const ShieldParams p, int epb, int log2n) {
    const PibtLds s = pibt_lds<T>();

    const int t = threadIdx.x;
    const int A = p.A;
    const PibtLane l = pibt_stage<T>(s, p, epb, log2n);

    // the five scores, candidate cells and (TIE) distances: loads first, the sweep below hides them
    const int px = (int)(l.w >> 16), py = (int)(l.w & 0xFFFFu);
    uint32_t cell[5], bits[5], dist[5];
    if (l.planned) {
        const uint32_t* bm = p.obst + (size_t)l.env * p.bmw;
#pragma unroll
        for (int a = 0; a < 5; ++a) bits[a] = shield_score_bits<SD>(p.scores, l.slot * 5 + a);
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            int ux, uy;
            const bool ok = pibt_cell(p, bm, px, py, a, cell[a], ux, uy);
            (void)ok;
            dist[a] = 0u;
            if constexpr (TIE) {
                const F* f = static_cast<const F*>(p.field) + l.slot * ((size_t)p.H * p.W);
                F d = (F)~F(0);
                if (ok) d = f[(size_t)ux * p.W + uy];
                dist[a] = d == (F)~F(0) ? PIBT_INF : (uint32_t)d;
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            cell[a] = PIBT_NO_CELL;
            bits[a] = 0u;
            dist[a] = 0u;
        }
    }
    __syncthreads();

    int best = 0;                             // argmax of the scores over all five actions, the lowest on ties
    if (l.planned) {
        uint32_t occ[5];
        const int rank = pibt_sweep(s, l, A, cell, occ);
        unsigned long long key[5], top = ~0ull;
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            const unsigned long long rk = shield_rank(bits[a]);
            const unsigned long long mine = (rk << 3) | (unsigned long long)a;
            top = mine < top ? mine : top;
            const bool other = occ[a] != PIBT_NOBODY && occ[a] != (uint32_t)l.i;
            key[a] = cell[a] == PIBT_NO_CELL
                         ? PIBT_DROP
                         : (rk << 25) | ((unsigned long long)dist[a] << 4) | ((TIE && other ? 1ull : 0ull) << 3) |
                               (unsigned long long)a;
        }
        best = (int)(top & 7ull);
        pibt_sort5(key);
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const uint32_t a = (uint32_t)key[q] & 7u;
            uint32_t o = PIBT_NOBODY;         // the occupant of candidate a's cell
#pragma unroll
            for (int c = 0; c < 5; ++c) o = a == (uint32_t)c ? occ[c] : o;
            const bool other = o != PIBT_NOBODY && o != (uint32_t)l.i;
            s.cand[5 * t + q] = key[q] == PIBT_DROP ? PIBT_END : pibt_pack(a, other ? 1u : 0u, other ? o : 0u);
        }
        s.order[l.base + rank] = (uint16_t)l.i;
        atomicAdd(&s.n[l.el], 1u);
    }
    __syncthreads();

    pibt_serial(s, l.nenv, A, log2n);
    __syncthreads();

    if (l.have) {
        const int a = s.act[t];
        pibt_store(p, l, px, py, a);
        if (p.overridden) p.overridden[l.slot] = (l.planned && a != best) ? 1 : 0;
    }
}

template <int T, int SD>
hipError_t shield_launch(const ShieldParams& p, hipStream_t stream) {
    int epb, log2n;
    unsigned grid;
    pibt_geometry<T>(p.batch, p.A, epb, log2n, grid);
    if (!p.tie_distance)
        hipLaunchKernelGGL((shield_kernel<T, SD, uint16_t, false>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    else if (p.cell_bytes == 4)
        hipLaunchKernelGGL((shield_kernel<T, SD, uint32_t, true>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    else
        hipLaunchKernelGGL((shield_kernel<T, SD, uint16_t, true>), dim3(grid), dim3(T), 0, stream, p, epb, log2n);
    return hipGetLastError();
}

template <int T>
hipError_t shield_launch(const ShieldParams& p, hipStream_t stream) {
    switch (p.score_dtype) {
        case SCORES_F32: return shield_launch<T, SCORES_F32>(p, stream);
        case SCORES_F16: return shield_launch<T, SCORES_F16>(p, stream);
        case SCORES_BF16: return shield_launch<T, SCORES_BF16>(p, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_shield(const ShieldParams& p, hipStream_t stream) {
    return p.A <= 256 ? shield_launch<256>(p, stream) : shield_launch<1024>(p, stream);
}

}  // namespace pgx
