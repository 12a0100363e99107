// pgx_outcomes.hip -- move outcomes (pgx_move_outcomes, docs/SPEC.md S17): what the move phase of pgx_step would do to
// each agent's action, and why a move that fails does.  The resolve phase of the step without its state write-back and
// without the observation stream: one launch that reads the state and the caller's actions and writes nothing but the
// caller's outputs.
//
// A lane per agent, T = 256 lanes (A <= 256, min(64, T / A) envs per workgroup) or 1024, the shape of pibt_kernel.
//   phase 1: a lane loads its cell, its `active` byte and its action, tests its destination against the padded obstacle
//       bitmap (the ring around the map is part of it, so the large-map range needs no second layout) and stages
//       pos = its cell if active and want = its destination if it is a mover.
//   phase 2: a mover sweeps the env's staged lanes (LDS broadcasts): o = lowest other agent standing on its destination,
//       cmin = lowest other mover claiming it, c1 = largest such claimant below the own index.  `stay` is S2's closed
//       form of the engine's collision system; under `priority` and `soft` the transitive "the agent on my destination
//       stays" follows by pointer doubling over o in LDS, at most ceil(log2 A) rounds, ended early when no chain of the
//       workgroup is open.
//   phase 3: the code from stay, stay of o and the claimant data (first rule of S17's table that applies); per-env counts
//       from wave ballots, gathered in LDS: no global atomics.
// LDS: 17 bytes per lane + 1.9 KB (6.2 KB / 19 KB), static.  The grid depends on batch and A only.
#include <algorithm>

#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr uint32_t OUT_FAR = 0x7FFF7FFFu;     // staged cell of an inactive agent: no destination equals it
constexpr uint32_t OUT_NONE = 0xFFFFFFFEu;    // staged destination of an agent that is no mover: no cell equals it
constexpr int OUT_CODES = 7;                  // PGX_NUM_OUTCOMES
constexpr int OUT_ROUNDS = 10;                // ceil(log2(1024)): the most rounds of the closure

__device__ __forceinline__ int out_dx(int a) { return (a == 2) - (a == 1); }  // MOVES: noop, up, down, left, right
__device__ __forceinline__ int out_dy(int a) { return (a == 4) - (a == 3); }

template <int T>
__global__ void __launch_bounds__(T) outcomes_kernel(const OutcomeParams p, int epb) {
    __shared__ uint32_t s_pos[T];
    __shared__ uint32_t s_want[T];
    __shared__ uint32_t s_x0[T];
    __shared__ uint32_t s_x1[T];
    __shared__ uint8_t s_stay[T];
    __shared__ uint32_t s_cnt[64 * OUT_CODES];
    __shared__ uint32_t s_open[OUT_ROUNDS];

    const int t = threadIdx.x;
    const int A = p.A;
    const int env0 = blockIdx.x * epb;
    const int nenv = min(epb, p.batch - env0);
    const int el = t / A;
    const int i = t - el * A;
    const int base = el * A;
    const int env = env0 + el;
    const bool have = el < nenv;
    const size_t slot = (size_t)env * A + i;

    // ---- phase 1 ----
    uint32_t w = OUT_FAR;
    bool active = false;
    int act = 0;
    if (have) {
        w = p.pos[slot];
        active = (p.active[slot] & ACTIVE_BIT) != 0;
        if (p.action_dtype == 0) act = static_cast<const int8_t*>(p.actions)[slot];
        else if (p.action_dtype == 1) act = static_cast<const int32_t*>(p.actions)[slot];
        else act = (int)static_cast<const long long*>(p.actions)[slot];   // as the step narrows it
        if (act < 0 || act > 4) act = 0;
    }
    const bool mover = active && act != 0;
    const int px = (int)(w >> 16), py = (int)(w & 0xFFFFu);
    const int vx = px + out_dx(act), vy = py + out_dy(act);
    const uint32_t d = ((uint32_t)vx << 16) | (uint32_t)vy;
    bool blocked = false;
    if (mover) {
        blocked = true;                       // (a cell beyond the padded bitmap cannot be reached from inside the map)
        if (vx >= 0 && vx < p.H + 2 * p.r && vy >= 0 && vy < p.W + 2 * p.r)
            blocked = ((p.obst[(size_t)env * p.bmw + (size_t)vx * p.wpr + (vy >> 5)] >> (vy & 31)) & 1u) != 0;
    }
    s_pos[t] = active ? w : OUT_FAR;
    s_want[t] = mover ? d : OUT_NONE;
    for (int q = t; q < 64 * OUT_CODES; q += T) s_cnt[q] = 0u;
    if (t < OUT_ROUNDS) s_open[t] = 0u;
    __syncthreads();

    // ---- phase 2 ----
    int o = -1, cmin = -1, c1 = -1;
    if (mover) {
        for (int j = 0; j < A; ++j) {
            const uint32_t pj = s_pos[base + j], qj = s_want[base + j];
            if (j == i) continue;
            if (pj == d && o < 0) o = j;
            if (qj == d) {
                if (cmin < 0) cmin = j;
                if (j < i) c1 = j;
            }
        }
    }
    const bool swap = o >= 0 && s_want[base + o] == w;
    bool stay;
    if (p.collision == COLLISION_BLOCK_BOTH) {
        stay = !mover || blocked || o >= 0 || cmin >= 0;
    } else {
        if (p.collision == COLLISION_PRIORITY) stay = !mover || blocked || o > i || c1 > o;
        else stay = !mover || blocked || (p.all_stay ? cmin >= 0 : c1 >= 0) || swap;
        int nxt = mover ? o : -1;
        int rounds = 1;
        while ((1 << rounds) < A) ++rounds;
        for (int it = 0; it < rounds; ++it) {  // block-uniform
            uint32_t* buf = (it & 1) ? s_x1 : s_x0;
            buf[t] = (stay ? 0x80000000u : 0u) | (uint32_t)(nxt + 1);
            if (nxt >= 0 && !stay) s_open[it] = 1u;
            __syncthreads();
            if (s_open[it] == 0u) break;
            if (nxt >= 0) {
                const uint32_t got = buf[base + nxt];
                stay = stay || (got >> 31);
                nxt = (int)(got & 0x7FFFFFFFu) - 1;
            }
        }
    }
    s_stay[t] = stay ? 1 : 0;
    __syncthreads();

    // ---- phase 3 ----
    int code = 0, who = -1;
    if (mover) {
        if (!stay) code = 1;
        else if (blocked) code = 2;
        else if (swap) code = 3;
        else if (o >= 0 && s_stay[base + o]) code = 4;
        else if (o >= 0 && cmin < 0) code = 5;
        else code = 6;
        who = code >= 3 && code <= 5 ? o : code == 6 ? cmin : -1;
    }
    if (have) {
        if (p.next_xy) {
            p.next_xy[2 * slot] = (stay ? px : vx) - p.r;
            p.next_xy[2 * slot + 1] = (stay ? py : vy) - p.r;
        }
        if (p.outcome) p.outcome[slot] = (uint8_t)code;
        if (p.blocker) p.blocker[slot] = who;
    }
    if (p.counts) {                           // (kernel-uniform)
        // the env's lanes inside this wave are [lo, hi); the first of them adds the wave's share to the env's row
        const int w0 = t & ~63;
        const int lo = max(base, w0) - w0, hi = min(base + A, w0 + 64) - w0;
        const unsigned long long span = (hi - lo >= 64 ? ~0ull : ((1ull << (hi - lo)) - 1ull)) << lo;
#pragma unroll
        for (int c = 0; c < OUT_CODES; ++c) {
            const unsigned long long m = __ballot(active && code == c);
            if (have && (t & 63) == lo) {
                const int n = __popcll(m & span);
                if (n) atomicAdd(&s_cnt[el * OUT_CODES + c], (uint32_t)n);
            }
        }
        __syncthreads();
        for (int q = t; q < nenv * OUT_CODES; q += T) p.counts[(size_t)env0 * OUT_CODES + q] = (int32_t)s_cnt[q];
    }
}

template <int T>
hipError_t outcomes_launch(const OutcomeParams& p, hipStream_t stream) {
    const int epb = std::min(64, T / p.A);
    const unsigned grid = (unsigned)((p.batch + epb - 1) / epb);
    hipLaunchKernelGGL((outcomes_kernel<T>), dim3(grid), dim3(T), 0, stream, p, epb);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_move_outcomes(const OutcomeParams& p, hipStream_t stream) {
    return p.A <= 256 ? outcomes_launch<256>(p, stream) : outcomes_launch<1024>(p, stream);
}

}  // namespace pgx
