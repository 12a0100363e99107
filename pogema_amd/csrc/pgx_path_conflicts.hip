// pgx_path_conflicts.hip -- where K-step paths collide, per agent (pgx_path_conflicts, docs/SPEC.md S26).
//
// The caller gives every agent K cells (pgx_pibt_plan's path_xy or pgx_agent_forecasts' cells); the kernel reports per
// agent the first step at which its path meets another agent's, with whom, how (vertex / edge / follow) and how many
// such incidences the K steps hold.  Cells are keys, never moves: nothing is read at an address computed from one.
//
// One launch, no distance field, no allocation.  Environments are packed into workgroups as pgx_pibt.hip packs them:
// one lane per agent, a workgroup holds min(64, floor(T / A)) whole envs (T = 256 lanes while A <= 256, 1024 above).
// Each env owns two hash sets in LDS, of 2^ceil(log2(2A)) words each, keyed by the cell index x * W + y (< 2^20): the
// set of step h holds the agents that take part at h, the other one those of step h - 1, and they swap roles every
// step.  A word packs key << 11 | head: the head is the last agent pushed onto the cell, s_next[] links the others (a
// chain per cell, in arbitrary order; 0x7FF ends it).  A word is claimed and pushed onto in one LDS compare-and-swap:
// linear probing from (key * 0x9E3779B1) >> (32 - log2n), never more than half full.  Per step:
//     clear the set of step h, publish the lane's key (all ones: takes no part)          | barrier
//     insert the lanes that take part                                                    | barrier
//     vertex: walk the chain of the own cell in set h; edge / follow: look the cell moved to up in set h - 1 and walk
//     its chain, comparing the keys of step h that the chain's agents published  | barrier
// The four results stay in registers over the K steps and are stored once.  They are a minimum, an OR and two sums over
// sets, so the order of a chain does not show.
// Work is O(A K) per env when cells are shared by few agents; A agents on one cell walk A^2 links, no more: the step
// loop has K trips from the host, a probe at most 2^log2n + A (a failed compare-and-swap means another lane's
// succeeded, and each lane succeeds once), a chain walk at most A.  Every LDS address derives from a lane index below
// A or from a hash masked to the env's set; path values select nothing but the key.
// The cell of step h + 1 is loaded before the barriers of step h, so that the only global-memory latency of a step
// hides behind them.
//
// LDS: 40 bytes per lane, static (10 KB / 40 KB).  Resources (-Rpass-analysis=kernel-resource-usage, gfx950, -O3): 37
// VGPRs and 66 SGPRs for the plan layout, 36 and 64 for the cells layout, with 256 and with 1024 lanes; no scratch,
// occupancy 8 waves per SIMD (tests/test_path_conflicts.py).  Measured on an MI355X per call (docs/EXPERIMENTS.md),
// forecast cells, all kinds: 8192 envs x 64 agents 47 us with K = 3 and 86 us with K = 8, where the torch all-pairs
// composition of the same outputs takes 4156 and 9049 us and the forecasts themselves 132 and 290 us; 1024 envs x 8
// agents 25 us against 481 us; 256 envs x 1024 agents (one env per workgroup) 64 us against 21113 us.
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr uint32_t PC_EMPTY = 0xFFFFFFFFu;   // a free word of a set (its key part matches no cell)
constexpr uint32_t PC_NONE = 0xFFFFFFFFu;    // the key of an agent that takes no part in a step
constexpr uint32_t PC_END = 0x7FFu;          // end of a chain (= the head part of PC_EMPTY)
constexpr int PC_HEAD_BITS = 11;             // local agent indices are < 1024

__device__ __forceinline__ uint32_t pc_hash(uint32_t key, int log2n) { return (key * 0x9E3779B1u) >> (32 - log2n); }

// T: lanes per workgroup; LAYOUT: CONFLICT_PATHS_*
template <int T, int LAYOUT>
__global__ void __launch_bounds__(T) path_conflicts_kernel(const ConflictParams p, int epb, int log2n) {
    __shared__ uint32_t s_set[2][4 * T];      // the envs' sets of the step and of the step before: key << 11 | head
    __shared__ uint16_t s_next[2][T];         // the chains' links, per set
    __shared__ uint32_t s_key[T];             // the agents' keys of the step, PC_NONE: no part

    const int t = threadIdx.x;
    const int A = p.A, K = p.steps, H = p.H, W = p.W;
    const int env0 = blockIdx.x * epb;
    const int nenv = min(epb, p.batch - env0);
    const int el = t / A, i = t - el * A, base = el * A;
    const bool have = el < nenv;
    const size_t env = (size_t)(env0 + el), slot = env * A + i;
    const uint32_t nslots = 1u << log2n, mask = nslots - 1u;
    const uint32_t set0 = have ? (uint32_t)el << log2n : 0u;   // the env's words in a set
    const int max_probe = (int)nslots + A;

    // step h's cell of this lane's agent, h = 1..K
    auto read_cell = [&](int h, int& x, int& y) {
        if constexpr (LAYOUT == CONFLICT_PATHS_PLAN) {
            const int32_t* q = static_cast<const int32_t*>(p.paths) + (((size_t)(h - 1) * p.batch + env) * A + i) * 2;
            x = q[0], y = q[1];
        } else {
            const int16_t* q = static_cast<const int16_t*>(p.paths) + (slot * K + (size_t)(h - 1)) * 2;
            x = q[0], y = q[1];
        }
    };

    bool live = false;                        // bit 0 of `active`
    int x = -1, y = -1, tx = -2, ty = -2;     // the cell of the step (unpadded), the target
    if (have) {
        live = (p.active[slot] & ACTIVE_BIT) != 0;
        const uint32_t pp = p.pos[slot], tt = p.tgt[slot];
        x = (int)(pp >> 16) - p.r, y = (int)(pp & 0xFFFFu) - p.r;
        tx = (int)(tt >> 16) - p.r, ty = (int)(tt & 0xFFFFu) - p.r;
    }
    int nx = -1, ny = -1;                     // the cell of the next step, loaded one step ahead
    if (live) read_cell(1, nx, ny);

    bool gone = false;                        // vanish: an earlier cell of the path was the target
    uint32_t kp = PC_NONE;                    // the key of the step before
    int first = -1, partner = -1, count = 0;
    uint32_t kind = 0u;

    for (int h = 0; h <= K; ++h) {            // K + 1 trips whatever the paths hold; step 0 only fills its set
        const int cur = h & 1, prev = cur ^ 1;
        uint32_t* set_c = s_set[cur] + set0;
        const uint32_t* set_p = s_set[prev] + set0;
        for (int q = t; q < (epb << log2n); q += T) s_set[cur][q] = PC_EMPTY;
        const bool inside = x >= 0 && x < H && y >= 0 && y < W;
        const uint32_t k = live && inside && !gone ? (uint32_t)(x * W + y) : PC_NONE;
        s_key[t] = k;
        if (p.vanish && x == tx && y == ty) gone = true;   // from the next step on
        x = nx, y = ny;
        if (live && h + 2 <= K) read_cell(h + 2, nx, ny);
        __syncthreads();                      // the set is clear, the keys are published

        uint32_t mine = PC_EMPTY;             // the word of the own cell in the step's set
        if (k != PC_NONE) {
            const uint32_t word = (k << PC_HEAD_BITS) | (uint32_t)i;
            uint32_t s = pc_hash(k, log2n);
            uint32_t old = set_c[s];
            for (int n = 0; n < max_probe; ++n) {
                if (old == PC_EMPTY || (old >> PC_HEAD_BITS) == k) {
                    const uint32_t got = atomicCAS(&set_c[s], old, word);
                    if (got == old) {         // claimed, or pushed in front of the cell's chain
                        s_next[cur][t] = (uint16_t)(old & PC_END);
                        mine = s;
                        break;
                    }
                    old = got;
                } else {
                    s = (s + 1u) & mask;
                    old = set_c[s];
                }
            }
        }
        __syncthreads();                      // the step's set and chains are complete

        if (h > 0 && k != PC_NONE) {
            int n_here = 0, low = 0x7FFFFFFF;
            uint32_t kinds = 0u;
            if ((p.kinds & CONFLICT_VERTEX) && mine != PC_EMPTY) {
                uint32_t j = set_c[mine] & PC_END;
                for (int n = 0; n < A && j != PC_END; ++n) {
                    if ((int)j != i) {
                        ++n_here;
                        low = min(low, (int)j);
                        kinds |= CONFLICT_VERTEX;
                    }
                    j = s_next[cur][base + j];
                }
            }
            if ((p.kinds & (CONFLICT_EDGE | CONFLICT_FOLLOW)) && kp != PC_NONE && kp != k) {
                // the agents that stood on the cell moved to, a step ago
                uint32_t j = PC_END;
                uint32_t s = pc_hash(k, log2n);
                for (uint32_t n = 0; n < nslots; ++n, s = (s + 1u) & mask) {
                    const uint32_t v = set_p[s];
                    if (v == PC_EMPTY) break;
                    if ((v >> PC_HEAD_BITS) == k) {
                        j = v & PC_END;
                        break;
                    }
                }
                for (int n = 0; n < A && j != PC_END; ++n) {
                    const uint32_t kj = s_key[base + j];   // (its key of the step before is k: never this lane)
                    uint32_t bit = 0u;
                    if (kj == kp) bit = CONFLICT_EDGE;                            // it moves to where this one was
                    else if (kj != PC_NONE && kj != k) bit = CONFLICT_FOLLOW;    // it moves on, elsewhere
                    if (bit & p.kinds) {
                        ++n_here;
                        low = min(low, (int)j);
                        kinds |= bit;
                    }
                    j = s_next[prev][base + j];
                }
            }
            if (n_here) {
                count += n_here;
                if (first < 0) first = h, partner = low, kind = kinds;
            }
        }
        kp = k;
        __syncthreads();                      // the walks are over: the older set may be cleared
    }

    if (have) {
        if (p.first_step) p.first_step[slot] = first;
        if (p.partner) p.partner[slot] = partner;
        if (p.kind) p.kind[slot] = (uint8_t)kind;
        if (p.count) p.count[slot] = count;
    }
}

template <int T>
hipError_t path_conflicts_launch(const ConflictParams& p, hipStream_t stream) {
    const int epb = std::min(64, T / p.A);
    int log2n = 1;
    while ((1 << log2n) < 2 * p.A) ++log2n;   // epb << log2n < epb * 4A <= 4T words
    const dim3 grid((unsigned)((p.batch + epb - 1) / epb)), block(T);
    if (p.layout == CONFLICT_PATHS_PLAN)
        hipLaunchKernelGGL((path_conflicts_kernel<T, CONFLICT_PATHS_PLAN>), grid, block, 0, stream, p, epb, log2n);
    else
        hipLaunchKernelGGL((path_conflicts_kernel<T, CONFLICT_PATHS_CELLS>), grid, block, 0, stream, p, epb, log2n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_path_conflicts(const ConflictParams& p, hipStream_t stream) {
    return p.A <= 256 ? path_conflicts_launch<256>(p, stream) : path_conflicts_launch<1024>(p, stream);
}

}  // namespace pgx
