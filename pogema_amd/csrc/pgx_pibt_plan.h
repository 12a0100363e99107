// pgx_pibt_plan.h -- what the two one-step planners share: pgx_pibt.hip (docs/SPEC.md S13, candidates ordered by the
// distance to the target) and pgx_shield.hip (S15, candidates ordered by the caller's scores).  They differ in how a
// lane orders its five candidate cells (phase 1, each kernel's own); the LDS arrays, the packed candidate lists phase 1
// leaves in them, the reservation set and the serial recursion-as-a-loop (phase 2) are the ones below.  Every function
// is inlined into the kernel that calls it; the layouts are described in pgx_pibt.hip.
#pragma once
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr uint32_t PIBT_FAR = 0x7FFF7FFFu;    // staged position of an unplanned agent: no candidate cell equals it
constexpr uint32_t PIBT_NO_CELL = 0xFFFFFFFEu;  // a candidate outside the map or on an obstacle
constexpr uint32_t PIBT_EMPTY = 0xFFFFFFFFu;  // free word of the reservation set
constexpr uint32_t PIBT_NOBODY = 0xFFFFu;     // `now` of a cell no planned agent stands on
constexpr uint16_t PIBT_END = 0xFFFFu;        // end of a candidate list
constexpr uint16_t PIBT_NONE = 0xFFFFu;       // no caller: the agent was started from the priority order
constexpr uint8_t PIBT_UNSET = 0xFFu;         // `next` not decided yet
constexpr unsigned long long PIBT_DROP = ~0ull;  // sort key of a candidate that is not kept
constexpr uint32_t PIBT_INF = (1u << 21) - 1u;   // D of an unreachable cell inside the key: above every distance (< 2^20)

__device__ __forceinline__ int pibt_dx(int a) { return (a == 2) - (a == 1); }  // MOVES: noop, up, down, left, right
__device__ __forceinline__ int pibt_dy(int a) { return (a == 4) - (a == 3); }

__device__ __forceinline__ void pibt_cswap(unsigned long long& a, unsigned long long& b) {
    const unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}
// the reservation set of one env: `set` has 1 << log2n words
__device__ __forceinline__ bool pibt_reserved(const uint32_t* set, int log2n, uint32_t cell) {
    const uint32_t mask = (1u << log2n) - 1u;
    for (uint32_t h = (cell * 0x9E3779B1u) >> (32 - log2n);; h = (h + 1u) & mask) {
        const uint32_t k = set[h];
        if (k == cell) return true;
        if (k == PIBT_EMPTY) return false;
    }
}
__device__ __forceinline__ void pibt_reserve(uint32_t* set, int log2n, uint32_t cell) {
    const uint32_t mask = (1u << log2n) - 1u;
    for (uint32_t h = (cell * 0x9E3779B1u) >> (32 - log2n);; h = (h + 1u) & mask) {
        const uint32_t k = set[h];
        if (k == cell) return;
        if (k == PIBT_EMPTY) {
            set[h] = cell;
            return;
        }
    }
}

// the workgroup's LDS, 40 bytes per lane + 256: pointers to separate __shared__ arrays of the kernel, not members of one
// struct -- the serial phase reads and writes most of them in every iteration, and only distinct variables let the
// compiler keep those accesses apart (measured: one struct slowed pibt_actions() by about 3 % at 8192 envs x 64 agents).
struct PibtLds {
    uint32_t* pos;               // [T] packed padded cell of a planned agent, PIBT_FAR otherwise
    int32_t* prio;               // [T]
    uint32_t* set;               // [4 T] the envs' reservation sets
    uint16_t* cand;              // [5 T] sorted candidate lists
    uint16_t* order;             // [T] the env's planned agents by (-prio, index)
    uint16_t* par;               // [T] phase 2: the agent's caller
    uint8_t* ci;                 // [T] phase 2: candidates of the agent already tried
    uint8_t* act;                // [T] the agent's action; PIBT_UNSET: `next` unset
    uint32_t* n;                 // [64] planned agents per env
};
// phase 2: lane e of wave 0 runs env e.  `cur` is the agent whose call is running; a call that succeeds ends the
// whole chain of its callers (each of them returns True at once), one that fails resumes its caller's loop.
__device__ __forceinline__ void pibt_serial(const PibtLds& s, int nenv, int A, int log2n) {
    const int t = threadIdx.x;
    if (t < nenv) {
        const int b = t * A;
        const int n = (int)s.n[t];
        uint32_t* set = s.set + ((size_t)t << log2n);
        int k = 0, cur = -1;
        for (;;) {
            if (cur < 0) {
                if (k >= n) break;
                const int c = s.order[b + k++];
                if (s.act[b + c] != PIBT_UNSET) continue;
                cur = c;
                s.par[b + c] = PIBT_NONE;
                s.ci[b + c] = 0;
                continue;
            }
            const int ci = s.ci[b + cur];
            const uint16_t e = ci < 5 ? s.cand[5 * (b + cur) + ci] : PIBT_END;
            const uint32_t here = s.pos[b + cur];
            const uint16_t par = s.par[b + cur];
            if (e == PIBT_END) {              // every candidate refused: stay, and hold the own cell
                s.act[b + cur] = 0;
                pibt_reserve(set, log2n, here);
                cur = par == PIBT_NONE ? -1 : (int)par;
                continue;
            }
            s.ci[b + cur] = (uint8_t)(ci + 1);
            const int a = e & 7;
            const uint32_t v = (uint32_t)((int)here + pibt_dx(a) * 65536 + pibt_dy(a));
            if (pibt_reserved(set, log2n, v)) continue;
            if (par != PIBT_NONE && v == s.pos[b + par]) continue;
            s.act[b + cur] = (uint8_t)a;
            pibt_reserve(set, log2n, v);
            const int j = e >> 4;
            if ((e & 8) && s.act[b + j] == PIBT_UNSET) {  // the cell's agent has to move on first
                s.par[b + j] = (uint16_t)cur;
                s.ci[b + j] = 0;
                cur = j;
                continue;
            }
            cur = -1;
        }
    }
}

}  // namespace
}  // namespace pgx
