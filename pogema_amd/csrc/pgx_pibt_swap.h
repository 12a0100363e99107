// pgx_pibt_swap.h -- what the two planners with the swap operation share: pgx_pibt_swap.hip (docs/SPEC.md S23, one step)
// and pgx_pibt_swap_horizon.hip (S27, the lookahead).  The per-env table cell -> lowest planned agent, the view a lane's
// corridor walks see (SwapView), the LDS arrays the swap rule adds to pgx_pibt_plan.h's (SwapLds) and the serial phase
// (pibt_swap_serial).  Every function is inlined into the kernel that calls it; pgx_pibt_swap.hip describes the phases.
#pragma once
#include "pgx_pibt_plan.h"

namespace pgx {
namespace {

constexpr uint32_t SWAP_NONE = 0xFFFFu;       // no partner

// ---- the table cell -> lowest planned agent of one env: `tab` has 1 << log2n words --------------------------------
__device__ __forceinline__ uint32_t swap_key(uint32_t cell) { return ((cell >> 16) << 11) | (cell & 0x7FFu); }

__device__ __forceinline__ void swap_now_insert(uint32_t* tab, int log2n, uint32_t cell, int agent) {
    const uint32_t mask = (1u << log2n) - 1u, key = swap_key(cell), word = (key << 10) | (uint32_t)agent;
    uint32_t h = (cell * 0x9E3779B1u) >> (32 - log2n);
    for (uint32_t n = 0; n <= mask; ++n, h = (h + 1u) & mask) {
        const uint32_t old = atomicCAS(&tab[h], PIBT_EMPTY, word);
        if (old == PIBT_EMPTY) return;
        if ((old >> 10) == key) {
            atomicMin(&tab[h], word);
            return;
        }
    }
}
__device__ __forceinline__ uint32_t swap_now(const uint32_t* tab, int log2n, uint32_t cell) {
    const uint32_t mask = (1u << log2n) - 1u, key = swap_key(cell);
    uint32_t h = (cell * 0x9E3779B1u) >> (32 - log2n);
    for (uint32_t n = 0; n <= mask; ++n, h = (h + 1u) & mask) {
        const uint32_t k = tab[h];
        if (k == PIBT_EMPTY) return PIBT_NOBODY;
        if ((k >> 10) == key) return k & 0x3FFu;
    }
    return PIBT_NOBODY;
}

// ---- what the walks of one lane see: its env's map, fields, targets and table ----------------------------------------
template <typename F>
struct SwapView {
    const uint32_t* bm;      // the env's padded obstacle bitmap
    const F* field;          // the env's distance fields: agent k's starts at k * cells
    const uint32_t* tgt;     // LDS: the env's packed padded targets
    const uint32_t* tab;     // LDS: the env's table
    size_t cells;            // H * W
    int H, W, r, wpr, log2n;

    __device__ __forceinline__ bool open(uint32_t c) const {   // in the map and no obstacle
        const int vx = (int)(c >> 16), vy = (int)(c & 0xFFFFu);
        const int ux = vx - r, uy = vy - r;
        if (!(ux >= 0 && ux < H && uy >= 0 && uy < W)) return false;
        return !((bm[(size_t)vx * wpr + (vy >> 5)] >> (vy & 31)) & 1u);
    }
    __device__ __forceinline__ uint32_t dist(int agent, uint32_t c) const {   // D_agent(c) of an open cell
        const int ux = (int)(c >> 16) - r, uy = (int)(c & 0xFFFFu) - r;
        const F d = field[(size_t)agent * cells + (size_t)ux * W + uy];
        return d == (F)~F(0) ? PIBT_INF : (uint32_t)d;
    }
    __device__ __forceinline__ uint32_t step(uint32_t c, int a) const {
        return (uint32_t)((int)c + pibt_dx(a) * 65536 + pibt_dy(a));
    }
    __device__ __forceinline__ bool parked(uint32_t u) const {  // an agent at home in a dead end
        const uint32_t k = swap_now(tab, log2n, u);
        if (k == PIBT_NOBODY || tgt[k] != u) return false;
        int n = 0;
        for (int a = 1; a < 5; ++a) n += open(step(u, a)) ? 1 : 0;
        return n == 1;
    }
    __device__ __forceinline__ int ahead(uint32_t v_pusher, uint32_t v_puller, uint32_t& tmp) const {
        bool ok[5];
#pragma unroll
        for (int a = 1; a < 5; ++a) {         // the four bitmap loads first: they do not depend on one another
            const uint32_t u = step(v_puller, a);
            ok[a] = u != v_pusher && open(u);
        }
        int n = 0;
#pragma unroll
        for (int a = 1; a < 5; ++a) {
            const uint32_t u = step(v_puller, a);
            if (ok[a] && !parked(u)) {
                ++n;
                tmp = u;
            }
        }
        return n;
    }
    __device__ __forceinline__ bool required(int pusher, int puller, uint32_t v_pusher, uint32_t v_puller) const {
        bool judge = false;
        for (int it = 0; it <= SWAP_MAX_WALK; ++it) {
            if (!(dist(pusher, v_puller) < dist(pusher, v_pusher))) {
                judge = true;
                break;
            }
            if (it == SWAP_MAX_WALK) return false;
            uint32_t tmp = v_puller;
            const int n = ahead(v_pusher, v_puller, tmp);
            if (n >= 2) return false;
            if (n == 0) {
                judge = true;
                break;
            }
            v_pusher = v_puller;
            v_puller = tmp;
        }
        if (!judge) return false;
        const uint32_t dp = dist(pusher, v_pusher);
        return dist(puller, v_pusher) < dist(puller, v_puller) && (dp == 0u || dist(pusher, v_puller) < dp);
    }
    __device__ __forceinline__ bool possible(uint32_t v_pusher0, uint32_t v_puller0) const {
        uint32_t v_pusher = v_pusher0, v_puller = v_puller0;
        for (int it = 0; it <= SWAP_MAX_WALK; ++it) {
            if (v_puller == v_pusher0) return false;
            if (it == SWAP_MAX_WALK) return false;
            uint32_t tmp = v_puller;
            const int n = ahead(v_pusher, v_puller, tmp);
            if (n >= 2) return true;
            if (n == 0) return false;
            v_pusher = v_puller;
            v_puller = tmp;
        }
        return false;
    }
};

// ---- phase 2 ------------------------------------------------------------------------------------------------------------
struct SwapLds {
    const uint32_t* sw;          // [T] phase 1: usual | clear << 16, SWAP_NONE where there is none
    const uint8_t* len;          // [T] phase 1: candidates in the agent's list
    uint16_t* swc;               // [T] phase 2: the partner the agent's call chose, SWAP_NONE: the list is walked forwards
};
// pibt_serial (pgx_pibt_plan.h) with S23's additions.  The loop runs at most 7 A + 2 times: every planned agent is
// started from the order at most once (A + 1 iterations with the one that ends the loop), is called at most once, and
// a call takes one iteration per candidate (at most 5) and one when the list is exhausted.
__device__ __forceinline__ void pibt_swap_serial(const PibtLds& s, const SwapLds& x, int nenv, int A, int log2n) {
    const int t = threadIdx.x;
    if (t < nenv) {
        const int b = t * A;
        const int n = (int)s.n[t];
        uint32_t* set = s.set + ((size_t)t << log2n);
        const uint32_t mask = (1u << log2n) - 1u;
        const auto reserved = [&](uint32_t cell) {
            uint32_t h = (cell * 0x9E3779B1u) >> (32 - log2n);
            for (uint32_t q = 0; q <= mask; ++q, h = (h + 1u) & mask) {
                const uint32_t k = set[h];
                if (k == cell) return true;
                if (k == PIBT_EMPTY) return false;
            }
            return false;
        };
        const auto reserve = [&](uint32_t cell) {
            uint32_t h = (cell * 0x9E3779B1u) >> (32 - log2n);
            for (uint32_t q = 0; q <= mask; ++q, h = (h + 1u) & mask) {
                const uint32_t k = set[h];
                if (k == cell) return;
                if (k == PIBT_EMPTY) {
                    set[h] = cell;
                    return;
                }
            }
        };
        bool pulls = false;                   // a call of the running chain chose a partner: its success may pull
        const auto begin = [&](int c, uint16_t caller) {   // the head of PIBT(c, caller): sw is chosen once per call
            const uint32_t pair = x.sw[b + c];
            const uint32_t usual = pair & 0xFFFFu, clear = pair >> 16;
            const uint32_t sw = (usual != SWAP_NONE && s.act[b + usual] == PIBT_UNSET) ? usual : clear;
            s.par[b + c] = caller;
            s.ci[b + c] = 0;
            x.swc[b + c] = (uint16_t)sw;
            pulls = (caller != PIBT_NONE && pulls) || sw != SWAP_NONE;
        };
        int k = 0, cur = -1;
        for (int it = 0; it < 7 * A + 2; ++it) {
            if (cur < 0) {
                if (k >= n) break;
                const int c = s.order[b + k++];
                if (s.act[b + c] != PIBT_UNSET) continue;
                cur = c;
                begin(c, PIBT_NONE);
                continue;
            }
            const int ci = s.ci[b + cur], len = x.len[b + cur];
            const uint32_t here = s.pos[b + cur];
            const uint16_t par = s.par[b + cur];
            if (ci >= len) {                  // every candidate refused: stay, and hold the own cell
                s.act[b + cur] = 0;
                reserve(here);
                cur = par == PIBT_NONE ? -1 : (int)par;
                continue;
            }
            const uint16_t e = s.cand[5 * (b + cur) + (x.swc[b + cur] != SWAP_NONE ? len - 1 - ci : ci)];
            s.ci[b + cur] = (uint8_t)(ci + 1);
            const int a = e & 7;
            const uint32_t v = (uint32_t)((int)here + pibt_dx(a) * 65536 + pibt_dy(a));
            if (reserved(v)) continue;
            if (par != PIBT_NONE && v == s.pos[b + par]) continue;
            s.act[b + cur] = (uint8_t)a;
            reserve(v);
            const int j = e >> 4;
            if ((e & 8) && s.act[b + j] == PIBT_UNSET) {  // the cell's agent has to move on first
                begin(j, (uint16_t)cur);
                cur = j;
                continue;
            }
            // success: cur and every caller up the chain return True, innermost first; a call whose first-tried
            // candidate held pulls its partner into the cell it leaves
            for (int d = 0, c = cur; pulls && d < A; ++d) {
                const uint32_t sw = x.swc[b + c], from = s.pos[b + c];
                if (s.ci[b + c] == 1 && sw != SWAP_NONE && s.act[b + sw] == PIBT_UNSET && !reserved(from)) {
                    const int step = (int)from - (int)s.pos[b + sw];
                    s.act[b + sw] = (uint8_t)(step == -65536 ? 1 : step == 65536 ? 2 : step == -1 ? 3 : 4);
                    reserve(from);
                }
                const uint16_t up = s.par[b + c];
                if (up == PIBT_NONE) break;
                c = up;
            }
            cur = -1;
        }
    }
}

}  // namespace
}  // namespace pgx
