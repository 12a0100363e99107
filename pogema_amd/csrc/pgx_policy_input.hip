// pgx_policy_input.hip -- the network's input tensor (pgx_policy_input, docs/SPEC.md S18).
//
// For every agent, the window planes a learnt policy reads, in the order and the number format it reads them: the three
// observation planes of S4 (obstacles, agents, own target), the targets of the visible agents (other_goals) and the four
// direction-to-goal planes of S14.  One launch writes [B][A][C][W][W] and nothing else; with a direction plane among the
// channels the stale fields of pgx_cost2go.hip's cache are refreshed first (launch_cost_to_go_refresh).
//
// The structure is dir_gather_kernel's (pgx_directions.hip).  A workgroup owns ranges of `spr` consecutive (env, agent)
// slots (a grid-stride loop over the ranges).  Per range:
//   1. the workgroup clears one byte per window cell and slot in LDS;
//   2. each wave takes a slot at a time and sets the bits of its bytes -- bit k = the plane with channel code k:
//        bit 0      lanes stride over the window cells and read the padded obstacle bitmap (the ring is r wide, so the
//                   window never leaves it, and `empty_outside=False` is already packed into it);
//        bits 1, 3  lanes stride over the env's agents j: bit 1 at j's cell if j is in the window and its `active` byte
//                   is exactly ACTIVE_BIT (hidden agents and Q2's ghosts are not in the occupancy array); bit 3 at j's
//                   clamped target if observer and j are both active, j is another agent and stands in the window;
//        bit 2      the observer's own clamped target;
//        bits 4..7  pgx_directions.hip's comparison over the (2r+3)^2 halo tile of the agent's field, only in the
//                   instances that serve a direction channel (the others read no field and have no tile in LDS).
//      Slots of different waves share 32-bit LDS words (W^2 is odd), so every bit is set with an atomic OR on the word;
//   3. the whole workgroup writes the range's output as one flat stream of 16-byte stores: element (slot, c, cell) is bit
//      code[c] of the cell's byte, expanded to the output format.  `spr` is chosen so that every range starts on a
//      16-byte boundary of an aligned `out`; the last bytes of the last range and every byte of a misaligned `out` go
//      out in stores of the element size.
// The engine state the next pgx_step reads is only read.
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr int PIN_WAVES = 4;               // waves per workgroup = slots in flight
constexpr size_t PIN_MAX_GRID = 2048;      // workgroups: 8 per CU; more ranges than that take the grid-stride loop
constexpr uint32_t PIN_UNDEF = 0xFFFFFFFFu;
// MOVES[1..4] of docs/SPEC.md: up, down, left, right as (row, column) offsets
__device__ constexpr int PIN_DX[4] = {-1, 1, 0, 0};
__device__ constexpr int PIN_DY[4] = {0, 0, -1, 1};

// The fewest slots whose C * W^2 * elem output bytes are a multiple of 16 (W^2 is odd, so C * slots must be a multiple of
// 16 / elem), rounded up to the waves in flight; every term is a power of two.
int pin_slots_per_range(int C, int elem) {
    const int per = 16 / elem;
    const int low = C & -C;                 // the largest power of two that divides C
    return std::max(per / std::min(low, per), PIN_WAVES);
}
__host__ __device__ size_t pin_mask_bytes(int spr, int ww) { return ((size_t)spr * ww + 15) / 16 * 16 + 16; }  // + one chunk of overrun
size_t pin_lds_bytes(int spr, int r, bool dirs) {
    const int ws = 2 * r + 1, hs = ws + 2;
    return pin_mask_bytes(spr, ws * ws) + (dirs ? (size_t)PIN_WAVES * hs * hs * sizeof(uint32_t) : 0);
}

__device__ __forceinline__ int pin_clamp(int v, int r) { return max(-r, min(r, v)); }

// T: the field's cell type (not used without DIRS); ELEM: bytes per output element; DIRS: a direction channel is served
template <typename T, int ELEM, bool DIRS>
__global__ void __launch_bounds__(64 * PIN_WAVES) policy_input_kernel(PolicyInputParams p, int spr, int vec) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_pin[];
    const int r = p.r, ws = 2 * r + 1, ww = ws * ws, hs = ws + 2, hh = hs * hs;
    const uint8_t* s_mask = s_pin;           // [spr][ww] one byte per window cell, the range's slots back to back
    uint32_t* s_word = reinterpret_cast<uint32_t*>(s_pin);  // ... as the words the atomics work on
    const int mask_chunks = (int)(pin_mask_bytes(spr, ww) / 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] uint32_t* s_tile = reinterpret_cast<uint32_t*>(s_pin + pin_mask_bytes(spr, ww)) + wave * hh;  // the wave's halo tile
    const int A = p.A, C = p.num_channels;
    const int PH = p.H + 2 * r, PW = p.W + 2 * r;
    const size_t total = (size_t)p.batch * A;
    const size_t ranges = (total + spr - 1) / spr;
    const uint32_t need = p.need, codes = p.codes, one = p.one;
    constexpr uint32_t PER = 16 / ELEM;      // elements per 16-byte store
    const uint32_t bps = (uint32_t)C * ww * ELEM;  // output bytes per slot
    auto set_bits = [&](uint32_t byte, uint32_t bits) { atomicOr(&s_word[byte >> 2], bits << (8 * (byte & 3u))); };

    for (size_t range = blockIdx.x; range < ranges; range += gridDim.x) {
        const size_t s0 = range * spr;
        const int ns = (int)min((size_t)spr, total - s0);
        __syncthreads();                     // the previous range's stream has read its bytes
        for (int q = tid; q < mask_chunks; q += 64 * PIN_WAVES) reinterpret_cast<uint4*>(s_pin)[q] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();                     // every byte is clear before the first bit is set
        // rounds are uniform over the workgroup, so that the barriers of the halo tiles are reached by every wave
        for (int base = 0; base < spr; base += PIN_WAVES) {
            const int sl = base + wave;
            const bool have = sl < ns;
            const size_t slot = s0 + (have ? sl : 0);
            const uint32_t pp = p.pos[slot];
            const bool act = have && (p.active[slot] & ACTIVE_BIT);
            const int x = (int)(pp >> 16), y = (int)(pp & 0xFFFFu);  // padded
            if constexpr (DIRS) {
                if (act) {
                    // padded position - 2r - 1 = the halo tile's corner (unpadded)
                    const int x0 = x - 2 * r - 1, y0 = y - 2 * r - 1;
                    const T* f = static_cast<const T*>(p.field) + slot * ((size_t)p.H * p.W);
                    for (int j = lane; j < hh; j += 64) {
                        const int hu = j / hs, hv = j - hu * hs;
                        const int cx = x0 + hu, cy = y0 + hv;
                        uint32_t d = PIN_UNDEF;
                        if (cx >= 0 && cx < p.H && cy >= 0 && cy < p.W) {
                            const T c = f[(size_t)cx * p.W + cy];
                            if (c != (T)~T(0)) d = c;
                        }
                        s_tile[j] = d;
                    }
                }
                __syncthreads();             // the tiles are complete
            }
            if (have) {
                const uint32_t m0 = (uint32_t)sl * ww;  // the slot's first byte
                const size_t env = slot / A;
                const int i = (int)(slot - env * A);
                if (need & 0xF1u) {          // per window cell: the obstacle bit and the direction bits
                    const uint32_t* bm = p.obst + env * p.bmw;
                    for (int w = lane; w < ww; w += 64) {
                        const int u = w / ws, v = w - u * ws;
                        uint32_t bits = 0;
                        if (need & 1u) {
                            const int cx = x - r + u, cy = y - r + v;
                            if (cx >= 0 && cx < PH && cy >= 0 && cy < PW) bits = (bm[cx * p.wpr + (cy >> 5)] >> (cy & 31)) & 1u;
                        }
                        if constexpr (DIRS) {
                            if (act) {
                                const uint32_t* t = s_tile + (u + 1) * hs + (v + 1);
                                const uint32_t c = *t;
                                if (c != PIN_UNDEF) {
#pragma unroll
                                    for (int a = 0; a < 4; ++a) bits |= (t[PIN_DX[a] * hs + PIN_DY[a]] < c ? 16u : 0u) << a;
                                }
                            }
                        }
                        if (bits) set_bits(m0 + w, bits);
                    }
                }
                if (need & 0xAu) {           // per agent of the env: where it stands, where it is going
                    const size_t e0 = env * A;
                    for (int j = lane; j < A; j += 64) {
                        const uint32_t pj = p.pos[e0 + j], aj = p.active[e0 + j];
                        const int dx = (int)(pj >> 16) - x, dy = (int)(pj & 0xFFFFu) - y;
                        if (dx < -r || dx > r || dy < -r || dy > r) continue;
                        if ((need & 2u) && aj == ACTIVE_BIT) set_bits(m0 + (r + dx) * ws + (r + dy), 2u);
                        if ((need & 8u) && act && (aj & ACTIVE_BIT) && j != i) {
                            const uint32_t tj = p.tgt[e0 + j];
                            const int fu = r + pin_clamp((int)(tj >> 16) - x, r), fv = r + pin_clamp((int)(tj & 0xFFFFu) - y, r);
                            set_bits(m0 + fu * ws + fv, 8u);
                        }
                    }
                }
                if ((need & 4u) && lane == 0) {  // S4's get_square_target: per-axis clamp of the offset to the window edge
                    const uint32_t ti = p.tgt[slot];
                    const int fu = r + pin_clamp((int)(ti >> 16) - x, r), fv = r + pin_clamp((int)(ti & 0xFFFFu) - y, r);
                    set_bits(m0 + fu * ws + fv, 4u);
                }
            }
            if constexpr (DIRS) __syncthreads();  // the tiles are free again
        }
        __syncthreads();                     // the bytes are complete

        // the range's output: nb bytes from `dst`, chunk c = bytes [16 c, 16 c + 16)
        const uint32_t nb = (uint32_t)ns * bps;
        uint8_t* dst = static_cast<uint8_t*>(p.planes) + s0 * bps;
        for (uint32_t c = tid; c < (nb + 15) / 16; c += 64 * PIN_WAVES) {
            // element e of the range = (slot, channel, cell): the cell's byte of the slot, bit code[channel]
            const uint32_t e0 = c * PER;
            const uint32_t sp = e0 / ww, s = sp / C;
            uint32_t cell = e0 - sp * ww, ch = sp - s * C, mi = s * ww + cell, shift = (codes >> (4 * ch)) & 7u;
            uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t e = 0; e < PER; ++e) {
                const uint32_t bit = (s_mask[mi] >> shift) & 1u;
                wd[(e * ELEM) >> 2] |= (bit ? one : 0u) << (8 * ((e * ELEM) & 3u));
                ++mi;
                if (++cell == (uint32_t)ww) {  // the next channel of the same slot, or channel 0 of the next slot
                    cell = 0;
                    if (++ch == (uint32_t)C) ch = 0;
                    else mi -= ww;
                    shift = (codes >> (4 * ch)) & 7u;
                }
            }
            if (vec && 16 * c + 16 <= nb) {
                *reinterpret_cast<uint4*>(dst + 16 * c) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            } else if constexpr (ELEM == 4) {
                for (uint32_t e = 0; e < 4 && 16 * c + 4 * e < nb; ++e) reinterpret_cast<uint32_t*>(dst + 16 * c)[e] = wd[e];
            } else if constexpr (ELEM == 2) {
                for (uint32_t e = 0; e < 8 && 16 * c + 2 * e < nb; ++e)
                    reinterpret_cast<uint16_t*>(dst + 16 * c)[e] = (uint16_t)(wd[e >> 1] >> (16 * (e & 1u)));
            } else {
                for (uint32_t e = 0; e < 16 && 16 * c + e < nb; ++e) dst[16 * c + e] = (uint8_t)(wd[e >> 2] >> (8 * (e & 3u)));
            }
        }
    }
}

template <typename T, bool DIRS>
hipError_t pin_launch(const PolicyInputParams& p, hipStream_t stream) {
    const int elem = p.dtype == POLICY_INPUT_F32 ? 4 : p.dtype == POLICY_INPUT_U8 ? 1 : 2;
    const int spr = pin_slots_per_range(p.num_channels, elem);
    const size_t total = (size_t)p.batch * p.A;
    const size_t ranges = (total + spr - 1) / spr;
    const dim3 grid((unsigned)std::min(ranges, PIN_MAX_GRID)), block(64 * PIN_WAVES);
    const size_t lds = pin_lds_bytes(spr, p.r, DIRS);
    const int vec = (reinterpret_cast<uintptr_t>(p.planes) & 15) == 0 ? 1 : 0;
    if (elem == 4) hipLaunchKernelGGL((policy_input_kernel<T, 4, DIRS>), grid, block, lds, stream, p, spr, vec);
    else if (elem == 2) hipLaunchKernelGGL((policy_input_kernel<T, 2, DIRS>), grid, block, lds, stream, p, spr, vec);
    else hipLaunchKernelGGL((policy_input_kernel<T, 1, DIRS>), grid, block, lds, stream, p, spr, vec);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_policy_input(const PolicyInputParams& p, hipStream_t stream) {
    if (!(p.need & 0xF0u)) return pin_launch<uint16_t, false>(p, stream);  // no field is read: `p`'s cache fields are not used
    const hipError_t err = launch_cost_to_go_refresh(p, stream);
    if (err != hipSuccess) return err;
    return p.cell_bytes == 4 ? pin_launch<uint32_t, true>(p, stream) : pin_launch<uint16_t, true>(p, stream);
}

}  // namespace pgx
