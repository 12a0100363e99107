// pgx_global_state.hip -- whole-map planes for centralised critics (pgx_global_state, docs/SPEC.md S20).
//
// For every environment, the picture of the whole map a critic, a mixer or a central planner reads: [B][C][H][W] in the
// caller's channel order and number format, row x, column y, unpadded.  One launch writes it and nothing else.
//
// A workgroup owns one (env, band of whole rows) at a time: R = GLOBAL_BAND_CELLS / W rows, the last band of an env
// what is left (a grid-stride loop over the bands).  Per band:
//   1. every lane builds 32-bit words of the band's LDS picture, one byte per cell: bit 0 of a byte is the cell's bit of
//      the padded obstacle bitmap (row and column offset by r, so a map row starts in the middle of a bitmap word), the
//      other bits are 0 -- this pass is the clear as well.  The instances that serve an id channel also fill two 16-bit
//      ids per cell with all ones;
//   2. lanes stride over the env's agents: an agent whose `active` byte is exactly ACTIVE_BIT sets bit 1 of its cell's
//      byte if its row lies in the band (hidden agents and Q2's ghosts are not in the occupancy array), an agent with
//      ACTIVE_BIT set (a ghost too) sets bit 2 of its target's byte.  Bytes of different cells share a word, so a bit is
//      set with an atomic OR on the word.  The id planes keep the minimum of `index + 1` per cell: an atomic
//      compare-and-swap on the word that holds the cell's 16 bits;
//   3. the band's rows of one plane are contiguous in `out` (rows * W elements): the whole workgroup writes them as one
//      flat stream of 16-byte stores, element e = bit code[c] of cell e's byte (or its id, all ones -> 0) in the output
//      format.  Offsets are 64-bit: B * C * H * W elements pass 2^32 bytes.  Where a plane's band does not start on a
//      16-byte boundary (odd H * W with a narrow format, a misaligned `out`), the elements before the first boundary and
//      after the last one go out in stores of the element size.
// A band reads the env's pos / tgt / active again (9 bytes per agent).  The engine state the next pgx_step reads is only read.
#include <hip/hip_fp16.h>

#include <algorithm>

#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr int GS_THREADS = 256;
constexpr size_t GS_MAX_GRID = 2048;       // workgroups: 8 per CU; more bands than that take the grid-stride loop
constexpr int GS_CELLS = GLOBAL_BAND_CELLS;
constexpr uint32_t GS_NO_ID = 0xFFFFu;

// min(ids[idx], v) on a 16-bit entry of an LDS array of words
__device__ __forceinline__ void gs_min16(uint32_t* ids, uint32_t idx, uint32_t v) {
    uint32_t* w = ids + (idx >> 1);
    const uint32_t sh = 16u * (idx & 1u);
    uint32_t old = *w;
    while (((old >> sh) & 0xFFFFu) > v) {
        const uint32_t seen = atomicCAS(w, old, (old & ~(0xFFFFu << sh)) | (v << sh));
        if (seen == old) break;
        old = seen;
    }
}

// ELEM: bytes per output element; IDS: an id channel is served
template <int ELEM, bool IDS>
__global__ void __launch_bounds__(GS_THREADS) global_state_kernel(GlobalStateParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t s_word[GS_CELLS / 4];     // one byte per cell of the band
    __shared__ __attribute__((aligned(16))) uint32_t s_ids[IDS ? GS_CELLS : 1];  // 16 bits per cell: agent ids, then target ids
    const uint8_t* s_cell = reinterpret_cast<const uint8_t*>(s_word);
    [[maybe_unused]] const uint16_t* s_id16 = reinterpret_cast<const uint16_t*>(s_ids);
    const int tid = threadIdx.x;
    const int A = p.A, C = p.num_channels, H = p.H, W = p.W, r = p.r;
    const int R = GS_CELLS / W;              // rows per band (W <= GS_CELLS: launch_global_state)
    const int nb = (H + R - 1) / R;          // bands per env
    const size_t bands = (size_t)p.batch * nb;
    const size_t plane = (size_t)H * W;
    const uint32_t need = p.need, codes = p.codes, one = p.one;
    constexpr uint32_t PER = 16 / ELEM;      // elements per 16-byte store
    // the integer v (0, 1 or an id the format holds exactly) as an output element
    auto enc = [&](uint32_t v) -> uint32_t {
        if constexpr (ELEM == 4) return __float_as_uint((float)v);
        else if constexpr (ELEM == 1) return v;
        else return p.dtype == POLICY_INPUT_BF16 ? __float_as_uint((float)v) >> 16
                                                 : (uint32_t)__half_as_ushort(__float2half_rn((float)v));
    };

    for (size_t band = blockIdx.x; band < bands; band += gridDim.x) {
        const size_t env = band / nb;
        const int row0 = (int)(band - env * nb) * R;
        const int rows = min(R, H - row0);
        const int n = rows * W;              // cells of the band, <= GS_CELLS
        __syncthreads();                     // the previous band's stream has read its picture

        // 1. the obstacle bits, four cells (one word) per lane and round; every other bit of the word is cleared
        const uint32_t* bm = p.obst + env * p.bmw;
        for (int q = tid; q < (n + 3) / 4; q += GS_THREADS) {
            uint32_t w = 0;
            if (need & 1u) {
                const int c0 = 4 * q;
                int row = c0 / W, col = c0 - row * W;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (c0 + k < n) {
                        const int px = row0 + row + r, py = col + r;
                        w |= ((bm[px * p.wpr + (py >> 5)] >> (py & 31)) & 1u) << (8 * k);
                    }
                    if (++col == W) col = 0, ++row;
                }
            }
            s_word[q] = w;
        }
        if constexpr (IDS) {
            for (int q = tid; q < (n + 1) / 2; q += GS_THREADS) s_ids[q] = s_ids[GS_CELLS / 2 + q] = 0xFFFFFFFFu;
        }
        __syncthreads();                     // every byte is initialised before the first bit is set

        // 2. where the env's agents stand and where they are going
        if (need & 0x1Eu) {
            const size_t e0 = env * A;
            for (int j = tid; j < A; j += GS_THREADS) {
                const uint32_t aj = p.active[e0 + j];
                if (!(aj & ACTIVE_BIT)) continue;
                if (aj == ACTIVE_BIT && (need & 0x0Au)) {
                    const uint32_t pj = p.pos[e0 + j];
                    const int x = (int)(pj >> 16) - r - row0, y = (int)(pj & 0xFFFFu) - r;
                    if ((unsigned)x < (unsigned)rows && (unsigned)y < (unsigned)W) {
                        const uint32_t cell = (uint32_t)(x * W + y);
                        atomicOr(&s_word[cell >> 2], 2u << (8 * (cell & 3u)));
                        if constexpr (IDS) gs_min16(s_ids, cell, (uint32_t)j + 1u);
                    }
                }
                if (need & 0x14u) {
                    const uint32_t tj = p.tgt[e0 + j];
                    const int x = (int)(tj >> 16) - r - row0, y = (int)(tj & 0xFFFFu) - r;
                    if ((unsigned)x < (unsigned)rows && (unsigned)y < (unsigned)W) {
                        const uint32_t cell = (uint32_t)(x * W + y);
                        atomicOr(&s_word[cell >> 2], 4u << (8 * (cell & 3u)));
                        if constexpr (IDS) gs_min16(s_ids, (uint32_t)GS_CELLS + cell, (uint32_t)j + 1u);
                    }
                }
            }
            __syncthreads();                 // the picture is complete
        }

        // 3. the band's rows of every chosen plane: nbytes bytes from `dst`
        const uint32_t nbytes = (uint32_t)n * ELEM;
        for (int c = 0; c < C; ++c) {
            const uint32_t code = (codes >> (4 * c)) & 7u;
            uint8_t* dst = static_cast<uint8_t*>(p.planes) + ((env * C + c) * plane + (size_t)row0 * W) * ELEM;
            // element e of the band in the output format
            auto value = [&](uint32_t e) -> uint32_t {
                if constexpr (IDS) {
                    if (code >= 3u) {
                        const uint32_t id = s_id16[(code == 3u ? 0u : (uint32_t)GS_CELLS) + e];
                        return id == GS_NO_ID ? 0u : enc(id);
                    }
                }
                return (s_cell[e] >> code) & 1u ? one : 0u;
            };
            auto store_one = [&](uint32_t e) {
                const uint32_t v = value(e);
                if constexpr (ELEM == 4) reinterpret_cast<uint32_t*>(dst)[e] = v;
                else if constexpr (ELEM == 2) reinterpret_cast<uint16_t*>(dst)[e] = (uint16_t)v;
                else dst[e] = (uint8_t)v;
            };
            // `dst` is aligned to the element size, so the bytes before the first 16-byte boundary are whole elements
            const uint32_t head = min(nbytes, (uint32_t)(-reinterpret_cast<uintptr_t>(dst) & 15u));
            const uint32_t hd = head / ELEM;                 // elements before the first boundary
            const uint32_t chunks = (nbytes - head) / 16;    // whole 16-byte pieces
            const uint32_t tail0 = hd + chunks * PER;        // first element behind them
            if ((uint32_t)tid < hd) store_one((uint32_t)tid);
            if (tail0 + (uint32_t)tid < (uint32_t)n) store_one(tail0 + (uint32_t)tid);   // fewer than PER <= 16 of them
            uint4* dst4 = reinterpret_cast<uint4*>(dst + head);
            for (uint32_t q = tid; q < chunks; q += GS_THREADS) {
                const uint32_t e0 = hd + q * PER;
                uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (uint32_t e = 0; e < PER; ++e) wd[(e * ELEM) >> 2] |= value(e0 + e) << (8 * ((e * ELEM) & 3u));
                dst4[q] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            }
        }
    }
}

template <int ELEM>
hipError_t gs_launch(const GlobalStateParams& p, dim3 grid, hipStream_t stream) {
    if (p.need & 0x18u) hipLaunchKernelGGL((global_state_kernel<ELEM, true>), grid, dim3(GS_THREADS), 0, stream, p);
    else hipLaunchKernelGGL((global_state_kernel<ELEM, false>), grid, dim3(GS_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_global_state(const GlobalStateParams& p, hipStream_t stream) {
    if (p.W < 1 || p.W > GS_CELLS || p.H < 1 || p.batch < 1) return hipErrorInvalidValue;  // a band is at least one whole row
    const int R = GS_CELLS / p.W;
    const size_t bands = (size_t)p.batch * ((p.H + R - 1) / R);
    const dim3 grid((unsigned)std::min(bands, GS_MAX_GRID));
    if (p.dtype == POLICY_INPUT_F32) return gs_launch<4>(p, grid, stream);
    if (p.dtype == POLICY_INPUT_U8) return gs_launch<1>(p, grid, stream);
    return gs_launch<2>(p, grid, stream);
}

}  // namespace pgx
