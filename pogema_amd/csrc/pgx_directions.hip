// pgx_directions.hip -- direction-to-goal planes (pgx_goal_directions, docs/SPEC.md S14).
//
// For every active agent and every cell c of its (2r+1)^2 window: which of the moves 1..4 lead from c to a cell that is
// strictly closer to the agent's current target.  The distances are pgx_cost2go.hip's cached fields: the call refreshes
// the stale ones (launch_cost_to_go_refresh) and then makes one launch of the kernel below.
//
// A workgroup owns ranges of `spr` consecutive (env, agent) slots (a grid-stride loop over the ranges).  Per range:
//   1. each wave takes a slot at a time and reads the (2r+3)^2 halo tile of its field -- the window and one cell around
//      it -- row-major, neighbouring lanes neighbouring cells, into LDS; a cell outside the H x W map is never read and
//      counts as undefined, like an obstacle or an unreachable cell (all ones in the field);
//   2. the same wave derives one byte per window cell from the tile: bit a-1 set iff the cell's distance is defined and
//      the neighbour's under move a is smaller (an undefined distance is all ones, so it is never the smaller one; the
//      target's 0 has nothing below it).  An agent that is not active gets zeros and its field is not read;
//   3. the whole workgroup writes the range's output as one flat stream of 16-byte stores, the bytes of step 2 expanded
//      to the requested format.  `spr` is chosen so that every range starts on a 16-byte boundary of an aligned `out`
//      (W^2 is odd: 16 slots for one byte per cell, 4 slots for four); the last bytes of the last range and every byte of
//      a misaligned `out` go out in stores of the element size.
// The engine state the next pgx_step reads is only read.
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr int DIR_WAVES = 4;               // waves per workgroup = tiles in flight
constexpr size_t DIR_MAX_GRID = 2048;      // workgroups: 8 per CU; more ranges than that take the grid-stride loop
constexpr uint32_t DIR_UNDEF = 0xFFFFFFFFu;
// MOVES[1..4] of docs/SPEC.md: up, down, left, right as (row, column) offsets
__device__ constexpr int DIR_DX[4] = {-1, 1, 0, 0};
__device__ constexpr int DIR_DY[4] = {0, 0, -1, 1};

int dir_slots_per_range(int format) { return format == DIRECTIONS_BITS ? 16 : 4; }
__host__ __device__ size_t dir_mask_bytes(int spr, int ww) { return ((size_t)spr * ww + 15) / 16 * 16 + 16; }  // + one chunk of overrun
size_t dir_lds_bytes(int spr, int r) {
    const int ws = 2 * r + 1, hs = ws + 2;
    return dir_mask_bytes(spr, ws * ws) + (size_t)DIR_WAVES * hs * hs * sizeof(uint32_t);
}

// T: the field's cell type; FMT: DIRECTIONS_*
template <typename T, int FMT>
__global__ void __launch_bounds__(64 * DIR_WAVES) dir_gather_kernel(CostToGoParams p, void* out, int spr, int vec) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dir[];
    const int ws = 2 * p.r + 1, ww = ws * ws, hs = ws + 2, hh = hs * hs;
    uint8_t* s_mask = s_dir;                 // [spr][ww] one byte per window cell, the range's slots back to back
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* s_tile = reinterpret_cast<uint32_t*>(s_dir + dir_mask_bytes(spr, ww)) + wave * hh;  // the wave's halo tile
    const size_t HW = (size_t)p.H * p.W;
    const size_t total = (size_t)p.batch * p.A;
    const size_t ranges = (total + spr - 1) / spr;
    const T* field = static_cast<const T*>(p.field);
    constexpr uint32_t ELEM = FMT == DIRECTIONS_F32 ? 4 : 1;                   // bytes per output element
    constexpr uint32_t PER = 16 / ELEM;                                        // elements per 16-byte store
    const uint32_t bps = (uint32_t)ww * (FMT == DIRECTIONS_BITS ? 1u : 4u * ELEM);  // output bytes per slot

    for (size_t range = blockIdx.x; range < ranges; range += gridDim.x) {
        const size_t s0 = range * spr;
        const int ns = (int)min((size_t)spr, total - s0);
        // rounds are uniform over the workgroup, so that the barriers are reached by every wave.  A wave reads only the
        // tile it wrote itself, so wave-level ordering would do for the tiles; only the barrier before the output stream
        // (and, through it, the ordering against the next range's mask writes) needs the whole workgroup.  Workgroup
        // barriers are used throughout to keep one kind of synchronisation: two per round, next to hundreds of cycles
        // of field loads
        for (int base = 0; base < spr; base += DIR_WAVES) {
            const int sl = base + wave;
            const bool have = sl < ns;
            const size_t slot = s0 + (have ? sl : 0);
            const bool act = have && (p.active[slot] & ACTIVE_BIT);
            if (act) {
                const uint32_t pp = p.pos[slot];
                // padded position - 2r - 1 = the halo tile's corner (unpadded)
                const int x0 = (int)(pp >> 16) - 2 * p.r - 1, y0 = (int)(pp & 0xFFFFu) - 2 * p.r - 1;
                const T* f = field + slot * HW;
                for (int j = lane; j < hh; j += 64) {
                    const int hu = j / hs, hv = j - hu * hs;
                    const int cx = x0 + hu, cy = y0 + hv;
                    uint32_t d = DIR_UNDEF;
                    if (cx >= 0 && cx < p.H && cy >= 0 && cy < p.W) {
                        const T c = f[(size_t)cx * p.W + cy];
                        if (c != (T)~T(0)) d = c;
                    }
                    s_tile[j] = d;
                }
            }
            __syncthreads();                 // the tiles are complete
            if (have) {
                uint8_t* m = s_mask + sl * ww;
                for (int w = lane; w < ww; w += 64) {
                    uint32_t bits = 0;
                    if (act) {
                        const int u = w / ws, v = w - u * ws;
                        const uint32_t* t = s_tile + (u + 1) * hs + (v + 1);
                        const uint32_t c = *t;
                        if (c != DIR_UNDEF) {
#pragma unroll
                            for (int a = 0; a < 4; ++a) bits |= (t[DIR_DX[a] * hs + DIR_DY[a]] < c ? 1u : 0u) << a;
                        }
                    }
                    m[w] = (uint8_t)bits;
                }
            }
            __syncthreads();                 // the tiles are free again; after the last round: the masks are complete
        }

        // the range's output: nb bytes from `dst`, chunk c = bytes [16 c, 16 c + 16)
        const uint32_t nb = (uint32_t)ns * bps;
        uint8_t* dst = static_cast<uint8_t*>(out) + s0 * bps;
        for (uint32_t c = tid; c < (nb + 15) / 16; c += 64 * DIR_WAVES) {
            uint32_t wd[4];
            if constexpr (FMT == DIRECTIONS_BITS) {
                const uint4 q = *reinterpret_cast<const uint4*>(s_mask + 16 * c);
                wd[0] = q.x, wd[1] = q.y, wd[2] = q.z, wd[3] = q.w;
            } else {
                // element e of the range = (slot, plane, cell): the cell's byte of the slot, bit `plane`
                const uint32_t e0 = c * PER;
                const uint32_t sp = e0 / ww;
                uint32_t cell = e0 - sp * ww, plane = sp & 3u, mi = (sp >> 2) * ww + cell;
                wd[0] = wd[1] = wd[2] = wd[3] = 0u;
#pragma unroll
                for (uint32_t e = 0; e < PER; ++e) {
                    const uint32_t bit = (s_mask[mi] >> plane) & 1u;
                    if constexpr (FMT == DIRECTIONS_F32) wd[e] = bit ? 0x3F800000u : 0u;
                    else wd[e >> 2] |= bit << (8 * (e & 3u));
                    ++mi;
                    if (++cell == (uint32_t)ww) {  // the next plane of the same slot, or plane 0 of the next slot
                        cell = 0;
                        plane = (plane + 1) & 3u;
                        if (plane) mi -= ww;
                    }
                }
            }
            if (vec && 16 * c + 16 <= nb) {
                *reinterpret_cast<uint4*>(dst + 16 * c) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            } else if constexpr (FMT == DIRECTIONS_F32) {
                for (uint32_t e = 0; e < 4 && 16 * c + 4 * e < nb; ++e) reinterpret_cast<uint32_t*>(dst + 16 * c)[e] = wd[e];
            } else {
                for (uint32_t e = 0; e < 16 && 16 * c + e < nb; ++e) dst[16 * c + e] = (uint8_t)(wd[e >> 2] >> (8 * (e & 3u)));
            }
        }
        // no barrier here: the next range writes its first mask byte behind a barrier every thread reaches after this loop
    }
}

template <typename T>
hipError_t dir_launch(const CostToGoParams& p, void* out, int format, hipStream_t stream) {
    const int spr = dir_slots_per_range(format);
    const size_t total = (size_t)p.batch * p.A;
    const size_t ranges = (total + spr - 1) / spr;
    const unsigned grid = (unsigned)std::min(ranges, DIR_MAX_GRID);
    const size_t lds = dir_lds_bytes(spr, p.r);
    const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0 ? 1 : 0;
    const dim3 block(64 * DIR_WAVES);
    if (format == DIRECTIONS_F32)
        hipLaunchKernelGGL((dir_gather_kernel<T, DIRECTIONS_F32>), dim3(grid), block, lds, stream, p, out, spr, vec);
    else if (format == DIRECTIONS_U8)
        hipLaunchKernelGGL((dir_gather_kernel<T, DIRECTIONS_U8>), dim3(grid), block, lds, stream, p, out, spr, vec);
    else
        hipLaunchKernelGGL((dir_gather_kernel<T, DIRECTIONS_BITS>), dim3(grid), block, lds, stream, p, out, spr, vec);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_goal_directions(const CostToGoParams& p, void* out, int format, hipStream_t stream) {
    const hipError_t err = launch_cost_to_go_refresh(p, stream);
    if (err != hipSuccess) return err;
    return p.cell_bytes == 4 ? dir_launch<uint32_t>(p, out, format, stream) : dir_launch<uint16_t>(p, out, format, stream);
}

}  // namespace pgx
