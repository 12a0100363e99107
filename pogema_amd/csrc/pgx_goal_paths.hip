// pgx_goal_paths.hip -- path-to-goal planes and sub-goals (pgx_goal_paths, docs/SPEC.md S22).
//
// For every active agent: the greedy descent of its distance field from its own cell -- at every cell the lowest of the
// moves 1..4 whose destination is defined and strictly closer to the target -- marked in its (2r+1)^2 window until the
// target, the window's edge or the caller's cap ends it; the last marked cell is the agent's sub-goal.  The distances
// are pgx_cost2go.hip's cached fields: the call refreshes the stale ones (launch_cost_to_go_refresh) and then makes one
// launch of the kernel below.
//
// A workgroup owns ranges of PATH_SLOTS = 256 consecutive (env, agent) slots (a grid-stride loop over the ranges).  Per
// range:
//   1. every lane takes one slot and walks its path in the field itself: per step the four neighbours' cells, each read
//      only when it lies inside the H x W map (a cell outside counts as undefined, like an obstacle or an unreachable
//      cell: all ones in the field, never the smaller one); the cell moved to is the next step's centre and is not read
//      again.  The loop's condition is `n < cap` with cap <= W^2 - 1 fixed by the host, and the walk only ever moves to
//      a cell it has just read inside the map and inside the window: whatever a field holds, the loop ends and no
//      address leaves the field.  An agent that is not active reads nothing.  The lane marks its cells in its own W row
//      masks in LDS (nobody else touches them) and stores its sub-goal and length: neighbouring lanes, neighbouring
//      addresses;
//   2. the whole workgroup writes the range's planes as one flat stream of 16-byte stores, expanded from the row masks
//      (element e of the range is bit e % W of row word e / W, the slots' rows lying back to back).  256 slots are a
//      multiple of 16, so every range starts on a 16-byte boundary of an aligned `planes` in every format; the last
//      bytes of the last range and every byte of a misaligned `planes` go out in stores of the element size.  Without
//      `planes` the row masks, the stream and the barriers are left out.
// Why not pgx_directions.hip's shape (a wave per slot: the (2r+3)^2 halo tile into LDS, then a wave-uniform walk over
// it), which was built and measured first: the walk is a serial chain of a dozen instructions and one LDS round trip
// per step, and a wave that issues it for one agent wastes 63 of its 64 lanes on every one of them -- on 8192 envs x 64
// agents at r = 5 it took 750 us where goal_directions("bits") takes 305 us with the same tile reads, 430 us of it in the
// walk (docs/EXPERIMENTS.md).  A path of n cells needs at most 4 n + 1 cells of the field, not (2r+3)^2, and a lane per
// agent turns the serial chain into 64 independent ones per wave; the loads of a step are dependent on the step before,
// which thousands of resident waves hide.
// The engine state the next pgx_step reads is only read.
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr int PATH_SLOTS = 256;             // slots per range = lanes per workgroup; a multiple of 16 (see above)
constexpr size_t PATH_MAX_GRID = 2048;      // workgroups: 8 per CU; more ranges than that take the grid-stride loop

// the range's row words, then a chunk of overrun and a row: the last chunk of a tail expands up to 15 elements past
// its end, and the expansion fetches the row word after the one it ends in
__host__ __device__ size_t path_lds_bytes(int r) { return ((size_t)PATH_SLOTS * (2 * r + 1) + 8 + 2 * r + 1) * sizeof(uint32_t); }

// T: the field's cell type; FMT: PATHS_*
template <typename T, int FMT>
__global__ void __launch_bounds__(PATH_SLOTS) goal_paths_kernel(GoalPathParams p, int vec) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_rows[];  // [PATH_SLOTS][ws] one word per window row, the range's slots back to back
    const int r = p.r, ws = 2 * r + 1, H = p.H, W = p.W;
    const int tid = threadIdx.x;
    const size_t HW = (size_t)H * W;
    const size_t total = (size_t)p.batch * p.A;
    const size_t ranges = (total + PATH_SLOTS - 1) / PATH_SLOTS;
    const T* field = static_cast<const T*>(p.field);
    const bool planes = p.planes != nullptr;
    constexpr uint32_t UNDEF = (uint32_t)(T)~T(0);                              // the field's "no distance"
    constexpr uint32_t ELEM = FMT == PATHS_U8 ? 1 : 4;                          // bytes per output element
    const uint32_t bps = (FMT == PATHS_ROWS ? (uint32_t)ws : (uint32_t)(ws * ws)) * ELEM;  // plane bytes per slot
    uint32_t* rows = s_rows + tid * ws;      // this lane's row masks (ws is odd: the lanes' words fall on different banks)

    for (size_t range = blockIdx.x; range < ranges; range += gridDim.x) {
        const size_t s0 = range * PATH_SLOTS;
        const int ns = (int)min((size_t)PATH_SLOTS, total - s0);
        if (tid < ns) {
            const size_t slot = s0 + tid;
            if (planes)
                for (int u = 0; u < ws; ++u) rows[u] = 0u;
            int u = r, v = r, n = 0;          // the walk's cell in window coordinates
            if (p.active[slot] & ACTIVE_BIT) {
                const uint32_t pp = p.pos[slot];
                int x = (int)(pp >> 16) - r, y = (int)(pp & 0xFFFFu) - r;   // padded position - r = the cell (unpadded)
                const T* f = field + slot * HW + (size_t)x * W + y;           // the walk's cell in the field
                uint32_t c = *f;
                while (n < p.cap && c != UNDEF) {  // bounded by the host's cap, whatever the field holds
                    // (an undefined neighbour is all ones: never the smaller one; the target's 0 has nothing below it)
                    const uint32_t d0 = x > 0 ? (uint32_t)f[-W] : UNDEF, d1 = x + 1 < H ? (uint32_t)f[W] : UNDEF;
                    const uint32_t d2 = y > 0 ? (uint32_t)f[-1] : UNDEF, d3 = y + 1 < W ? (uint32_t)f[1] : UNDEF;
                    int du, dv;
                    uint32_t d;
                    if (d0 < c) du = -1, dv = 0, d = d0;
                    else if (d1 < c) du = 1, dv = 0, d = d1;
                    else if (d2 < c) du = 0, dv = -1, d = d2;
                    else if (d3 < c) du = 0, dv = 1, d = d3;
                    else break;                        // the target, or no way down
                    const int nu = u + du, nv = v + dv;
                    if (nu < 0 || nu >= ws || nv < 0 || nv >= ws) break;  // the next cell is outside the window
                    u = nu, v = nv, x += du, y += dv, ++n;
                    f += du * W + dv;
                    c = d;
                    if (planes) rows[u] |= 1u << v;
                }
            }
            if (p.subgoal) {
                p.subgoal[2 * slot] = (int8_t)(u - r);
                p.subgoal[2 * slot + 1] = (int8_t)(v - r);
            }
            if (p.length) p.length[slot] = n;
        }
        if (!planes) continue;               // (uniform: the barriers stay matched)
        __syncthreads();                     // the range's row masks are complete

        // the range's planes: nb bytes from `dst`, chunk c = bytes [16 c, 16 c + 16)
        const uint32_t nb = (uint32_t)ns * bps;
        uint8_t* dst = static_cast<uint8_t*>(p.planes) + s0 * bps;
        for (uint32_t c = tid; c < (nb + 15) / 16; c += PATH_SLOTS) {
            uint32_t wd[4];
            if constexpr (FMT == PATHS_ROWS) {
                const uint4 q = *reinterpret_cast<const uint4*>(s_rows + 4 * c);
                wd[0] = q.x, wd[1] = q.y, wd[2] = q.z, wd[3] = q.w;
            } else {
                // element e of the range = bit e % ws of row word e / ws
                constexpr uint32_t PER = 16 / ELEM;
                const uint32_t e0 = c * PER;
                uint32_t ri = e0 / ws, bit = e0 - ri * ws;
                uint32_t word = s_rows[ri];
                wd[0] = wd[1] = wd[2] = wd[3] = 0u;
#pragma unroll
                for (uint32_t e = 0; e < PER; ++e) {
                    const uint32_t b = (word >> bit) & 1u;
                    if constexpr (FMT == PATHS_F32) wd[e] = b ? 0x3F800000u : 0u;
                    else wd[e >> 2] |= b << (8 * (e & 3u));
                    if (++bit == (uint32_t)ws) {       // the next row: of the same slot or the first of the next one
                        bit = 0;
                        word = s_rows[++ri];
                    }
                }
            }
            if (vec && 16 * c + 16 <= nb) {
                *reinterpret_cast<uint4*>(dst + 16 * c) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            } else if constexpr (ELEM == 4) {
                for (uint32_t e = 0; e < 4 && 16 * c + 4 * e < nb; ++e) reinterpret_cast<uint32_t*>(dst + 16 * c)[e] = wd[e];
            } else {
                for (uint32_t e = 0; e < 16 && 16 * c + e < nb; ++e) dst[16 * c + e] = (uint8_t)(wd[e >> 2] >> (8 * (e & 3u)));
            }
        }
        __syncthreads();                     // the row masks are free for the next range
    }
}

template <typename T>
hipError_t path_launch(const GoalPathParams& p, hipStream_t stream) {
    const size_t total = (size_t)p.batch * p.A;
    const size_t ranges = (total + PATH_SLOTS - 1) / PATH_SLOTS;
    const unsigned grid = (unsigned)std::min(ranges, PATH_MAX_GRID);
    const size_t lds = p.planes ? path_lds_bytes(p.r) : 0;
    const int vec = (reinterpret_cast<uintptr_t>(p.planes) & 15) == 0 ? 1 : 0;
    const dim3 block(PATH_SLOTS);
    if (p.format == PATHS_F32)
        hipLaunchKernelGGL((goal_paths_kernel<T, PATHS_F32>), dim3(grid), block, lds, stream, p, vec);
    else if (p.format == PATHS_U8)
        hipLaunchKernelGGL((goal_paths_kernel<T, PATHS_U8>), dim3(grid), block, lds, stream, p, vec);
    else
        hipLaunchKernelGGL((goal_paths_kernel<T, PATHS_ROWS>), dim3(grid), block, lds, stream, p, vec);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_goal_paths(const GoalPathParams& p, hipStream_t stream) {
    const hipError_t err = launch_cost_to_go_refresh(p, stream);
    if (err != hipSuccess) return err;
    return p.cell_bytes == 4 ? path_launch<uint32_t>(p, stream) : path_launch<uint16_t>(p, stream);
}

}  // namespace pgx
