// pgx_agent_forecasts.hip -- where the visible agents will be, K steps ahead (pgx_agent_forecasts, docs/SPEC.md S24).
//
// Every active agent's FORECAST is K steps of the greedy descent of its distance field from its own cell -- at every cell
// the lowest of the moves 1..4 whose destination is defined and strictly closer to the target, pgx_goal_paths.hip's rule
// with no window ending it; where nothing is closer (the target, an unreachable target) it waits.  The distances are
// pgx_cost2go.hip's cached fields: the call refreshes the stale ones (launch_cost_to_go_refresh) and then makes two
// launches.
//
// 1. forecast_walk_kernel.  A workgroup owns ranges of WALK_SLOTS = 256 consecutive (env, agent) slots (a grid-stride
//    loop over the ranges); every lane takes one slot and walks in the field itself: per step the four neighbours' cells,
//    each read only when it lies inside the H x W map (a cell outside counts as undefined: all ones, never the smaller
//    one); the cell moved to is the next step's centre and is not read again.  The trip count is K, fixed by the host,
//    and the walk only ever moves to a cell it has just read inside the map: whatever a field holds, the loop ends and no
//    address leaves the field.  The lane's K cells go straight to `cells`, 4 K contiguous bytes per slot, in 2-byte
//    stores (`cells` may sit at any 2-byte address).  A lane whose agent is not active writes -1s and reads no field.
//    Why a lane per agent and not a wave per agent: the walk is a serial chain -- the loads of a step depend on the
//    compare of the step before -- of four loads and a dozen instructions per step.  A wave that issues it for one agent
//    keeps 63 of its 64 lanes idle on every one of them and has nothing to do during the load's latency; a lane per
//    agent makes it 64 independent chains per wave, and the latency of a step is hidden by the thousands of waves that are
//    resident.  pgx_goal_paths.hip measured the two shapes for the same chain (757 us against 303 us on 8192 envs x 64
//    agents, docs/EXPERIMENTS.md).
// 2. forecast_gather_kernel (only with `planes`).  pgx_policy_input.hip's structure for other_goals.  A workgroup owns
//    ranges of `spr` consecutive slots (a grid-stride loop over the ranges).  Per range:
//      a. the workgroup clears the range's row words in LDS: K * W words per slot, word (s, u) of a slot = row u of its
//         plane s, the slots back to back;
//      b. each wave takes one observer at a time; its lanes stride over the env's agents j and read `pos` and `active`
//         and, for an active j != i inside the observer's window, j's K cells from `cells` (4 K bytes, written by the
//         first launch: they stay in L2).  For each forecast cell inside the window the lane sets its bit with an LDS
//         atomic OR (lanes of a wave meet on one word).  An inactive observer keeps its zeros;
//      c. the whole workgroup writes the range's planes as one flat stream of 16-byte stores, expanded from the row words
//         (element e of the range is bit e % W of row word e / W).  `spr` is a multiple of 16, so every range starts on a
//         16-byte boundary of an aligned `planes` in every format and for every K; the last bytes of the last range and
//         every byte of a misaligned `planes` go out in stores of the element size.
//    `spr` is FC_SLOTS = 64 unless the row words of 64 slots exceed FC_LDS_BUDGET: a slot takes 4 K W bytes, 992 at
//    r = 15, K = 8, where the range shrinks to 32 slots (forecast_slots_per_range, on the host).
// The engine state the next pgx_step reads is only read.
//
// The gather reads no field, so unlike the walk it is not templated on the field's cell type.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950, -O3): forecast_walk_kernel 18 VGPRs for 2- and for 4-byte
// fields; forecast_gather_kernel 29 (float32), 52 (uint8) and 24 (rows) VGPRs; no scratch in any instance, occupancy 8
// waves per SIMD in all of them.  Measured on 8192 envs x 64 agents, r = 5, K = 3 (docs/EXPERIMENTS.md): the walk 149 us,
// the gather 157 us with uint8 and 213 us with float32 planes, where a fill of the same bytes takes 28 and 106 us: the
// gather is bound by the dependent reads in front of its stream, not by the stream.
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr int WALK_SLOTS = 256;             // slots per range of the walk = lanes per workgroup
constexpr int FC_WAVES = 4;                 // waves per workgroup of the gather = observers in flight
constexpr int FC_SLOTS = 64;                // most slots per range of the gather; a multiple of 16 (see above)
constexpr size_t FC_LDS_BUDGET = 32768;     // bytes of row words per workgroup: five workgroups per CU
constexpr size_t FC_MAX_GRID = 2048;        // workgroups: 8 per CU; more ranges than that take the grid-stride loop

// the slots per range of the gather: FC_SLOTS, or the largest multiple of 16 whose row words fit the budget (never
// below 16: 16 slots of the largest K and W take 15872 bytes)
int forecast_slots_per_range(int K, int ws) {
    const int fit = (int)(FC_LDS_BUDGET / ((size_t)K * ws * sizeof(uint32_t))) / 16 * 16;
    return std::max(16, std::min(FC_SLOTS, fit));
}
// the range's row words, then a chunk of overrun and a row: the last chunk of a tail expands up to 15 elements past
// its end, and the expansion fetches the row word after the one it ends in
size_t forecast_lds_bytes(int spr, int K, int ws) { return ((size_t)spr * K * ws + 8 + ws) * sizeof(uint32_t); }

// T: the field's cell type
template <typename T>
__global__ void __launch_bounds__(WALK_SLOTS) forecast_walk_kernel(ForecastParams p) {
    const int r = p.r, H = p.H, W = p.W, K = p.steps;
    const size_t HW = (size_t)H * W;
    const size_t total = (size_t)p.batch * p.A;
    const size_t ranges = (total + WALK_SLOTS - 1) / WALK_SLOTS;
    const T* field = static_cast<const T*>(p.field);
    constexpr uint32_t UNDEF = (uint32_t)(T)~T(0);                              // the field's "no distance"

    for (size_t range = blockIdx.x; range < ranges; range += gridDim.x) {
        const size_t slot = range * WALK_SLOTS + threadIdx.x;
        if (slot >= total) continue;
        int16_t* out = p.cells + slot * (size_t)(2 * K);
        if (!(p.active[slot] & ACTIVE_BIT)) {
            for (int s = 0; s < 2 * K; ++s) out[s] = (int16_t)-1;
            continue;
        }
        const uint32_t pp = p.pos[slot];
        int x = (int)(pp >> 16) - r, y = (int)(pp & 0xFFFFu) - r;               // padded position - r = the cell (unpadded)
        const T* f = field + slot * HW + (size_t)x * W + y;                      // the walk's cell in the field
        uint32_t c = *f;
        bool moving = c != UNDEF;                 // (an unreachable agent waits where it is)
        for (int s = 0; s < K; ++s) {             // K trips, whatever the field holds
            if (moving) {
                // (an undefined neighbour is all ones: never the smaller one; the target's 0 has nothing below it)
                const uint32_t d0 = x > 0 ? (uint32_t)f[-W] : UNDEF, d1 = x + 1 < H ? (uint32_t)f[W] : UNDEF;
                const uint32_t d2 = y > 0 ? (uint32_t)f[-1] : UNDEF, d3 = y + 1 < W ? (uint32_t)f[1] : UNDEF;
                int dx = 0, dy = 0;
                if (d0 < c) dx = -1, c = d0;
                else if (d1 < c) dx = 1, c = d1;
                else if (d2 < c) dy = -1, c = d2;
                else if (d3 < c) dy = 1, c = d3;
                else moving = false;              // the target, or no way down: it waits here from now on
                x += dx, y += dy;
                f += dx * W + dy;
            }
            out[2 * s] = (int16_t)x;
            out[2 * s + 1] = (int16_t)y;
        }
    }
}

// FMT: FORECAST_*
template <int FMT>
__global__ void __launch_bounds__(64 * FC_WAVES) forecast_gather_kernel(ForecastParams p, int spr, int vec) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_rows[];  // [spr][K][ws] one word per plane row, the range's slots back to back
    const int r = p.r, ws = 2 * r + 1, K = p.steps, A = p.A;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t total = (size_t)p.batch * A;
    const size_t ranges = (total + spr - 1) / spr;
    const uint32_t wps = (uint32_t)(K * ws);                                     // row words per slot
    constexpr uint32_t ELEM = FMT == FORECAST_U8 ? 1 : 4;                        // bytes per output element
    const uint32_t bps = (FMT == FORECAST_ROWS ? wps : wps * (uint32_t)ws) * ELEM;  // plane bytes per slot

    for (size_t range = blockIdx.x; range < ranges; range += gridDim.x) {
        const size_t s0 = range * spr;
        const int ns = (int)min((size_t)spr, total - s0);
        __syncthreads();                     // the previous range's stream has read its words
        for (uint32_t q = tid; q < (uint32_t)ns * wps; q += 64 * FC_WAVES) s_rows[q] = 0u;
        __syncthreads();                     // every word is clear before the first bit is set
        for (int sl = wave; sl < ns; sl += FC_WAVES) {
            const size_t slot = s0 + sl;
            if (!(p.active[slot] & ACTIVE_BIT)) continue;    // (wave-uniform) an inactive observer gets zeros
            const uint32_t pp = p.pos[slot];
            const int px = (int)(pp >> 16), py = (int)(pp & 0xFFFFu);            // padded
            const size_t env = slot / A, e0 = env * A;
            const int i = (int)(slot - e0);
            uint32_t* rows = s_rows + (uint32_t)sl * wps;
            for (int j = lane; j < A; j += 64) {
                const uint32_t pj = p.pos[e0 + j], aj = p.active[e0 + j];
                const int dx = (int)(pj >> 16) - px, dy = (int)(pj & 0xFFFFu) - py;
                if (j == i || !(aj & ACTIVE_BIT) || dx < -r || dx > r || dy < -r || dy > r) continue;
                const int16_t* cj = p.cells + (e0 + j) * (size_t)(2 * K);
                for (int s = 0; s < K; ++s) {
                    // unpadded forecast cell - (padded observer - r) + r = the window cell
                    const int u = (int)cj[2 * s] - px + 2 * r, v = (int)cj[2 * s + 1] - py + 2 * r;
                    if (u >= 0 && u < ws && v >= 0 && v < ws) atomicOr(&rows[s * ws + u], 1u << v);
                }
            }
        }
        __syncthreads();                     // the range's row words are complete

        // the range's planes: nb bytes from `dst`, chunk c = bytes [16 c, 16 c + 16)
        const uint32_t nb = (uint32_t)ns * bps;
        uint8_t* dst = static_cast<uint8_t*>(p.planes) + s0 * bps;
        for (uint32_t c = tid; c < (nb + 15) / 16; c += 64 * FC_WAVES) {
            uint32_t wd[4];
            if constexpr (FMT == FORECAST_ROWS) {
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
                    if constexpr (FMT == FORECAST_F32) wd[e] = b ? 0x3F800000u : 0u;
                    else wd[e >> 2] |= b << (8 * (e & 3u));
                    if (++bit == (uint32_t)ws) {       // the next row: of the same plane, the next plane or the next slot
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
    }
}

template <typename T>
hipError_t forecast_walk_launch(const ForecastParams& p, hipStream_t stream) {
    const size_t total = (size_t)p.batch * p.A;
    const size_t ranges = (total + WALK_SLOTS - 1) / WALK_SLOTS;
    hipLaunchKernelGGL((forecast_walk_kernel<T>), dim3((unsigned)std::min(ranges, FC_MAX_GRID)), dim3(WALK_SLOTS), 0, stream, p);
    return hipGetLastError();
}

hipError_t forecast_gather_launch(const ForecastParams& p, hipStream_t stream) {
    const int ws = 2 * p.r + 1;
    const int spr = forecast_slots_per_range(p.steps, ws);
    const size_t total = (size_t)p.batch * p.A;
    const size_t ranges = (total + spr - 1) / spr;
    const dim3 grid((unsigned)std::min(ranges, FC_MAX_GRID)), block(64 * FC_WAVES);
    const size_t lds = forecast_lds_bytes(spr, p.steps, ws);
    const int vec = (reinterpret_cast<uintptr_t>(p.planes) & 15) == 0 ? 1 : 0;
    if (p.format == FORECAST_F32) hipLaunchKernelGGL((forecast_gather_kernel<FORECAST_F32>), grid, block, lds, stream, p, spr, vec);
    else if (p.format == FORECAST_U8) hipLaunchKernelGGL((forecast_gather_kernel<FORECAST_U8>), grid, block, lds, stream, p, spr, vec);
    else hipLaunchKernelGGL((forecast_gather_kernel<FORECAST_ROWS>), grid, block, lds, stream, p, spr, vec);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_agent_forecasts(const ForecastParams& p, hipStream_t stream) {
    hipError_t err = launch_cost_to_go_refresh(p, stream);
    if (err != hipSuccess) return err;
    err = p.cell_bytes == 4 ? forecast_walk_launch<uint32_t>(p, stream) : forecast_walk_launch<uint16_t>(p, stream);
    if (err != hipSuccess || !p.planes) return err;
    return forecast_gather_launch(p, stream);
}

}  // namespace pgx
