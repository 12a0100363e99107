// pgx_neighbours.hip -- neighbour lists (pgx_visible_agents, docs/SPEC.md S12).
//
// For every agent i: the other ACTIVE agents j of its env inside its square observation window (|dx| <= r and
// |dy| <= r, obstacles hide nobody), ordered by the key (dx^2 + dy^2, dx + r, dy + r, j), the first K of them, and their
// number.  Only `pos` and `active` are read; nothing is written but the caller's outputs.
//
// One lane per agent, 256 lanes per workgroup: floor(256 / A) whole envs per workgroup while A <= 256, ceil(A / 256)
// workgroups per env above.  The envs' words `pos | inactive -> far away` are staged in LDS once (at most 4 KB); every
// lane then sweeps the A agents of its env.  Lanes of one env read the same LDS address (a broadcast); the envs of a
// wave are an odd number of words apart, so that their reads fall into different banks.
//
// The whole key fits 29 bits of one word,
//     [28:20] dx^2 + dy^2 (<= 450 at r = 15)   [19:15] dx + r   [14:10] dy + r   [9:0] j
// and all ones is "empty".  A lane keeps its KT smallest keys in KT registers, sorted, and inserts a key with a fully
// unrolled min / max chain -- the list is never indexed at run time, so nothing goes to scratch.  The chain is skipped
// while no lane of the wave has a key below its largest kept one, and left early once every lane's carried key is empty.
// KT is 8, 16 or 32; the caller's K is rounded up to it and the tail is not written.
//
// Stores: the rows of a wave's lanes are contiguous in `index` and `offset`, so each wave transposes its keys through
// LDS (row stride KT + 1 words: odd, no bank conflict) and writes its range with consecutive lanes on consecutive
// elements, 256 B (index) or 128 B (offset) per store instruction, whatever K is.
#include "pgx_internal.h"

namespace pgx {
namespace {

constexpr int NB_THREADS = 256;               // lanes per workgroup
constexpr int NB_WAVES = NB_THREADS / 64;
constexpr int NB_MAX_AGENTS = 1024;           // PGX_MAX_AGENTS: the env stage of the layout above 256 agents
constexpr uint32_t NB_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t NB_FAR = 0x7FFF7FFFu;      // a staged word no window reaches: padded coordinates stay below 2048

template <int KT>
__global__ void __launch_bounds__(NB_THREADS) visible_agents_kernel(const NeighbourParams p) {
    constexpr int ROW = KT + 1;               // words between the staged rows of neighbouring lanes
    constexpr int STAGE = NB_WAVES * 64 * ROW;
    // the env stage of the sweep, then (after a barrier) the waves' key rows
    __shared__ uint32_t s_mem[STAGE > NB_MAX_AGENTS ? STAGE : NB_MAX_AGENTS];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int A = p.A, r = p.r, k = p.k;
    size_t row0;                              // row (= env * A + agent) of thread 0
    int rows;                                 // rows of this workgroup: threads [0, rows) own one each
    int i, base;                              // this thread's agent and the LDS word of agent 0 of its env
    if (A <= NB_THREADS) {
        const int epb = NB_THREADS / A;
        const int env0 = blockIdx.x * epb;
        const int nenv = min(epb, p.batch - env0);
        const int stride = A | 1;
        row0 = (size_t)env0 * A;
        rows = nenv * A;
        const int el = t / A;
        i = t - el * A;
        base = el * stride;
        if (t < rows) {
            const uint32_t w = p.pos[row0 + t];
            s_mem[base + i] = (p.active[row0 + t] & ACTIVE_BIT) ? w : NB_FAR;
        }
    } else {
        const int bpe = (A + NB_THREADS - 1) / NB_THREADS;
        const int env = blockIdx.x / bpe, chunk = blockIdx.x - env * bpe;
        const size_t e0 = (size_t)env * A;
        row0 = e0 + (size_t)chunk * NB_THREADS;
        rows = min(NB_THREADS, A - chunk * NB_THREADS);
        i = chunk * NB_THREADS + t;
        base = 0;
        for (int j = t; j < A; j += NB_THREADS) {
            const uint32_t w = p.pos[e0 + j];
            s_mem[j] = (p.active[e0 + j] & ACTIVE_BIT) ? w : NB_FAR;
        }
    }
    __syncthreads();

    const bool have = t < rows;
    // an inactive observer sees nobody: its own staged word is NB_FAR, out of every partner's reach
    const uint32_t self = have ? s_mem[base + i] : NB_FAR;
    const int xi = (int)(self >> 16), yi = (int)(self & 0xFFFFu);
    const uint32_t side = 2u * (uint32_t)r;

    uint32_t list[KT];
#pragma unroll
    for (int q = 0; q < KT; ++q) list[q] = NB_EMPTY;
    int count = 0;

    for (int j = 0; j < A; ++j) {
        const uint32_t w = s_mem[base + j];
        const int dx = (int)(w >> 16) - xi, dy = (int)(w & 0xFFFFu) - yi;
        const uint32_t u = (uint32_t)(dx + r), v = (uint32_t)(dy + r);
        const bool visible = u <= side && v <= side && j != i && self != NB_FAR;
        uint32_t key = ((uint32_t)(dx * dx + dy * dy) << 20) | (u << 15) | (v << 10) | (uint32_t)j;
        if (!visible) key = NB_EMPTY;
        count += visible ? 1 : 0;
        if (__ballot(key < list[KT - 1]) != 0ull) {
            // the carried key turns empty once it has dropped into an empty slot: when that holds in every lane the
            // rest of the chain changes nothing (checked every 4 slots; lists are mostly far shorter than KT)
#pragma unroll
            for (int q = 0; q < KT; ++q) {
                if (q != 0 && (q & 3) == 0 && __ballot(key != NB_EMPTY) == 0ull) break;
                const uint32_t lo = min(list[q], key);
                key = max(list[q], key);
                list[q] = lo;
            }
        }
    }
    if (have && p.count) p.count[row0 + t] = count;

    __syncthreads();                          // every sweep is done: the env stage becomes the key rows
    uint32_t* keys = s_mem + wave * 64 * ROW;
#pragma unroll
    for (int q = 0; q < KT; ++q) keys[lane * ROW + q] = list[q];
    __syncthreads();

    // the wave's rows [wave * 64, wave * 64 + nw) are one contiguous range of nw * k entries of each output
    const int nw = min(64, rows - wave * 64);
    if (nw <= 0) return;
    const int total = nw * k;
    const size_t out0 = (row0 + (size_t)wave * 64) * (size_t)k;
    const int step_row = 64 / k, step_col = 64 - step_row * k;
    int row = lane / k, col = lane - row * k;
    uint16_t* off16 = reinterpret_cast<uint16_t*>(p.offset);
    for (int f = lane; f < total; f += 64) {
        const uint32_t key = keys[row * ROW + col];
        const bool empty = key == NB_EMPTY;
        p.index[out0 + f] = empty ? -1 : (int32_t)(key & 1023u);
        if (off16) {
            const uint32_t dx = (((key >> 15) & 31u) - (uint32_t)r) & 0xFFu;
            const uint32_t dy = (((key >> 10) & 31u) - (uint32_t)r) & 0xFFu;
            off16[out0 + f] = empty ? (uint16_t)0 : (uint16_t)(dx | (dy << 8));
        }
        row += step_row;
        col += step_col;
        if (col >= k) {
            col -= k;
            ++row;
        }
    }
}

}  // namespace

hipError_t launch_visible_agents(const NeighbourParams& p, hipStream_t stream) {
    const int A = p.A;
    const unsigned grid = A <= NB_THREADS ? (unsigned)((p.batch + NB_THREADS / A - 1) / (NB_THREADS / A))
                                          : (unsigned)p.batch * (unsigned)((A + NB_THREADS - 1) / NB_THREADS);
    auto kernel = p.k <= 8 ? visible_agents_kernel<8> : p.k <= 16 ? visible_agents_kernel<16> : visible_agents_kernel<32>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NB_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace pgx
