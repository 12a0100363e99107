// pgx_agent_tokens.hip -- token observations (pgx_agent_tokens, docs/SPEC.md S21).
//
// For every agent i one row of `length` one-byte token ids: its cost-to-go window relative to its own cost, clipped
// (W^2 entries), then S slots of 10 entries -- the agent itself and its S - 1 nearest visible agents in pgx_visible_agents'
// order: offset, goal seen from i, the caller's five recorded actions, greedy-move mask -- then PAD.  The distances are
// pgx_cost2go.hip's cached fields: the call refreshes the stale ones (launch_cost_to_go_refresh) and then makes one
// launch of the kernel below, which reads `pos`, `tgt`, `active`, the fields and the caller's history and writes nothing
// but `tokens`.
//
// One lane per agent, 256 lanes per workgroup, pgx_neighbours.hip's layout: floor(256 / A) whole envs per workgroup
// while A <= 256, ceil(A / 256) workgroups per env above.
//   1. per agent of the workgroup's envs, once: position (inactive -> far away), target, and what every observer that
//      lists the agent copies -- its five history tokens and its greedy-mask token, from its own cell and the four
//      around it in its own field (S14's rule: an undefined distance is all ones and never the smaller one) -- into LDS;
//      the lane that owns the agent's row keeps the agent's own cost;
//   2. per lane: the sweep over the env's agents with the KT smallest keys (dx^2 + dy^2, dx + r, dy + r, j) in KT
//      registers, sorted by a fully unrolled min / max chain (a private copy of pgx_neighbours.hip's: the list is never
//      indexed at run time, nothing goes to scratch);
//   3. the rows, a group of min(TK_GROUP, TK_STAGE / length) at a time, assembled in LDS: the lanes that own the group's
//      rows put their lists into LDS (every register at a compile-time index); the workgroup gathers the group's
//      windows from the fields as one flat stream of cells, neighbouring lanes neighbouring cells; each wave takes a row
//      at a time and writes its slots, a lane each; then the whole workgroup writes the group, one contiguous byte range of `tokens`, with consecutive lanes on consecutive
//      16-byte pieces.  The group is staged at the byte offset its first byte has inside
//      a 16-byte line of `tokens`, so that LDS reads and global stores are aligned together whatever `length` and the
//      base address are; the up to 15 bytes before the first and after the last whole piece go out as byte stores.
// Every loop is bounded by A, KT, W^2, `length` or the rows of a workgroup.
#include "pgx_internal.h"
#include "../../include/pogema_amd.h"

namespace pgx {
namespace {

constexpr int TK_THREADS = 256;               // lanes per workgroup
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_MAX_AGENTS = 1024;           // PGX_MAX_AGENTS: the env stage of the layout above 256 agents
constexpr int TK_GROUP = 64;                  // rows assembled at a time, at most: the rows a wave's lanes own
constexpr int TK_STAGE = 16384;               // ... and their bytes: 64 rows of 256, 8 of 2048
constexpr int TK_UNROLL = 8;                  // field loads a lane has in flight in the window gather
constexpr uint32_t TK_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t TK_FAR = 0x7FFF7FFFu;      // a staged word no window reaches: padded coordinates stay below 2048
constexpr int TK_INACTIVE = -2;               // an own cost: the row is all PAD
constexpr int TK_UNDEFINED = -1;              // ... the agent's cell has no distance: its window is all BLOCKED

static_assert(TK_STAGE >= PGX_MAX_TOKEN_LENGTH, "a group holds at least one row");
static_assert(PGX_TOKEN_HISTORY == 5 && PGX_TOKEN_SLOT_LEN == 2 + 2 + PGX_TOKEN_HISTORY + 1, "the slot layout below");
static_assert(PGX_TOKEN_ACTION0 == PGX_TOKEN_ACTION_NONE + 1, "a history code is the token's distance from ACTION_NONE");
static_assert(PGX_MAX_TOKEN_SLOTS - 1 <= 32, "the largest register list holds every neighbour slot");

__device__ __forceinline__ uint32_t tk_clip(int v) { return (uint32_t)(min(max(v, -PGX_TOKEN_CLIP), PGX_TOKEN_CLIP) + PGX_TOKEN_CLIP); }

// T: the field's cell type; KT: the register list, >= slots - 1
template <typename T, int KT>
__global__ void __launch_bounds__(TK_THREADS) agent_tokens_kernel(const TokenParams p) {
    __shared__ uint32_t s_pos[TK_MAX_AGENTS];     // pos | inactive -> TK_FAR, per agent of the workgroup's envs
    __shared__ uint32_t s_tgt[TK_MAX_AGENTS];
    __shared__ uint32_t s_info[TK_MAX_AGENTS];    // bits 3e .. 3e+2: history token e - ACTION_NONE; bits 15..18: the greedy mask
    __shared__ int s_own[TK_THREADS];             // per row of the workgroup: the agent's own cost, TK_UNDEFINED, TK_INACTIVE
    __shared__ uint32_t s_rowat[TK_THREADS];      // ... and its place in the arrays above: agent 0 of its env | the agent << 16
    constexpr int KROW = KT + 1;                  // words between the key rows of neighbouring rows (odd: no bank conflict)
    __shared__ uint32_t s_keys[TK_GROUP * KROW];  // the lists of the group's rows
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[TK_STAGE + 16];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int A = p.A, r = p.r, S = p.slots, length = p.length;
    const int ws = 2 * r + 1, ww = ws * ws;
    const size_t HW = (size_t)p.H * p.W;
    const T* field = static_cast<const T*>(p.field);
    constexpr T NONE = (T)~T(0);

    // 1. what an agent contributes: `slot` = env * A + agent, `idx` its place in the LDS arrays; returns its own cost
    auto stage_agent = [&](size_t slot, int idx) -> int {
        const uint32_t pp = p.pos[slot];
        const bool act = (p.active[slot] & ACTIVE_BIT) != 0;
        s_pos[idx] = act ? pp : TK_FAR;
        s_tgt[idx] = p.tgt[slot];
        uint32_t info = 0;                    // PGX_TOKEN_ACTION0 = PGX_TOKEN_ACTION_NONE + 1: codes 0 (none), 1 + action
#pragma unroll
        for (int q = 0; q < PGX_TOKEN_HISTORY; ++q) {
            const int v = p.history ? (int)p.history[slot * PGX_TOKEN_HISTORY + q] : -1;
            info |= ((v >= 0 && v <= 4) ? (uint32_t)(v + 1) : 0u) << (3 * q);
        }
        // the agent's cell and the four around it, moves 1..4 of docs/SPEC.md: up, down, left, right as (row, column)
        // offsets.  The five loads are unconditional, at addresses clamped into the slot's own field (cell 0 for an
        // agent that has no cell to look at), so that they are in flight together; what a clamped load returns is not used
        const int x = (int)(pp >> 16) - r, y = (int)(pp & 0xFFFFu) - r;   // unpadded
        const bool on_map = act && x >= 0 && x < p.H && y >= 0 && y < p.W;
        const int xc = on_map ? x : 0, yc = on_map ? y : 0;
        const bool up = on_map && x > 0, down = on_map && x + 1 < p.H, left = on_map && y > 0, right = on_map && y + 1 < p.W;
        const T* f = field + slot * HW;
        const T c = f[(size_t)xc * p.W + yc];
        const T cu = f[(size_t)(xc - (up ? 1 : 0)) * p.W + yc], cd = f[(size_t)(xc + (down ? 1 : 0)) * p.W + yc];
        const T cl = f[(size_t)xc * p.W + yc - (left ? 1 : 0)], cr = f[(size_t)xc * p.W + yc + (right ? 1 : 0)];
        int own = act ? TK_UNDEFINED : TK_INACTIVE;
        uint32_t bits = 0;
        if (on_map && c != NONE) {
            own = (int)c;
            bits = (up && cu < c ? 1u : 0u) | (down && cd < c ? 2u : 0u) | (left && cl < c ? 4u : 0u) | (right && cr < c ? 8u : 0u);
        }
        s_info[idx] = info | (bits << 15);
        return own;
    };

    size_t row0;                              // row (= env * A + agent) of thread 0
    int rows;                                 // rows of this workgroup: threads [0, rows) own one each
    int i, base;                              // this thread's agent and the LDS index of agent 0 of its env
    int own = TK_INACTIVE;
    if (A <= TK_THREADS) {
        const int epb = TK_THREADS / A;
        const int env0 = blockIdx.x * epb;
        const int nenv = min(epb, p.batch - env0);
        const int stride = A | 1;
        row0 = (size_t)env0 * A;
        rows = nenv * A;
        const int el = t / A;
        i = t - el * A;
        base = el * stride;
        if (t < rows) own = stage_agent(row0 + t, base + i);
    } else {
        const int bpe = (A + TK_THREADS - 1) / TK_THREADS;
        const int env = blockIdx.x / bpe, chunk = blockIdx.x - env * bpe;
        const size_t e0 = (size_t)env * A;
        row0 = e0 + (size_t)chunk * TK_THREADS;
        rows = min(TK_THREADS, A - chunk * TK_THREADS);
        i = chunk * TK_THREADS + t;
        base = 0;
        for (int j = t; j < A; j += TK_THREADS) {
            const int o = stage_agent(e0 + j, j);
            if (j == i) own = o;
        }
    }
    s_own[t] = own;
    s_rowat[t] = (uint32_t)base | ((uint32_t)(base + i) << 16);
    __syncthreads();

    // 2. the sweep (as pgx_neighbours.hip); an inactive observer's staged word is TK_FAR and it lists nobody
    const bool have = t < rows;
    const uint32_t self = have ? s_pos[base + i] : TK_FAR;
    const int xi = (int)(self >> 16), yi = (int)(self & 0xFFFFu);
    uint32_t list[KT];
#pragma unroll
    for (int q = 0; q < KT; ++q) list[q] = TK_EMPTY;
    if (S > 1) {
        const uint32_t side = 2u * (uint32_t)r;
        for (int j = 0; j < A; ++j) {
            const uint32_t w = s_pos[base + j];
            const int dx = (int)(w >> 16) - xi, dy = (int)(w & 0xFFFFu) - yi;
            const uint32_t u = (uint32_t)(dx + r), v = (uint32_t)(dy + r);
            const bool visible = u <= side && v <= side && j != i && self != TK_FAR;
            uint32_t key = ((uint32_t)(dx * dx + dy * dy) << 20) | (u << 15) | (v << 10) | (uint32_t)j;
            if (!visible) key = TK_EMPTY;
            if (__ballot(key < list[KT - 1]) != 0ull) {
#pragma unroll
                for (int q = 0; q < KT; ++q) {
                    if (q != 0 && (q & 3) == 0 && __ballot(key != TK_EMPTY) == 0ull) break;
                    const uint32_t lo = min(list[q], key);
                    key = max(list[q], key);
                    list[q] = lo;
                }
            }
        }
    }

    // 3. the rows, `group` at a time
    const int group = min(TK_GROUP, TK_STAGE / length);
    const int l0 = ww + PGX_TOKEN_SLOT_LEN * S;
    // ceil(2^32 / d) for the odd d = W^2 and W: __umulhi(n, magic) = n / d for every n below 2^32 / d (here n < 64 * 961)
    const uint32_t ww_magic = 0xFFFFFFFFu / (uint32_t)ww + 1u, ws_magic = 0xFFFFFFFFu / (uint32_t)ws + 1u;
    for (int g0 = 0; g0 < rows; g0 += group) {
        const int gn = min(group, rows - g0);
        uint8_t* dst = p.tokens + (row0 + (size_t)g0) * (size_t)length;
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
        uint8_t* src = s_stage + mis;         // row g0 + k of the group at src + k * length

        // the lists of the group's rows leave the registers, every entry at a compile-time index
        if (t >= g0 && t < g0 + gn) {
            uint32_t* kq = s_keys + (t - g0) * KROW;
#pragma unroll
            for (int q = 0; q < KT; ++q) kq[q] = list[q];
        }
        __syncthreads();                      // the keys are in place (and the last group's stores have read the stage)

        // the windows of the group as one flat stream of (row, cell) pairs: neighbouring lanes neighbouring cells.  A lane
        // issues TK_UNROLL loads before it uses the first, each unconditional at an address clamped into the row's own
        // field (cell 0 where the window cell is outside the map, the row has no window, or the stream has ended)
        const int cells = gn * ww;
        for (int it0 = t; it0 < cells; it0 += TK_THREADS * TK_UNROLL) {
            T c[TK_UNROLL];
            int at[TK_UNROLL], own_of[TK_UNROLL];   // the byte in the stage (-1: none) and the row's own cost
#pragma unroll
            for (int e = 0; e < TK_UNROLL; ++e) {
                const int it = it0 + e * TK_THREADS;
                const bool in_stream = it < cells;
                const int itc = in_stream ? it : 0;
                const int k = (int)__umulhi((uint32_t)itc, ww_magic), q = itc - k * ww;
                const int u = (int)__umulhi((uint32_t)q, ws_magic), v = q - u * ws;
                const int rr = g0 + k;        // the row = the thread that owns it
                const int o = s_own[rr];
                const uint32_t pp = s_pos[s_rowat[rr] >> 16];
                // padded position - 2r = the window's corner (unpadded)
                const int cx = (int)(pp >> 16) - 2 * r + u, cy = (int)(pp & 0xFFFFu) - 2 * r + v;
                const bool read = in_stream && o >= 0 && cx >= 0 && cx < p.H && cy >= 0 && cy < p.W;
                c[e] = field[(row0 + (size_t)rr) * HW + (read ? (size_t)cx * p.W + cy : (size_t)0)];
                own_of[e] = read ? o : TK_UNDEFINED;
                at[e] = (in_stream && o != TK_INACTIVE) ? k * length + q : -1;   // (an inactive row: its wave fills it below)
            }
#pragma unroll
            for (int e = 0; e < TK_UNROLL; ++e) {
                const uint32_t tok = (own_of[e] >= 0 && c[e] != NONE) ? tk_clip((int)c[e] - own_of[e]) : (uint32_t)PGX_TOKEN_BLOCKED;
                if (at[e] >= 0) src[at[e]] = (uint8_t)tok;
            }
        }

        // a wave per row: the slots (a lane each) and the tail, or the PADs of an inactive agent's row
        for (int k = wave; k < gn; k += TK_WAVES) {
            const int rr = g0 + k;
            uint8_t* row = src + k * length;
            if (s_own[rr] == TK_INACTIVE) {
                for (int q = lane; q < length; q += 64) row[q] = (uint8_t)PGX_TOKEN_PAD;
                continue;
            }
            const uint32_t at0 = s_rowat[rr];
            const int eb = (int)(at0 & 0xFFFFu), idx = (int)(at0 >> 16);
            const uint32_t pp = s_pos[idx];
            const int px = (int)(pp >> 16), py = (int)(pp & 0xFFFFu);
            if (lane < S) {
                uint8_t* d = row + ww + PGX_TOKEN_SLOT_LEN * lane;
                const uint32_t key = lane == 0 ? 0u : s_keys[k * KROW + lane - 1];
                if (key == TK_EMPTY) {
#pragma unroll
                    for (int e = 0; e < PGX_TOKEN_SLOT_LEN; ++e) d[e] = (uint8_t)PGX_TOKEN_PAD;
                } else {
                    const int at = lane == 0 ? idx : eb + (int)(key & 1023u);
                    const int dx = lane == 0 ? 0 : (int)((key >> 15) & 31u) - r;
                    const int dy = lane == 0 ? 0 : (int)((key >> 10) & 31u) - r;
                    const uint32_t tj = s_tgt[at];
                    const uint32_t in = s_info[at];
                    d[0] = (uint8_t)(dx + PGX_TOKEN_CLIP);
                    d[1] = (uint8_t)(dy + PGX_TOKEN_CLIP);
                    d[2] = (uint8_t)tk_clip((int)(tj >> 16) - px);
                    d[3] = (uint8_t)tk_clip((int)(tj & 0xFFFFu) - py);
#pragma unroll
                    for (int e = 0; e < PGX_TOKEN_HISTORY; ++e)
                        d[4 + e] = (uint8_t)(PGX_TOKEN_ACTION_NONE + ((in >> (3 * e)) & 7u));
                    d[9] = (uint8_t)(PGX_TOKEN_GREEDY0 + ((in >> 15) & 15u));
                }
            }
            for (int q = l0 + lane; q < length; q += 64) row[q] = (uint8_t)PGX_TOKEN_PAD;
        }
        __syncthreads();                      // the group is complete (and its keys are read)

        // bytes [0, nb) of the group: `head` up to the first 16-byte line of `tokens`, whole lines, the rest
        const uint32_t nb = (uint32_t)gn * (uint32_t)length;
        const uint32_t head = mis ? min(16u - mis, nb) : 0u;
        const uint32_t lines = (nb - head) / 16u;
        const uint32_t tail0 = head + 16u * lines;
        if ((uint32_t)t < head) dst[t] = src[t];
        for (uint32_t c = (uint32_t)t; c < lines; c += TK_THREADS)
            *reinterpret_cast<uint4*>(dst + head + 16u * c) = *reinterpret_cast<const uint4*>(src + head + 16u * c);
        if (t < 16 && tail0 + (uint32_t)t < nb) dst[tail0 + t] = src[tail0 + t];
        // no barrier here: the next group writes the stage behind the barrier that follows its key rows
    }
}

template <typename T>
hipError_t tk_launch(const TokenParams& p, hipStream_t stream) {
    const int A = p.A, n = p.slots - 1;
    const unsigned grid = A <= TK_THREADS ? (unsigned)((p.batch + TK_THREADS / A - 1) / (TK_THREADS / A))
                                          : (unsigned)p.batch * (unsigned)((A + TK_THREADS - 1) / TK_THREADS);
    auto kernel = n <= 8 ? agent_tokens_kernel<T, 8> : n <= 16 ? agent_tokens_kernel<T, 16> : agent_tokens_kernel<T, 32>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TK_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_agent_tokens(const TokenParams& p, hipStream_t stream) {
    const hipError_t err = launch_cost_to_go_refresh(p, stream);
    if (err != hipSuccess) return err;
    return p.cell_bytes == 4 ? tk_launch<uint32_t>(p, stream) : tk_launch<uint16_t>(p, stream);
}

}  // namespace pgx
