// pgx_copy.hip -- pgx_copy_envs (docs/SPEC.md S19): environment dst[k] becomes a copy of environment src[k], on the
// device.  The per-environment state is a set of arrays [B][row bytes] (pgx_api.cpp: snapshot_segments()); a copy is a
// row gather/scatter over them, with the list of pairs read from device memory:
//   1. copy_compare_kernel  one workgroup per pair: are the padded bitmaps (and the pool indices) of the two envs equal?
//                           One flag per destination env.  Equal maps have equal map_u8 / component tables too, so the
//                           copy leaves those rows alone -- a branch inside one map moves ~17 A bytes, not 13 H W.
//   2. copy_rows_kernel     the rows.  Workgroup (pair, chunk): chunk 0 takes every small row of the pair (one launch for
//                           all of them), the chunks behind it each take a slice of one large row.  How many slices a
//                           row is cut into depends on the number of pairs alone (copy_plan_chunks), so the workgroups
//                           that find nothing to do for a pair with equal maps do not grow with the map.
// The same copy_rows_kernel moves the rows of the distance-field cache (tags, map bits, fields) in a launch of its own.
// A pair with an index outside 0..batch-1, or with src == dst, is skipped by every workgroup that meets it: nothing is
// read or written out of range whatever the index tensors hold.
#include <hip/hip_runtime.h>

#include "pgx_internal.h"

namespace pgx {

namespace {

constexpr int COPY_THREADS = 256;

// Is pair k one to copy?  Unsigned compares: a negative index is out of range too.
__device__ __forceinline__ bool copy_pair(const CopyParams& p, long long k, int& s, int& d) {
    s = p.src[k];
    d = p.dst[k];
    return (uint32_t)s < (uint32_t)p.batch && (uint32_t)d < (uint32_t)p.batch && s != d;
}

__global__ void __launch_bounds__(COPY_THREADS) copy_compare_kernel(CopyParams p, const uint32_t* __restrict__ obst,
                                                                    int bmw, const int32_t* __restrict__ map_index,
                                                                    uint8_t* __restrict__ same_map) {
    int s, d;
    if (!copy_pair(p, (long long)p.pair0 + blockIdx.x, s, d)) return;  // (uniform over the workgroup)
    const uint32_t* a = obst + (size_t)s * bmw;
    const uint32_t* b = obst + (size_t)d * bmw;
    bool diff = map_index && map_index[s] != map_index[d];
    for (int i = threadIdx.x; i < bmw; i += COPY_THREADS) diff |= a[i] != b[i];
    const int any = __syncthreads_or(diff ? 1 : 0);
    if (threadIdx.x == 0) same_map[d] = any ? 0 : 1;
}

// 16 bytes from `s`, which is aligned to `al` bytes (a power of two, 1..16; uniform over the workgroup)
__device__ __forceinline__ uint4 copy_load16(const char* s, int al) {
    if (al >= 16) return *reinterpret_cast<const uint4*>(s);
    if (al == 8) {
        const uint2 a = *reinterpret_cast<const uint2*>(s), b = *reinterpret_cast<const uint2*>(s + 8);
        return make_uint4(a.x, a.y, b.x, b.y);
    }
    if (al == 4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(s);
        return make_uint4(q[0], q[1], q[2], q[3]);
    }
    uint32_t w[4];
    if (al == 2) {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(s);
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = (uint32_t)q[2 * i] | ((uint32_t)q[2 * i + 1] << 16);
    } else {
        const uint8_t* q = reinterpret_cast<const uint8_t*>(s);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = (uint32_t)q[4 * i] | ((uint32_t)q[4 * i + 1] << 8) | ((uint32_t)q[4 * i + 2] << 16) | ((uint32_t)q[4 * i + 3] << 24);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// Slice `chunk` of `nchunks` of the copy of `row` bytes from `s` to `d`.  The body is cut on 16-byte boundaries of the
// DESTINATION (the two rows of one array need not share their offset inside a 16-byte line): 16-byte stores, loads as
// wide as the source's offset against them allows.  Head and tail, fewer than 16 bytes each, go byte by byte with
// slice 0.  `tid` of `nthreads` lanes work on it: the workgroup, or one wave of it.
__device__ __forceinline__ void copy_row_chunk(const char* __restrict__ s, char* __restrict__ d, size_t row, uint32_t chunk,
                                               uint32_t nchunks, int tid, int nthreads) {
    size_t head = (size_t)(-reinterpret_cast<uintptr_t>(d) & 15);
    if (head > row) head = row;
    const size_t vecs = (row - head) / 16;
    const size_t tail = row - head - vecs * 16;
    const uintptr_t delta = (reinterpret_cast<uintptr_t>(s) - reinterpret_cast<uintptr_t>(d)) & 15;
    const int al = delta ? (int)(delta & (~delta + 1)) : 16;
    const size_t per = (vecs + nchunks - 1) / nchunks;
    const size_t v0 = (size_t)chunk * per;
    const size_t v1 = v0 + per < vecs ? v0 + per : vecs;
    const char* sb = s + head;
    uint4* db = reinterpret_cast<uint4*>(d + head);
    for (size_t v = v0 + tid; v < v1; v += nthreads) db[v] = copy_load16(sb + v * 16, al);
    if (chunk == 0) {
        if ((size_t)tid < head) d[tid] = s[tid];
        if ((size_t)tid < tail) d[head + vecs * 16 + tid] = s[head + vecs * 16 + tid];
    }
}

__global__ void __launch_bounds__(COPY_THREADS) copy_rows_kernel(CopyParams p, const uint8_t* __restrict__ same_map) {
    const long long k = (long long)p.pair0 + blockIdx.x / p.chunks;
    const uint32_t chunk = blockIdx.x % p.chunks;
    int s, d;
    if (!copy_pair(p, k, s, d)) return;
    const bool same = same_map && same_map[d];
    if (chunk == 0) {  // the small rows of the pair, dealt out over the waves: their load-to-store latencies overlap
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        int j = 0;
        for (int i = 0; i < p.nseg; ++i) {
            const CopySeg& g = p.seg[i];
            if (g.chunk0 != 0 || (j++ & (COPY_THREADS / 64 - 1)) != wave || (g.of_map && same)) continue;
            copy_row_chunk(g.base + (size_t)s * g.row, g.base + (size_t)d * g.row, g.row, 0, 1, lane, 64);
        }
        return;
    }
    for (int i = 0; i < p.nseg; ++i) {
        const CopySeg& g = p.seg[i];
        if (chunk < g.chunk0 || chunk >= g.chunk0 + g.nchunks || (g.of_map && same)) continue;
        copy_row_chunk(g.base + (size_t)s * g.row, g.base + (size_t)d * g.row, g.row, chunk - g.chunk0, g.nchunks,
                       threadIdx.x, COPY_THREADS);
    }
}

}  // namespace

uint32_t copy_plan_chunks(CopySeg* seg, int nseg, int count) {
    // slices per large row: about COPY_TARGET_GROUPS workgroups per row array over all pairs, each of at least 16 KiB
    const size_t want = ((size_t)COPY_TARGET_GROUPS + (size_t)count - 1) / (size_t)count;
    uint32_t next = 1;  // chunk 0: every small row of the pair
    for (int i = 0; i < nseg; ++i) {
        if (seg[i].row <= COPY_SMALL_ROW) {
            seg[i].chunk0 = 0;
            seg[i].nchunks = 1;
        } else {
            const size_t most = (seg[i].row + COPY_CHUNK_VECS * 16 - 1) / (COPY_CHUNK_VECS * 16);
            seg[i].chunk0 = next;
            seg[i].nchunks = (uint32_t)(want < most ? want : most);
            next += seg[i].nchunks;
        }
    }
    return next;
}

hipError_t launch_copy_compare(CopyParams p, const uint32_t* obst, int bmw, const int32_t* map_index, uint8_t* same_map,
                               hipStream_t stream) {
    hipLaunchKernelGGL(copy_compare_kernel, dim3((unsigned)p.count), dim3(COPY_THREADS), 0, stream, p, obst, bmw, map_index, same_map);
    return hipGetLastError();
}

// One launch, but for sizes whose pairs x chunks exceed the 2^31 - 1 workgroups of a grid: those go in slices of pairs.
hipError_t launch_copy_rows(CopyParams p, const uint8_t* same_map, hipStream_t stream) {
    const long long per = 0x7FFFFFFFll / (long long)p.chunks;  // pairs per launch
    for (long long k0 = 0; k0 < p.count; k0 += per) {
        const long long n = p.count - k0 < per ? p.count - k0 : per;
        CopyParams q = p;
        q.pair0 = (int32_t)k0;
        hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)(n * p.chunks)), dim3(COPY_THREADS), 0, stream, q, same_map);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace pgx
