// holed_stream.hip -- what a store stream with holes costs on this device (tools/time_holed_stream.py builds and runs it).
// Streams the configs[2] observation footprint (8192 environments x 64 agents x 1452 bytes = 761 MB; 16-byte nontemporal
// stores, 1 KiB per wave instruction, three waves per 92 928-byte environment slice, each wave a contiguous third -- the step
// kernel's launch shape) into three rotating buffers: dense, or leaving out, per agent, the aligned U-byte units that lie
// wholly inside the agent's target plane [1452 a + 968, 1452 a + 1452) except the units holding two pseudo-random floats
// of the plane (the old and the new 1.0).  U = 16 / 32 / 64 / 128.  Interleaved repeats, HIP events.
//   hipcc -O3 --offload-arch=gfx950 tools/holed_stream.hip -o tools/holed_stream ; tools/holed_stream [repeats] [launches]
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int ENVS = 8192, AGENTS = 64, PER_AGENT = 1452, PLANE0 = 968, SLICE = AGENTS * PER_AGENT;  // bytes
constexpr int NVEC = SLICE / 16, WAVES = 3, PART = NVEC / WAVES;
static_assert(SLICE % 128 == 0 && NVEC % WAVES == 0, "slices are whole 128-byte lines, thirds are whole float4s");

__device__ __forceinline__ uint32_t mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    return x ^ (x >> 16);
}

// ulog2 = 0: dense
__global__ __launch_bounds__(64 * WAVES) void holed_stream(char* out, int ulog2, uint32_t salt) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x4* o = reinterpret_cast<f32x4*>(out + (size_t)blockIdx.x * SLICE);
    const f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int q = wave * PART + lane; q < (wave + 1) * PART; q += 64) {
        bool skip = false;
        if (ulog2) {
            const int byte = q * 16, a = byte / PER_AGENT, p0 = a * PER_AGENT + PLANE0, p1 = (a + 1) * PER_AGENT;
            const int u = byte >> ulog2, u0 = u << ulog2;
            const uint32_t h = mix((uint32_t)(blockIdx.x * AGENTS + a) ^ salt);
            const int was = (p0 + 4 * (int)(h % 121u)) >> ulog2, now = (p0 + 4 * (int)((h >> 16) % 121u)) >> ulog2;
            skip = u0 >= p0 && u0 + (1 << ulog2) <= p1 && u != was && u != now;
        }
        if (!skip) __builtin_nontemporal_store(v, &o[q]);
    }
}

int main(int argc, char** argv) {
    const int repeats = argc > 1 ? atoi(argv[1]) : 6, launches = argc > 2 ? atoi(argv[2]) : 12;
    const size_t bytes = (size_t)ENVS * SLICE;
    char* buf[3];
    for (auto& b : buf) {
        CHECK(hipMalloc(&b, bytes));
        CHECK(hipMemset(b, 0, bytes));
    }
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const int modes[5] = {0, 4, 5, 6, 7};
    printf("footprint %zu bytes, %d launches per timing, three rotating buffers\n", bytes, launches);
    for (int w = 0; w < 3; ++w) hipLaunchKernelGGL(holed_stream, dim3(ENVS), dim3(64 * WAVES), 0, 0, buf[w], 0, 0u);
    CHECK(hipDeviceSynchronize());
    for (int rep = 0; rep < repeats; ++rep) {
        for (int m : modes) {
            CHECK(hipEventRecord(e0, 0));
            for (int k = 0; k < launches; ++k)
                hipLaunchKernelGGL(holed_stream, dim3(ENVS), dim3(64 * WAVES), 0, 0, buf[k % 3], m, (uint32_t)(rep * 64 + k));
            CHECK(hipEventRecord(e1, 0));
            CHECK(hipEventSynchronize(e1));
            CHECK(hipGetLastError());
            float ms = 0.f;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            printf("repeat %d unit %3d B: %8.2f us per launch\n", rep, m ? 1 << m : 0, ms * 1e3f / launches);
        }
    }
    for (auto& b : buf) CHECK(hipFree(b));
    return 0;
}
