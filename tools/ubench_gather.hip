// micro-benchmark: the random-gather regime of MI355X HBM, the bound of the probe-search kernel.
// Every thread performs `iters` rounds of U independent 8-byte (or 4-byte) loads at pseudo-random
// element indices of a table far larger than the Infinity Cache; with DEP the next round's indices
// depend on the loaded values (the dependent chain prefix table -> key bisection -> suffix array).
// Prints gathers per second; run it under `rocprofv3 --pmc FETCH_SIZE --kernel-trace` to read the
// bytes the memory side counts per gather (calibrates FETCH_SIZE for this access width, which
// MI355X_MICROARCH.md leaves uncalibrated).
//   hipcc -O3 --offload-arch=gfx950 -o tools/bin/ubench_gather tools/ubench_gather.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

__device__ __host__ inline uint64_t mix(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

__global__ void fill(uint64_t *t, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        t[i] = mix(i);
}

template <class T, int U, bool DEP>
__global__ __launch_bounds__(256) void gather(const T *__restrict__ table, uint64_t mask, int iters,
                                              unsigned long long *out) {
    uint64_t idx = mix(((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 0x9E3779B97F4A7C15ull + 1);
    uint64_t acc = 0;
    for (int it = 0; it < iters; ++it) {
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = table[mix(idx + u) & mask];
        uint64_t s = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) s += v[u];
        acc += s;
        idx = DEP ? mix(idx ^ s) : mix(idx + 0x1234567ull);
    }
    if (acc == 0x123456789abcdefull) out[0] = acc;  // keeps the loads alive
}

template <class T, int U, bool DEP>
static void run(const void *table, size_t bytes, const char *name) {
    const uint64_t mask = bytes / sizeof(T) - 1;
    const int iters = 64 / U * 4, blocks = 256 * 8;
    unsigned long long *d_out;
    hipMalloc(&d_out, 8);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    gather<T, U, DEP><<<blocks, 256>>>((const T *)table, mask, iters, d_out);  // warm-up
    hipEventRecord(e0);
    const int reps = 5;
    for (int r = 0; r < reps; ++r) gather<T, U, DEP><<<blocks, 256>>>((const T *)table, mask, iters, d_out);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    const double gathers = (double)reps * blocks * 256 * iters * U;
    printf("%-34s %7.2f G gathers/s  (x64 B = %6.2f TB/s, x128 B = %6.2f TB/s)  %.3f ms per launch, %.0f gathers per launch\n",
           name, gathers / ms / 1e6, gathers * 64 / ms / 1e9, gathers * 128 / ms / 1e9, ms / reps,
           gathers / reps);
    hipFree(d_out);
}

// The shape of the probe search's lookup: one wave per workgroup, `a` of its 64 lanes active, every active lane walks
// chains of `c` dependent 8-byte gathers (a new chain starts at a fresh index) with ONE load in flight.  The grid is
// 256 CUs x 4 SIMDs x w workgroups, all resident from launch to exit (w <= 8), so w is the occupancy.
__global__ __launch_bounds__(64) void gather_lanes(const uint64_t *__restrict__ table, uint64_t mask, int a, int c, int chains,
                                                   unsigned long long *out) {
    if ((int)threadIdx.x >= a) return;
    uint64_t seed = mix(((uint64_t)blockIdx.x * 64u + threadIdx.x) * 0x9E3779B97F4A7C15ull + 1);
    uint64_t acc = 0;
#pragma unroll 1
    for (int it = 0; it < chains; ++it) {
        uint64_t idx = mix(seed + (uint64_t)it);
#pragma unroll 1
        for (int j = 0; j < c; ++j) {
            const uint64_t v = table[idx & mask];
            acc += v;
            idx = mix(idx ^ v);
        }
    }
    if (acc == 0x123456789abcdefull) out[0] = acc;
}

#define HIP_OK(call)                                                                              \
    do {                                                                                          \
        const hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                                   \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                            \
            return false;                                                                         \
        }                                                                                         \
    } while (0)

static bool run_lanes(const uint64_t *table, size_t bytes, int a, int w, int c) {
    const uint64_t mask = bytes / 8 - 1;
    const int blocks = 256 * 4 * w, chains = 3072 / c;
    unsigned long long *d_out;
    HIP_OK(hipMalloc(&d_out, 8));
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    gather_lanes<<<blocks, 64>>>(table, mask, a, c, chains, d_out);  // warm-up
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(e0));
    const int reps = 3;
    for (int r = 0; r < reps; ++r) gather_lanes<<<blocks, 64>>>(table, mask, a, c, chains, d_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(e1));
    HIP_OK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    if (!(ms > 0.f)) {
        fprintf(stderr, "lanes: no time measured\n");
        return false;
    }
    const double gathers = (double)reps * blocks * a * chains * c;
    printf("lanes a=%d of 64, w=%d waves per SIMD, chain c=%d: %7.2f G gathers/s, %d loads in flight per CU, %.3f ms per launch\n",
           a, w, c, gathers / ms / 1e6, 4 * w * a, ms / reps);
    HIP_OK(hipEventDestroy(e0));
    HIP_OK(hipEventDestroy(e1));
    HIP_OK(hipFree(d_out));
    return true;
}

static bool fill_table(uint64_t *table, size_t bytes) {
    fill<<<4096, 256>>>(table, bytes / 8);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    return true;
}

// usage:
//   ubench_gather [GIB]                         the rounds of U independent / dependent gathers, table of GIB (16) GiB
//   ubench_gather lanes    A W C [A W C ...]     lane fill A of 64, W waves per SIMD, chains of C: table of 16 GiB
//   ubench_gather lanes<G> A W C [A W C ...]     ... on a table of G GiB, a power of two (lanes64 ALLOCATES 64 GiB of device
//                                               memory: the index of a GRCh38-sized text spreads its gathers over 41 GB)
int main(int argc, char **argv) {
    if (argc > 1 && !strncmp(argv[1], "lanes", 5)) {
        char *end = argv[1] + 5;
        const long g = *end ? strtol(argv[1] + 5, &end, 10) : 16;
        if (*end || g < 1 || g > 128 || (g & (g - 1)) || argc < 5 || (argc - 2) % 3) {
            fprintf(stderr, "usage: %s lanes[GiB: a power of two up to 128, default 16] A W C [A W C ...]\n", argv[0]);
            return 1;
        }
        const size_t gib = (size_t)g, bytes = gib << 30;
        uint64_t *table;
        if (hipMalloc(&table, bytes) != hipSuccess) {
            fprintf(stderr, "hipMalloc(%zu GiB) failed\n", gib);
            return 1;
        }
        if (!fill_table(table, bytes)) return 1;
        printf("table %zu GiB\n", gib);
        for (int i = 2; i + 2 < argc; i += 3) {
            const int a = atoi(argv[i]), w = atoi(argv[i + 1]), c = atoi(argv[i + 2]);
            if (a < 1 || a > 64 || w < 1 || w > 8 || c < 1 || c > 3072) {
                fprintf(stderr, "lanes: 1 <= a <= 64, 1 <= w <= 8, 1 <= c <= 3072\n");
                return 1;
            }
            if (!run_lanes(table, bytes, a, w, c)) return 1;
        }
        hipFree(table);
        return 0;
    }
    if (argc > 1 && (argv[1][0] < '0' || argv[1][0] > '9')) {
        fprintf(stderr, "usage: %s [GiB] | lanes[GiB] A W C [A W C ...]\n", argv[0]);
        return 1;
    }
    const size_t gib = argc > 1 ? (size_t)atoi(argv[1]) : 16;  // power of two
    const size_t bytes = gib << 30;
    uint64_t *table;
    if (hipMalloc(&table, bytes) != hipSuccess) {
        fprintf(stderr, "hipMalloc(%zu GiB) failed\n", gib);
        return 1;
    }
    fill<<<4096, 256>>>(table, bytes / 8);
    hipDeviceSynchronize();
    printf("table %zu GiB, 2048 workgroups x 256 threads (8 waves per SIMD)\n", gib);
    run<uint64_t, 1, true>(table, bytes, "u64 x1 dependent");
    run<uint64_t, 1, false>(table, bytes, "u64 x1 independent rounds");
    run<uint64_t, 4, true>(table, bytes, "u64 x4 in flight, dependent");
    run<uint64_t, 4, false>(table, bytes, "u64 x4 in flight, independent");
    run<uint32_t, 4, false>(table, bytes, "u32 x4 in flight, independent");
    run<uint64_t, 8, false>(table, bytes, "u64 x8 in flight, independent");
    hipFree(table);
    return 0;
}
