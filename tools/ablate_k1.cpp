/* tools/ablate_k1.cpp — doubling ablation for K1 as shipped on the headline shape
 * (k_hash_count_round<i64> — DESIGN.md §13.5): 60M rows, one i64 key, P=128, u8 pids, one
 * 1024-thread block per 4096-row round, wave w owns segment r*16 + w, 4 row groups per
 * lane with all key loads issued before the first wait, LDS atomicAdd counts, one barrier,
 * then the segoff / roundcnt / rofftab tail. Marginal phase cost = t(2x phase) - t(full);
 * a doubled phase goes to a second buffer of its own, so its pattern and its HBM traffic
 * are both doubled (a repeated access to the same address would hit in cache).
 * Variants: 1=2x key loads, 2=2x hash, 3=2x pid stores, 4=2x LDS counting, 5=2x tail
 * stores, 6=no barrier and no tail (prices them as full - t6), 7=loads one group at a
 * time (load, wait, hash, store per group: what the run-time key loop compiles to).
 * Build+run: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ablate_k1.cpp -o /tmp/ak1 && /tmp/ak1
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define WAVE 64
#define W 16
#define G 4
#define SEG (G * WAVE)
#define RROWS (W * SEG)

#define HC(x)                                                                                \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) {                                                              \
            printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__);                 \
            exit(1);                                                                         \
        }                                                                                    \
    } while (0)

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

/* keys / pid_out / segoff / roundcnt / rofftab each hold two copies (stride k2 / p2 / s2 /
 * c2 / c2 elements); the doubled phases use the second */
template <int D>
__global__ __launch_bounds__(W * WAVE) void k1_abl(
    const uint64_t *keys, int64_t k2, int64_t n, uint32_t P, uint32_t sP2, uint8_t *pid_out,
    int64_t p2, uint16_t *segoff, int64_t s2, uint32_t *roundcnt, uint16_t *rofftab,
    int64_t c2, uint32_t *sink) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wid = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    uint32_t *hist_all = (uint32_t *)smem; /* [2][W][sP2]: the second set for D == 4 */
    uint32_t *hist = hist_all + (size_t)wid * sP2;
    uint32_t *histb = hist + (size_t)W * sP2;
    const int64_t r = blockIdx.x;
    const int64_t seg = r * W + wid;
    for (uint32_t p = lane; p < sP2; p += WAVE) hist[p] = histb[p] = 0;

    const int64_t start = seg * SEG;
    const int64_t end = (start + SEG < n) ? start + SEG : n;
    uint32_t acc = 0;
    if (start < end) {
        int64_t row[G], crow[G];
        bool act[G];
        uint64_t kv[G], kw[G];
        uint32_t pid[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            row[g] = start + g * WAVE + lane;
            act[g] = row[g] < end;
            crow[g] = act[g] ? row[g] : end - 1;
        }
        if (D == 7) { /* one group at a time */
#pragma unroll
            for (int g = 0; g < G; g++) {
                kv[g] = keys[crow[g]];
                pid[g] = (uint32_t)((mix64(kv[g]) + 0x9e3779b97f4a7c15ULL) & (uint64_t)(P - 1));
                if (act[g]) pid_out[row[g]] = (uint8_t)pid[g];
                __builtin_amdgcn_s_waitcnt(0); /* vmcnt(0) expcnt(0) lgkmcnt(0) */
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int g = 0; g < G; g++) kv[g] = keys[crow[g]];
            if (D == 1) {
#pragma unroll
                for (int g = 0; g < G; g++) kw[g] = keys[k2 + crow[g]];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (D == 1) acc += (uint32_t)kw[g];
                pid[g] = (uint32_t)((mix64(kv[g]) + 0x9e3779b97f4a7c15ULL) & (uint64_t)(P - 1));
                if (D == 2) acc += (uint32_t)(mix64(kv[g] ^ 1) + 0x9e3779b97f4a7c15ULL);
            }
#pragma unroll
            for (int g = 0; g < G; g++)
                if (act[g]) pid_out[row[g]] = (uint8_t)pid[g];
            if (D == 3) {
#pragma unroll
                for (int g = 0; g < G; g++)
                    if (act[g]) pid_out[p2 + row[g]] = (uint8_t)pid[g];
            }
        }
#pragma unroll
        for (int g = 0; g < G; g++)
            if (act[g]) atomicAdd(&hist[pid[g]], 1u);
        if (D == 4) {
#pragma unroll
            for (int g = 0; g < G; g++)
                if (act[g]) atomicAdd(&histb[pid[g]], 1u);
        }
    }
    if (D != 6) {
        __syncthreads();
        const uint2 *h2 = (const uint2 *)hist_all;
        const uint32_t npair = sP2 / 2;
        const bool last = wid == W - 1;
        for (int rep = 0; rep < (D == 5 ? 2 : 1); rep++) {
            uint32_t *srow = (uint32_t *)(segoff + rep * s2 + (size_t)seg * sP2);
            uint2 *crw = (uint2 *)(roundcnt + rep * c2 + (size_t)r * sP2);
            uint32_t *orow = (uint32_t *)(rofftab + rep * c2 + (size_t)r * sP2);
            uint32_t carry = 0;
            for (uint32_t d0 = 0; d0 < npair; d0 += WAVE) {
                const uint32_t d = d0 + lane;
                const bool in = d < npair;
                uint32_t s0 = 0, s1 = 0;
                if (in) {
                    for (int w = 0; w < wid; w++) {
                        const uint2 v = h2[(size_t)w * npair + d];
                        s0 += v.x;
                        s1 += v.y;
                    }
                    srow[d] = s0 | (s1 << 16);
                }
                if (last) {
                    uint32_t c0 = 0, c1 = 0;
                    if (in) {
                        const uint2 v = h2[(size_t)wid * npair + d];
                        c0 = s0 + v.x;
                        c1 = s1 + v.y;
                        crw[d] = make_uint2(c0, c1);
                    }
                    uint32_t v = c0 + c1;
#pragma unroll
                    for (int k = 1; k < WAVE; k <<= 1) {
                        uint32_t u = (uint32_t)__shfl_up((int)v, k);
                        if (lane >= k) v += u;
                    }
                    if (in) orow[d] = (carry + v - c0 - c1) | ((carry + v - c1) << 16);
                    carry += (uint32_t)__shfl((int)v, WAVE - 1);
                }
            }
        }
    }
    if (acc == 0xdeadbeefu) sink[0] = acc;
}

int main() {
    const int64_t n = 59986052;
    const uint32_t P = 128, sP2 = 128;
    const int64_t nrounds = (n + RROWS - 1) / RROWS;
    const int64_t nseg = nrounds * W;
    std::vector<uint64_t> keys(n);
    srand(7);
    for (int64_t i = 0; i < n; i++)
        keys[i] = ((uint64_t)rand() << 32) ^ (uint64_t)rand();
    uint64_t *d_keys;
    uint8_t *d_pid;
    uint16_t *d_segoff, *d_roff;
    uint32_t *d_rcnt, *d_sink;
    const int64_t s2 = nseg * sP2, c2 = nrounds * sP2;
    HC(hipMalloc(&d_keys, 2 * n * 8));
    HC(hipMalloc(&d_pid, 2 * n));
    HC(hipMalloc(&d_segoff, 2 * s2 * 2));
    HC(hipMalloc(&d_rcnt, 2 * c2 * 4));
    HC(hipMalloc(&d_roff, 2 * c2 * 2));
    HC(hipMalloc(&d_sink, 4));
    HC(hipMemcpy(d_keys, keys.data(), n * 8, hipMemcpyHostToDevice));
    HC(hipMemcpy(d_keys + n, keys.data(), n * 8, hipMemcpyHostToDevice));
    const size_t lds = (size_t)2 * W * sP2 * 4;
    auto run = [&](auto tag, const char *name) {
        constexpr int A = decltype(tag)::value;
        hipEvent_t e0, e1;
        HC(hipEventCreate(&e0));
        HC(hipEventCreate(&e1));
        std::vector<float> t;
        for (int rep = 0; rep < 23; rep++) {
            HC(hipEventRecord(e0, 0));
            hipLaunchKernelGGL((k1_abl<A>), dim3((unsigned)nrounds), dim3(W * WAVE), lds, 0,
                               d_keys, n, n, P, sP2, d_pid, n, d_segoff, s2, d_rcnt, d_roff,
                               c2, d_sink);
            HC(hipGetLastError());
            HC(hipEventRecord(e1, 0));
            HC(hipEventSynchronize(e1));
            float ms;
            HC(hipEventElapsedTime(&ms, e0, e1));
            if (rep >= 2) t.push_back(ms);
        }
        std::sort(t.begin(), t.end());
        const float med = t[t.size() / 2];
        printf("%-26s median %.4f ms  min %.4f  max %.4f\n", name, med, t.front(), t.back());
        HC(hipEventDestroy(e0));
        HC(hipEventDestroy(e1));
        return med;
    };
    setvbuf(stdout, nullptr, _IONBF, 0);
    float full = run(std::integral_constant<int, 0>{}, "full");
    float t1 = run(std::integral_constant<int, 1>{}, "2x_key_loads");
    float t2 = run(std::integral_constant<int, 2>{}, "2x_hash");
    float t3 = run(std::integral_constant<int, 3>{}, "2x_pid_stores");
    float t4 = run(std::integral_constant<int, 4>{}, "2x_lds_counting");
    float t5 = run(std::integral_constant<int, 5>{}, "2x_tail_stores");
    float t6 = run(std::integral_constant<int, 6>{}, "no_barrier_no_tail");
    float t7 = run(std::integral_constant<int, 7>{}, "one_group_at_a_time");
    float full2 = run(std::integral_constant<int, 0>{}, "full (again)");
    printf("marginal: keys=%.3f hash=%.3f pid=%.3f lds=%.3f tail_stores=%.3f | "
           "barrier+tail=%.3f serialised_loads=%.3f | full drift %.3f\n",
           t1 - full, t2 - full, t3 - full, t4 - full, t5 - full, full - t6, t7 - full,
           full2 - full);
    return 0;
}
