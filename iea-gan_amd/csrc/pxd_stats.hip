// Detector-level validation statistics of a batch of PXD sensor images in detector units (ADU): per image the hit count and the
// summed hit charge, per sensor the ADC spectrum.  Restates the per-batch part of the reference's acceptance test
// (Evaluation/eval_all.py:75-101 get_stats, :115 the 7 ADU cut) on the device, on the tensor the export epilogue left in HBM.
//
//   v' = v < threshold ? 0 : v;   hit = v' > 0;   bin(v') = v' < 1 ? 0 : v' < 7 ? 1 : 2 + min(floor(v') - 7, 248)
//
// Launch shape: grid (P, N), block (p, n) owns the pixels [p * chunk, (p + 1) * chunk) of image n.  About 99 % of the pixels
// are zero: they touch neither LDS nor global atomics -- a block counts its hits and adds (pixels - hits) to bin 0 once.
// Hits go to the block's LDS histogram; one 64-bit integer atomic per non-empty bin and block at the end (order-independent,
// exact).  The charge is a float sum: every block stores its partial sum into its own slot and a second launch folds the P
// slots of an image in slot order, so the reported charge is bit-reproducible run to run (no float atomics).
#include "common.h"

#include "pxd_common.h"

#define PXD_BINS 251

struct PxdAcc {
    int hits;
    float charge;
};

__device__ __forceinline__ void pxd_pixel(float v, float threshold, unsigned* hist, PxdAcc& a) {
    if (!(v >= threshold) || !(v > 0.f)) return;        // below the cut, zero, negative or NaN: a bin-0 pixel, counted by difference
    a.hits += 1;
    a.charge += v;
    const int b = v < 1.f ? 0 : v < 7.f ? 1 : 2 + min((int)fminf(v, 255.f) - 7, PXD_BINS - 3);
    atomicAdd(&hist[b], 1u);
}

template <typename T> struct PxdVec;
template <> struct PxdVec<float> {
    static constexpr int V = 4;
    __device__ static __forceinline__ void run(const float* p, float threshold, unsigned* hist, PxdAcc& a) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        pxd_pixel(q.x, threshold, hist, a);
        pxd_pixel(q.y, threshold, hist, a);
        pxd_pixel(q.z, threshold, hist, a);
        pxd_pixel(q.w, threshold, hist, a);
    }
};
template <> struct PxdVec<uint8_t> {
    static constexpr int V = 16;
    __device__ static __forceinline__ void run(const uint8_t* p, float threshold, unsigned* hist, PxdAcc& a) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (w[i] == 0u) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) pxd_pixel((float)((w[i] >> (8 * j)) & 255u), threshold, hist, a);
        }
    }
};

template <typename T>
__global__ __launch_bounds__(PXD_THREADS) void pxd_stats_kernel(const T* __restrict__ x, long HW, long chunk, int n_sensors, float threshold,
                                                                unsigned long long* __restrict__ spectrum, int* __restrict__ part_hits,
                                                                float* __restrict__ part_charge) {
    __shared__ unsigned hist[256];
    __shared__ int w_hits[PXD_THREADS / 64];
    __shared__ float w_charge[PXD_THREADS / 64];
    constexpr int V = PxdVec<T>::V;
    const int tid = threadIdx.x, n = blockIdx.y, p = blockIdx.x, P = gridDim.x;
    hist[tid] = 0u;
    __syncthreads();
    const long s = (long)p * chunk;
    const PxdSpan<T, V, long> r(x + (long)n * HW + s, pxd_clip(HW, s, chunk));
    PxdAcc a = {0, 0.f};
    if (tid < r.head) pxd_pixel((float)r.base[tid], threshold, hist, a);
    for (long i = tid; i < r.nvec; i += PXD_THREADS) PxdVec<T>::run(r.base + r.head + i * V, threshold, hist, a);
    if (r.tail0 + tid < r.len) pxd_pixel((float)r.base[r.tail0 + tid], threshold, hist, a);
    // block totals in a fixed order: lanes (butterfly), then the four waves
    int h = a.hits;
    float c = a.charge;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        h += __shfl_xor(h, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if ((tid & 63) == 0) {
        w_hits[tid >> 6] = h;
        w_charge[tid >> 6] = c;
    }
    __syncthreads();
    int bh = 0;
#pragma unroll
    for (int w = 0; w < PXD_THREADS / 64; ++w) bh += w_hits[w];
    if (tid == 0) {
        float bc = 0.f;
#pragma unroll
        for (int w = 0; w < PXD_THREADS / 64; ++w) bc += w_charge[w];
        part_hits[(long)n * P + p] = bh;
        part_charge[(long)n * P + p] = bc;
    }
    if (tid < PXD_BINS) {
        unsigned long long cnt = hist[tid];
        if (tid == 0) cnt += (unsigned long long)(r.len - bh);
        if (cnt) atomicAdd(&spectrum[(long)(n % n_sensors) * PXD_BINS + tid], cnt);
    }
}

__global__ __launch_bounds__(64) void pxd_fold_kernel(const int* __restrict__ part_hits, const float* __restrict__ part_charge, int N, int P,
                                                      int* __restrict__ hits, float* __restrict__ charge) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    int h = 0;
    float c = 0.f;
    for (int p = 0; p < P; ++p) {           // slot order: the same sum every run
        h += part_hits[(long)n * P + p];
        c += part_charge[(long)n * P + p];
    }
    hits[n] = h;
    charge[n] = c;
}

extern "C" long ieagan_pxd_stats_scratch(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return 2L * N * pxd_parts(N, (long)H * W);
}

extern "C" int ieagan_pxd_stats(const void* images, int is_u8, int N, int H, int W, int n_sensors, float threshold,
                                unsigned long long* spectrum, int* hits, float* charge, float* scratch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pxd_check_images("pxd_stats", images, is_u8, threshold)) return rc;
    if (int rc = pxd_check_geometry("pxd_stats", N, H, W, false)) return rc;
    CHECK_ARG(n_sensors > 0 && N % n_sensors == 0, "pxd_stats: N = %d is not a multiple of n_sensors = %d", N, n_sensors);
    CHECK_ARG(spectrum != nullptr && ((uintptr_t)spectrum & 7u) == 0, "pxd_stats: spectrum is NULL or not 8-byte aligned");
    CHECK_ARG(hits != nullptr && charge != nullptr, "pxd_stats: hits / charge is NULL");
    CHECK_ARG(scratch != nullptr && ((uintptr_t)scratch & 3u) == 0, "pxd_stats: scratch (ieagan_pxd_stats_scratch floats) is NULL or misaligned");
    const long HW = (long)H * W;
    const int P = pxd_parts(N, HW);
    long chunk = (HW + P - 1) / P;
    chunk = (chunk + 15) / 16 * 16;
    int* part_hits = (int*)scratch;
    float* part_charge = scratch + (long)N * P;
    const double bytes = (double)N * HW * (is_u8 ? 1.0 : 4.0) + 16.0 * N * P + 8.0 * N;
    ProfScope prof(is_u8 ? "pxd_stats_u8" : "pxd_stats_f32", 0.0, bytes, st);
    PXD_LAUNCH(pxd_stats_kernel, is_u8, P, N, st, images, HW, chunk, n_sensors, threshold, spectrum, part_hits, part_charge);
    CHECK_LAUNCH("pxd_stats");
    hipLaunchKernelGGL(pxd_fold_kernel, dim3(cdiv(N, 64)), dim3(64), 0, st, (const int*)part_hits, (const float*)part_charge, N, P, hits, charge);
    CHECK_LAUNCH("pxd_stats fold");
    return 0;
}
