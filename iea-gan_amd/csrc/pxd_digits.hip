// Event production: a batch of PXD sensor images in detector units (ADU) -> the sparse digits the detector software consumes,
// (flat pixel index, charge), in ascending flat index.  Restates the tail of the reference's production path
// (Physics_Analysis/create_g1.py:73-79: clamp, .to(uint8), nonzero(), gather) on the device, on the tensor the export epilogue
// left in HBM, so that only the digits (about 1 % of the pixels) cross PCIe.
//
//   q = (uint8) trunc(min(max(v, 0), 255))   (NaN -> 0);      digit iff q > 0 && v >= threshold;      uint8 input: q = v
//
// Order is part of the contract and no atomic decides a position.  Three launches:
//   count    grid (P, N), the partition of pxd_stats.  Workgroup (p, n) owns a contiguous pixel range of image n and each of its four
//            waves a contiguous quarter of it; a wave counts its digits and stores the count into its own slot [n][p][wave].
//   scan     one workgroup: exclusive prefix sum over the slots in slot order (= ascending flat index), in place; one thread per
//            workgroup of the count launch (<= 2048 unless N > 2048).  Also writes counts[N] and total.
//   compact  the count launch's grid again.  A wave walks its range in address order, 64 lanes x V pixels a step; the rank of a digit
//            is base[slot] + digits of the wave's earlier steps + digits of the lower lanes of this step (wave prefix sum) + digits
//            of the lane's lower pixels.  Stores with rank >= capacity are dropped.
// Every step of count and compact evaluates the same function of the same bytes, so the ranks fill [0, total) exactly once.
#include "common.h"
#include "pxd_common.h"

// V pixels at a 16-byte aligned address -> V / 4 dwords of packed charges, four pixels a dword in address order, 0 where the pixel
// is no digit.  `one` is the same rule for a single pixel (scalar head and tail), charge in the low byte.
template <typename T> struct DigVec;
template <> struct DigVec<float> {
    static constexpr int V = 4, W = 1;
    __device__ static __forceinline__ unsigned q(float v, float thr) {        // v >= 1 <=> trunc(clamp(v)) > 0; NaN fails it
        return (v >= 1.f && v >= thr) ? (unsigned)fminf(v, 255.f) : 0u;
    }
    __device__ static __forceinline__ unsigned one(const float* p, float thr, unsigned) { return q(*p, thr); }
    __device__ static __forceinline__ void load(const float* p, float thr, unsigned, unsigned (&w)[W]) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        w[0] = 0u;
        if ((__float_as_uint(f.x) | __float_as_uint(f.y) | __float_as_uint(f.z) | __float_as_uint(f.w)) == 0u) return;      // four zero pixels
        w[0] = q(f.x, thr) | (q(f.y, thr) << 8) | (q(f.z, thr) << 16) | (q(f.w, thr) << 24);
    }
};
template <> struct DigVec<uint8_t> {
    static constexpr int V = 16, W = 4;
    __device__ static __forceinline__ unsigned cut(unsigned w, unsigned tq) {   // clears the bytes below tq = ceil(threshold)
        if (w == 0u || tq <= 1u) return w;
        unsigned r = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned b = (w >> (8 * j)) & 255u;
            r |= (b >= tq ? b : 0u) << (8 * j);
        }
        return r;
    }
    __device__ static __forceinline__ unsigned one(const uint8_t* p, float, unsigned tq) { return cut((unsigned)*p, tq); }
    __device__ static __forceinline__ void load(const uint8_t* p, float, unsigned tq, unsigned (&w)[W]) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        w[0] = cut(u.x, tq);
        w[1] = cut(u.y, tq);
        w[2] = cut(u.z, tq);
        w[3] = cut(u.w, tq);
    }
};

__device__ __forceinline__ int pxd_nz_bytes(unsigned w) {
    return (int)((w & 0xffu) != 0u) + (int)((w & 0xff00u) != 0u) + (int)((w & 0xff0000u) != 0u) + (int)((w >> 24) != 0u);
}

// The pixel range of one wave: quarter `wave` of part p of image n.  chunk is a multiple of 64 pixels, a wave's quarter of 16.
template <typename T> using WaveRange = PxdSpan<T, DigVec<T>::V, int>;
template <typename T> __device__ __forceinline__ WaveRange<T> pxd_wave_range(const T* x, long HW, long chunk, int n, int p, int wave) {
    const long sub = chunk / PXD_WAVES, s = (long)p * chunk + (long)wave * sub;
    return WaveRange<T>(x + (long)n * HW + (s > HW ? HW : s), (int)pxd_clip(HW, s, sub));
}

template <typename T>
__global__ __launch_bounds__(PXD_THREADS) void pxd_digits_count_kernel(const T* __restrict__ x, long HW, long chunk, float thr, unsigned tq,
                                                                       int* __restrict__ slots) {
    constexpr int V = DigVec<T>::V, W = DigVec<T>::W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y, p = blockIdx.x;
    const WaveRange<T> r = pxd_wave_range(x, HW, chunk, n, p, wave);
    int c = 0;
    if (lane < r.head) c += (int)(DigVec<T>::one(r.base + lane, thr, tq) != 0u);      // head and tail are shorter than V <= 16 pixels
    for (int i = lane; i < r.nvec; i += 64) {
        unsigned w[W];
        DigVec<T>::load(r.base + r.head + (long)i * V, thr, tq, w);
#pragma unroll
        for (int k = 0; k < W; ++k) c += pxd_nz_bytes(w[k]);
    }
    if (r.tail0 + lane < r.len) c += (int)(DigVec<T>::one(r.base + r.tail0 + lane, thr, tq) != 0u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) slots[((long)n * gridDim.x + p) * PXD_WAVES + wave] = c;
}

// The prefix sum of pxd_common.h over the slots of the count launch; then counts[N] and total from the bases.
__global__ __launch_bounds__(PXD_SCAN_THREADS) void pxd_digits_scan_kernel(int* __restrict__ slots, int groups, int N, int P,
                                                                           int* __restrict__ counts, int* __restrict__ total) {
    const int tid = threadIdx.x;
    const int all = pxd_scan_slots(slots, groups);
    if (tid == 0) total[0] = all;
    for (int n = tid; n < N; n += PXD_SCAN_THREADS) {
        const int end = n + 1 < N ? slots[(long)(n + 1) * P * PXD_WAVES] : all;
        counts[n] = end - slots[(long)n * P * PXD_WAVES];
    }
}

// One step of a wave: every lane holds W dwords of packed charges whose first pixel has flat index flat0.  All 64 lanes call it.
template <int W>
__device__ __forceinline__ void pxd_wave_emit(const unsigned (&w)[W], int flat0, int lane, int& run, int cap, int* __restrict__ index,
                                              uint8_t* __restrict__ charge) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) c += pxd_nz_bytes(w[k]);
    if (__ballot(c > 0) == 0ull) return;            // wave-uniform: no digit in this step
    const int incl = pxd_wave_scan(c, lane);
    int k = run + incl - c;
    run += __shfl(incl, 63, 64);
#pragma unroll
    for (int d = 0; d < W; ++d) {
        if (w[d] == 0u) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned b = (w[d] >> (8 * j)) & 255u;
            if (b != 0u) {
                if (k < cap) {
                    index[k] = flat0 + 4 * d + j;
                    charge[k] = (uint8_t)b;
                }
                ++k;
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(PXD_THREADS) void pxd_digits_compact_kernel(const T* __restrict__ x, long HW, long chunk, float thr, unsigned tq,
                                                                         const int* __restrict__ slots, int cap, int* __restrict__ index,
                                                                         uint8_t* __restrict__ charge) {
    constexpr int V = DigVec<T>::V, W = DigVec<T>::W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y, p = blockIdx.x;
    const WaveRange<T> r = pxd_wave_range(x, HW, chunk, n, p, wave);
    int run = slots[((long)n * gridDim.x + p) * PXD_WAVES + wave];
    if (run >= cap) return;                         // wave-uniform: everything this wave would store is beyond the capacity
    const int flat = (int)(r.base - x);             // N * H * W < 2^31 (checked by the launcher)
    {
        const unsigned one[1] = {lane < r.head ? DigVec<T>::one(r.base + lane, thr, tq) : 0u};
        pxd_wave_emit<1>(one, flat + lane, lane, run, cap, index, charge);
    }
    for (int i0 = 0; i0 < r.nvec; i0 += 64) {
        const int i = i0 + lane;
        unsigned w[W];
#pragma unroll
        for (int k = 0; k < W; ++k) w[k] = 0u;
        if (i < r.nvec) DigVec<T>::load(r.base + r.head + (long)i * V, thr, tq, w);
        pxd_wave_emit<W>(w, flat + r.head + i * V, lane, run, cap, index, charge);
    }
    {
        const unsigned one[1] = {r.tail0 + lane < r.len ? DigVec<T>::one(r.base + r.tail0 + lane, thr, tq) : 0u};
        pxd_wave_emit<1>(one, flat + r.tail0 + lane, lane, run, cap, index, charge);
    }
}

extern "C" long ieagan_pxd_digits_scratch(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (long)PXD_WAVES * N * pxd_parts(N, (long)H * W);
}

extern "C" int ieagan_pxd_digits(const void* images, int is_u8, int N, int H, int W, float threshold, long capacity, int* index,
                                 unsigned char* charge, int* counts, int* total, int* scratch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pxd_check_images("pxd_digits", images, is_u8, threshold)) return rc;
    if (int rc = pxd_check_geometry("pxd_digits", N, H, W, true)) return rc;
    CHECK_ARG(capacity >= 0, "pxd_digits: capacity = %ld is negative", capacity);
    CHECK_ARG(capacity == 0 || (index != nullptr && charge != nullptr), "pxd_digits: index / charge is NULL with capacity %ld", capacity);
    CHECK_ARG(((uintptr_t)index & 3u) == 0, "pxd_digits: index is not 4-byte aligned");
    CHECK_ARG(counts != nullptr && total != nullptr && (((uintptr_t)counts | (uintptr_t)total) & 3u) == 0,
              "pxd_digits: counts / total is NULL or misaligned");
    CHECK_ARG(scratch != nullptr && ((uintptr_t)scratch & 3u) == 0, "pxd_digits: scratch (ieagan_pxd_digits_scratch int32 words) is NULL or misaligned");
    const long HW = (long)H * W;
    const int P = pxd_parts(N, HW);
    long chunk = (HW + P - 1) / P;
    chunk = (chunk + 16 * PXD_WAVES - 1) / (16 * PXD_WAVES) * (16 * PXD_WAVES);
    const int cap = pxd_cap(capacity);
    // uint8 input: v >= threshold <=> v >= ceil(threshold) in integers
    const float tc = ceilf(threshold);
    const unsigned tq = tc <= 0.f ? 0u : tc >= 256.f ? 256u : (unsigned)tc;
    // two reads of the input, the slots written, scanned (read + write) and read again, the header; the digit stores (5 bytes each)
    // depend on the data and are not counted
    const double in_bytes = (double)N * HW * (is_u8 ? 1.0 : 4.0);
    const double bytes = 2.0 * in_bytes + 4.0 * 4.0 * PXD_WAVES * N * P + 4.0 * (N + 1);
    ProfScope prof(is_u8 ? "pxd_digits_u8" : "pxd_digits_f32", 0.0, bytes, st, nullptr, in_bytes);
    PXD_LAUNCH(pxd_digits_count_kernel, is_u8, P, N, st, images, HW, chunk, threshold, tq, scratch);
    CHECK_LAUNCH("pxd_digits count");
    hipLaunchKernelGGL(pxd_digits_scan_kernel, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, scratch, N * P, N, P, counts, total);
    CHECK_LAUNCH("pxd_digits scan");
    if (cap > 0) {
        PXD_LAUNCH(pxd_digits_compact_kernel, is_u8, P, N, st, images, HW, chunk, threshold, tq, (const int*)scratch, cap, index, charge);
        CHECK_LAUNCH("pxd_digits compact");
    }
    return 0;
}
