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
#include <climits>

#include "common.h"
#include "pxd_common.h"

#define PXD_WAVES (PXD_THREADS / 64)
#define PXD_SCAN_THREADS 1024

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

// The pixel range of one wave: [start, start + len) of image n, split into a scalar head up to the first 16-byte boundary, nvec
// 16-byte vectors and a scalar tail -- any H x W and any image offset.  chunk is a multiple of 64 pixels, a wave's quarter of 16.
template <typename T> struct WaveRange {
    const T* base;
    long start;
    int head, nvec, tail0, len;
    __device__ __forceinline__ WaveRange(const T* x, long HW, long chunk, int n, int p, int wave) {
        constexpr int V = DigVec<T>::V;
        const long sub = chunk / PXD_WAVES;
        long s = (long)p * chunk + (long)wave * sub;
        long l = HW - s;
        if (l > sub) l = sub;
        if (l < 0) l = 0;
        if (s > HW) s = HW;
        start = (long)n * HW + s;
        base = x + start;
        len = (int)l;
        head = (int)(((16u - (unsigned)((uintptr_t)base & 15u)) & 15u) / sizeof(T));
        if (head > len) head = len;
        nvec = (len - head) / V;
        tail0 = head + nvec * V;
    }
};

template <typename T>
__global__ __launch_bounds__(PXD_THREADS) void pxd_digits_count_kernel(const T* __restrict__ x, long HW, long chunk, float thr, unsigned tq,
                                                                       int* __restrict__ slots) {
    constexpr int V = DigVec<T>::V, W = DigVec<T>::W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y, p = blockIdx.x;
    const WaveRange<T> r(x, HW, chunk, n, p, wave);
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

// Exclusive prefix sum over slots[groups][4] in place; thread i of a tile owns the four slots of workgroup i.
__global__ __launch_bounds__(PXD_SCAN_THREADS) void pxd_digits_scan_kernel(int* __restrict__ slots, int groups, int N, int P,
                                                                           int* __restrict__ counts, int* __restrict__ total) {
    __shared__ int wsum[PXD_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int g0 = 0; g0 < groups; g0 += PXD_SCAN_THREADS) {
        const int g = g0 + tid;
        int c[PXD_WAVES] = {0, 0, 0, 0};
        if (g < groups) {
#pragma unroll
            for (int k = 0; k < PXD_WAVES; ++k) c[k] = slots[(long)g * PXD_WAVES + k];
        }
        const int mine = c[0] + c[1] + c[2] + c[3];
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = 0, tile = 0;
#pragma unroll
        for (int k = 0; k < PXD_SCAN_THREADS / 64; ++k) {
            const int s = wsum[k];
            before += k < wave ? s : 0;
            tile += s;
        }
        int run = carry + before + incl - mine;
        if (g < groups) {
#pragma unroll
            for (int k = 0; k < PXD_WAVES; ++k) {
                slots[(long)g * PXD_WAVES + k] = run;
                run += c[k];
            }
        }
        carry += tile;
        __syncthreads();                    // wsum is rewritten by the next tile; the bases written above are visible to this workgroup
    }
    if (tid == 0) total[0] = carry;
    for (int n = tid; n < N; n += PXD_SCAN_THREADS) {
        const int end = n + 1 < N ? slots[(long)(n + 1) * P * PXD_WAVES] : carry;
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
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
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
    const WaveRange<T> r(x, HW, chunk, n, p, wave);
    int run = slots[((long)n * gridDim.x + p) * PXD_WAVES + wave];
    if (run >= cap) return;                         // wave-uniform: everything this wave would store is beyond the capacity
    const int flat = (int)r.start;                  // N * H * W < 2^31 (checked by the launcher)
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
    CHECK_ARG(images != nullptr, "pxd_digits: images is NULL");
    CHECK_ARG(is_u8 == 0 || is_u8 == 1, "pxd_digits: is_u8 must be 0 (fp32) or 1 (uint8), got %d", is_u8);
    CHECK_ARG(N > 0 && N <= 65535, "pxd_digits: N = %d outside 1 .. 65535", N);
    CHECK_ARG(H > 0 && W > 0, "pxd_digits: bad image size %d x %d", H, W);
    CHECK_ARG((double)N * H * W < 2147483648.0, "pxd_digits: N * H * W = %d * %d * %d does not fit the int32 flat index", N, H, W);
    CHECK_ARG(threshold == threshold, "pxd_digits: threshold is NaN");
    CHECK_ARG(capacity >= 0, "pxd_digits: capacity = %ld is negative", capacity);
    CHECK_ARG(capacity == 0 || (index != nullptr && charge != nullptr), "pxd_digits: index / charge is NULL with capacity %ld", capacity);
    CHECK_ARG(((uintptr_t)index & 3u) == 0, "pxd_digits: index is not 4-byte aligned");
    CHECK_ARG(counts != nullptr && total != nullptr && (((uintptr_t)counts | (uintptr_t)total) & 3u) == 0,
              "pxd_digits: counts / total is NULL or misaligned");
    CHECK_ARG(scratch != nullptr && ((uintptr_t)scratch & 3u) == 0, "pxd_digits: scratch (ieagan_pxd_digits_scratch int32 words) is NULL or misaligned");
    CHECK_ARG(is_u8 || ((uintptr_t)images & 3u) == 0, "pxd_digits: fp32 images are not 4-byte aligned");
    const long HW = (long)H * W;
    const int P = pxd_parts(N, HW);
    long chunk = (HW + P - 1) / P;
    chunk = (chunk + 16 * PXD_WAVES - 1) / (16 * PXD_WAVES) * (16 * PXD_WAVES);
    const int cap = capacity > INT_MAX ? INT_MAX : (int)capacity;
    // uint8 input: v >= threshold <=> v >= ceil(threshold) in integers
    const float tc = ceilf(threshold);
    const unsigned tq = tc <= 0.f ? 0u : tc >= 256.f ? 256u : (unsigned)tc;
    // two reads of the input, the slots written, scanned (read + write) and read again, the header; the digit stores (5 bytes each)
    // depend on the data and are not counted
    const double in_bytes = (double)N * HW * (is_u8 ? 1.0 : 4.0);
    const double bytes = 2.0 * in_bytes + 4.0 * 4.0 * PXD_WAVES * N * P + 4.0 * (N + 1);
    ProfScope prof(is_u8 ? "pxd_digits_u8" : "pxd_digits_f32", 0.0, bytes, st, nullptr, in_bytes);
    if (is_u8)
        hipLaunchKernelGGL(pxd_digits_count_kernel<uint8_t>, dim3(P, N), dim3(PXD_THREADS), 0, st, (const uint8_t*)images, HW, chunk, threshold, tq,
                           scratch);
    else
        hipLaunchKernelGGL(pxd_digits_count_kernel<float>, dim3(P, N), dim3(PXD_THREADS), 0, st, (const float*)images, HW, chunk, threshold, tq,
                           scratch);
    CHECK_LAUNCH("pxd_digits count");
    hipLaunchKernelGGL(pxd_digits_scan_kernel, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, scratch, N * P, N, P, counts, total);
    CHECK_LAUNCH("pxd_digits scan");
    if (cap > 0) {
        if (is_u8)
            hipLaunchKernelGGL(pxd_digits_compact_kernel<uint8_t>, dim3(P, N), dim3(PXD_THREADS), 0, st, (const uint8_t*)images, HW, chunk,
                               threshold, tq, (const int*)scratch, cap, index, charge);
        else
            hipLaunchKernelGGL(pxd_digits_compact_kernel<float>, dim3(P, N), dim3(PXD_THREADS), 0, st, (const float*)images, HW, chunk, threshold,
                               tq, (const int*)scratch, cap, index, charge);
        CHECK_LAUNCH("pxd_digits compact");
    }
    return 0;
}
