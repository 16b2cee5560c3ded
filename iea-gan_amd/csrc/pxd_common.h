// What the kernels over PXD sensor images share (pxd_stats.hip, pxd_digits.hip, pxd_clusters.hip, pxd_reco.hip, pxd_hits.hip, pxd_events.hip, pxd_overlay.hip, pxd_match.hip, pxd_corr.hip): the launch partition, the walk
// of a pixel range, the prefix sums, the row / column split and the launchers' argument checks.  Include after common.h.
//
// Launch partition: grid (P, N), workgroup (p, n) owns a contiguous pixel range of image n.
#pragma once

#include <climits>

#define PXD_THREADS 256
#define PXD_WAVES (PXD_THREADS / 64)
#define PXD_SCAN_THREADS 1024
#define PXD_CHUNK 4096          // pixels per block at the least: 4 float4 / 1 x 16 uint8 per thread
#define PXD_MAX_BLOCKS 2048
#define PXD_MAX_PARTS 64

static inline int pxd_parts(int N, long HW) {
    long p = (HW + PXD_CHUNK - 1) / PXD_CHUNK;
    const long cap = PXD_MAX_BLOCKS / N > 1 ? PXD_MAX_BLOCKS / N : 1;
    if (p > cap) p = cap;
    if (p > PXD_MAX_PARTS) p = PXD_MAX_PARTS;
    return (int)(p < 1 ? 1 : p);
}

static inline int pxd_cap(long capacity) { return capacity > INT_MAX ? INT_MAX : (int)capacity; }

// Launch partition of the kernels over a digit list or a cluster table of `cap` entries (pxd_clusters.hip, pxd_reco.hip): B workgroups,
// wave g of the launch owns the entries [g * chunk, (g + 1) * chunk).
#define CL_MAX_BLOCKS 1024          // one tile of the scan below: 4 * CL_MAX_BLOCKS wave slots = 4 per thread of its workgroup
static inline int cl_blocks(long cap) {
    long b = (cap + 1023) / 1024;
    if (b > CL_MAX_BLOCKS) b = CL_MAX_BLOCKS;
    return (int)(b < 1 ? 1 : b);
}
static inline int cl_chunk(long cap, int B) {       // digits per wave, a multiple of 64
    const long c = (cap + (long)B * PXD_WAVES - 1) / ((long)B * PXD_WAVES);
    return (int)((c + 63) / 64 * 64 < 64 ? 64 : (c + 63) / 64 * 64);
}

// Argument checks of the launchers, in front of the first launch; `who` is the launcher's name in the error text.  0 when they hold:
//     if (int rc = pxd_check_geometry(...)) return rc;
static inline int pxd_check_images(const char* who, const void* images, int is_u8, float threshold) {
    CHECK_ARG(images != nullptr, "%s: images is NULL", who);
    CHECK_ARG(is_u8 == 0 || is_u8 == 1, "%s: is_u8 must be 0 (fp32) or 1 (uint8), got %d", who, is_u8);
    CHECK_ARG(threshold == threshold, "%s: threshold is NaN", who);
    CHECK_ARG(is_u8 || ((uintptr_t)images & 3u) == 0, "%s: fp32 images are not 4-byte aligned", who);
    return 0;
}
static inline int pxd_check_geometry(const char* who, int N, int H, int W, bool flat_int32) {
    CHECK_ARG(N > 0 && N <= 65535, "%s: N = %d outside 1 .. 65535", who, N);
    CHECK_ARG(H > 0 && W > 0, "%s: bad image size %d x %d", who, H, W);
    CHECK_ARG(!flat_int32 || (double)N * H * W < 2147483648.0, "%s: N * H * W = %d * %d * %d does not fit the int32 flat index", who, N, H, W);
    return 0;
}

// kernel<float> or kernel<uint8_t> over grid (P, N) on the images
#define PXD_LAUNCH(kernel, is_u8, P, N, st, images, ...)                                                                              \
    do {                                                                                                                              \
        if (is_u8) hipLaunchKernelGGL(kernel<uint8_t>, dim3(P, N), dim3(PXD_THREADS), 0, st, (const uint8_t*)(images), __VA_ARGS__);  \
        else hipLaunchKernelGGL(kernel<float>, dim3(P, N), dim3(PXD_THREADS), 0, st, (const float*)(images), __VA_ARGS__);            \
    } while (0)

// The part of [s, s + n) that lies inside an image of HW pixels.
__device__ __forceinline__ long pxd_clip(long HW, long s, long n) {
    const long l = HW - s;
    return l > n ? n : l < 0 ? 0 : l;
}

// A pixel range [base, base + len) split into a scalar head up to the first 16-byte boundary, nvec vectors of V pixels (16 bytes) and a
// scalar tail from tail0 on: any H x W, any image offset.  Head and tail are shorter than V <= 16 pixels, so one step of any walk
// (stride 256 for a workgroup, 64 for a wave) covers each of them.
template <typename T, int V, typename Len> struct PxdSpan {
    const T* base;
    Len len, head, nvec, tail0;
    __device__ __forceinline__ PxdSpan(const T* b, Len l) : base(b), len(l) {
        head = (Len)(((16u - (unsigned)((uintptr_t)base & 15u)) & 15u) / sizeof(T));
        if (head > len) head = len;
        nvec = (len - head) / V;
        tail0 = head + nvec * V;
    }
};

// Inclusive prefix sum over the 64 lanes of a wave.
__device__ __forceinline__ int pxd_wave_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    return v;
}

// Exclusive prefix sum over slots[groups][PXD_WAVES] in place, in slot order, by one workgroup of PXD_SCAN_THREADS threads: thread i of a
// tile owns the four slots of group i, tiles of 1024 groups follow one another with a carry (groups <= 1024: one tile).  Every thread
// gets the grand total; the bases written are visible to the whole workgroup on return.
__device__ __forceinline__ int pxd_scan_slots(int* __restrict__ slots, int groups) {
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
        const int incl = pxd_wave_scan(mine, lane);
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
    return carry;
}

// Runs of equal label in lane order (digits ascend in flat index, so the 64 digits of a wave's step fall into few runs).  `head`: this lane
// is the first of its run; `end`: the lane behind its run's last.
struct PxdRun {
    bool head;
    int end;
};
__device__ __forceinline__ PxdRun pxd_run(int lab, int lane) {
    const int before = __shfl_up(lab, 1, 64);
    const bool head = lane == 0 || before != lab;
    const unsigned long long later = __ballot(head) & ~((2ull << lane) - 1ull);          // heads in the higher lanes
    return {head, later ? __ffsll(later) - 1 : 64};
}
// Segmented reduction over the runs: a lane combines its own run from itself to the run's end, so the head lane of a run gets it all.
template <typename T, typename Op> __device__ __forceinline__ T pxd_run_reduce(T x, int lane, int end, Op op) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_down(x, o, 64);
        if (lane + o < end) x = op(x, y);
    }
    return x;
}
template <typename T> __device__ __forceinline__ T pxd_run_sum(T x, int lane, int end) {
    return pxd_run_reduce(x, lane, end, [](T a, T b) { return a + b; });
}

__device__ __forceinline__ int cl_lower_bound(const int* __restrict__ a, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Flat pixel index -> row and column inside its image.
__device__ __forceinline__ void pxd_row_col(int idx, int HW, int W, int& r, int& c) {
    const int rem = idx % HW;
    r = rem / W;
    c = rem - r * W;
}
