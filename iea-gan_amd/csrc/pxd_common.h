// What the PXD kernels share.  Include after common.h.
//
//   image kernels (pxd_stats.hip, pxd_digits.hip; grid (P, N), workgroup (p, n) owns a contiguous pixel range of image n):
//       pxd_parts, PXD_LAUNCH, pxd_clip, PxdSpan, pxd_wave_scan, pxd_scan_slots, pxd_check_images
//   list kernels (pxd_clusters.hip, pxd_reco.hip, pxd_hits.hip, pxd_overlay.hip, pxd_match.hip, pxd_corr.hip; a digit list or a cluster
//   table of `cap` entries, wave g of the launch owns the entries [g * chunk, (g + 1) * chunk)):
//       pxd_blocks / cl_blocks / cl_chunk      the launch shape, from the capacity alone
//       pxd_total                              every digit, cluster and accepted total
//       PxdWaveRange                           the wave's range of a list: all six
//       pxd_digit_label                        reco, hits, match        pxd_run / pxd_run_reduce / pxd_run_sum   reco, hits, match, corr
//       pxd_wave_sum                           clusters, reco           pxd_ballot_rank                          clusters, reco, overlay
//       pxd_scan_total_kernel                  clusters, reco           pxd_scan_slots, pxd_wave_scan            overlay
//       cl_lower_bound                         clusters, overlay, match (pxd_events.hip has the workgroup-wide form of its own)
//       pxd_grid_thread / pxd_grid_threads     the kernels with one thread per entry
//   every launcher: pxd_cap, pxd_check_geometry and the pxd_check_* of capacities and pointer groups beside it; pxd_row_col.
//
// The one rule for totals: a total is read on the device through pxd_total, which clips it to [0, cap] before it bounds a loop or a label
// test, and an accepted total is clipped to the clipped cluster total.  A label or a row is compared with such a total before it indexes
// a table, so inputs that break their contract give wrong numbers, never a wrong address.  Only the overflow tests (total[0] > cap) read
// the raw value.
#pragma once

#include <climits>
#include <initializer_list>

typedef long long i64;
typedef unsigned long long u64;

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

// Launch partition of the kernels over a digit list or a cluster table of `cap` entries: B workgroups, wave g of the launch owns the entries
// [g * chunk, (g + 1) * chunk).  B = one workgroup per `per_block` entries, 1 .. max_blocks.
static inline int pxd_blocks(long entries, int per_block, int max_blocks) {
    long b = (entries + per_block - 1) / per_block;
    if (b > max_blocks) b = max_blocks;
    return (int)(b < 1 ? 1 : b);
}
#define CL_MAX_BLOCKS 1024          // one tile of the scan below: 4 * CL_MAX_BLOCKS wave slots = 4 per thread of its workgroup
static inline int cl_blocks(long cap) { return pxd_blocks(cap, 1024, CL_MAX_BLOCKS); }
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
static inline int pxd_check_capacity(const char* who, const char* name, long capacity) {
    CHECK_ARG(capacity >= 0, "%s: %s = %ld is negative", who, name, capacity);
    return 0;
}
static inline int pxd_check_whole_events(const char* who, int N, int n_sensors) {
    CHECK_ARG(n_sensors > 0 && N % n_sensors == 0, "%s: N = %d is not a multiple of n_sensors = %d", who, N, n_sensors);
    return 0;
}
static inline int pxd_check_cluster_charge(const char* who, int H, int W) {
    CHECK_ARG((double)H * W * 255.0 < 2147483648.0, "%s: H * W * 255 = %d * %d * 255 does not fit the int32 cluster charge", who, H, W);
    return 0;
}
// Checks of a group of pointers; `group` names it in the error text.
typedef std::initializer_list<const void*> PxdPtrs;
static inline bool pxd_any_null(PxdPtrs ptrs) {
    bool any = false;
    for (const void* p : ptrs) any |= p == nullptr;
    return any;
}
static inline bool pxd_all_aligned(PxdPtrs ptrs, int bytes) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    return (bits & (uintptr_t)(bytes - 1)) == 0;
}
// totals and other int32 words the kernels read whatever the capacity: non-NULL and 4-byte aligned
static inline int pxd_check_totals(const char* who, const char* group, PxdPtrs ptrs) {
    CHECK_ARG(!pxd_any_null(ptrs) && pxd_all_aligned(ptrs, 4), "%s: %s is NULL or misaligned", who, group);
    return 0;
}
// arrays a launch touches whatever the capacity (counts, tables, scratch): non-NULL and aligned to `bytes`
static inline int pxd_check_needed(const char* who, const char* group, int bytes, PxdPtrs ptrs) {
    CHECK_ARG(!pxd_any_null(ptrs) && pxd_all_aligned(ptrs, bytes), "%s: %s is NULL or not %d-byte aligned", who, group, bytes);
    return 0;
}
// arrays of `count` entries (`count_name`: "capacity", "digits", ...): non-NULL when count > 0
static inline int pxd_check_arrays(const char* who, const char* group, const char* count_name, long count, PxdPtrs ptrs) {
    CHECK_ARG(count == 0 || !pxd_any_null(ptrs), "%s: %s is NULL with %s %ld", who, group, count_name, count);
    return 0;
}
static inline int pxd_check_aligned(const char* who, const char* group, int bytes, PxdPtrs ptrs) {
    CHECK_ARG(pxd_all_aligned(ptrs, bytes), "%s: %s is not %d-byte aligned", who, group, bytes);
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

// A total read on the device, clipped to [0, cap]: the one way a kernel takes a digit, cluster or accepted total.
__device__ __forceinline__ int pxd_total(const int* __restrict__ total, int cap) { return max(min(total[0], cap), 0); }

// The grid-stride walk of the kernels with one thread per entry: first entry and step.
__device__ __forceinline__ unsigned pxd_grid_thread() { return blockIdx.x * PXD_THREADS + threadIdx.x; }
__device__ __forceinline__ unsigned pxd_grid_threads() { return gridDim.x * PXD_THREADS; }

// The range of a list of M entries that wave g of the launch owns, `chunk` entries a wave: k0 and k1 are wave-uniform, the wave walks
// for (kb = k0; kb < k1; kb += 64) with entry kb + lane in each lane, which is an entry iff it is < k1.
struct PxdWaveRange {
    int lane, g;
    long k0, k1;
    __device__ __forceinline__ PxdWaveRange(long M, long chunk) {
        lane = threadIdx.x & 63;
        g = blockIdx.x * PXD_WAVES + (threadIdx.x >> 6);
        k0 = (long)g * chunk;
        k1 = k0 + chunk < M ? k0 + chunk : M;
    }
};

// The label of digit kk of a wave's range, or -1: no digit (kk >= k1), or a label that is no row of the table of T >= 0 clusters.
__device__ __forceinline__ int pxd_digit_label(const int* __restrict__ label, long kk, long k1, int T) {
    const int lab = kk < k1 ? label[kk] : -1;
    return (unsigned)lab < (unsigned)T ? lab : -1;
}

// Sum over the 64 lanes of a wave, in every lane.
__device__ __forceinline__ int pxd_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The set lanes of a ballot below `lane`: the rank of a lane among the lanes that voted.
__device__ __forceinline__ int pxd_ballot_rank(u64 m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// Inclusive prefix sum over the 64 lanes of a wave (int or long).
template <typename T> __device__ __forceinline__ T pxd_wave_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(v, o, 64);
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

// pxd_scan_slots over the wave slots of a counting launch (groups <= CL_MAX_BLOCKS: one tile); writes the grand total.  A template, so
// that every file that launches it holds its own instance and none is defined twice in the library.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void pxd_scan_total_kernel(int* __restrict__ slots, int groups, int* __restrict__ total) {
    static_assert(THREADS == PXD_SCAN_THREADS, "pxd_scan_slots is written for PXD_SCAN_THREADS threads");
    const int all = pxd_scan_slots(slots, groups);
    if (threadIdx.x == 0) total[0] = all;
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

// The number of entries of the ascending a[0, n) below v; every probe is inside [0, n) whatever the list holds.
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
