// Detector-level validation, cluster level: the sparse digits of pxd_digits.hip (flat pixel index ascending, uint8 charge) -> connected
// components under 8-connectivity, the first thing PXD reconstruction does with digits, and their per-cluster observables.
//
//   neighbours: same image, |dr| <= 1 && |dc| <= 1 (never across an image boundary, never from column W-1 to column 0 of the next row)
//   cluster j = j-th connected component in the order of its first (smallest flat index) digit: the raster numbering of
//   scipy.ndimage.label(img > 0, ones((3, 3))) per image with a running offset
//   per cluster: first, size, charge (sum), seed (max), size_u / size_v (row / column extent);  per digit: label;  per image: counts
//
// Union-find over the digit list, every quantity an integer.  Six launches, the launch shape depends on the capacity alone (the digit
// total is read on the device), kernel boundaries are the only global barriers:
//   init     parent[k] = k, the accumulators of slot k to the neutral values.
//   link     one thread per digit k: the four neighbours that precede k in flat order.  Left is digit k-1; the three of the row above are
//            found by one lower_bound for index[k] - W - 1 over [k - W - 1, k) (ascending indices: no more than W + 1 digits lie between).
//            union = find both roots, atomicMin(&parent[larger], smaller), and when the returned value shows that `larger` was no root any
//            more, go on from that value.  parent[k] <= k always and parents only decrease, so every find walks strictly downwards and
//            every failed atomicMin means another thread made progress: no thread waits on another.  Stale reads are harmless: every value
//            parent[x] ever held is an ancestor of x in the same set.
//   flatten  wave g owns the digits [g * chunk, (g + 1) * chunk): parent[k] = find(k).  Smaller roots absorb larger ones, so the root of a
//            cluster is its first digit whatever the schedule was.  Every digit adds into its root's slots with integer atomics (add, min,
//            max: order-independent, exact), and the wave stores the number of roots among its digits into its own slot.
//   scan     one workgroup: exclusive prefix sum over the wave slots (ascending k), in place; writes total.
//   compact  the partition of flatten: rank of root k = base[slot] + roots of the wave's earlier steps + roots in the lower lanes (ballot).
//            Writes the cluster table at the rank and rank[k].  No atomic decides a position.
//   label    label[k] = rank[parent[k]];  counts[n] = clusters whose first digit lies in image n (two lower_bounds over `first`).
// Two calls on the same digits write the same bytes.
#include "common.h"
#include "pxd_common.h"

#define CL_ACC 7                    // per-root accumulators: size, charge, seed, row min, row max, column min, column max

#define CL_SIZE_BINS 64
#define CL_CHARGE_BINS 256
#define CL_SEED_BINS 256
#define CL_EXTENT_BINS 32
#define CL_COLUMNS (CL_SIZE_BINS + CL_CHARGE_BINS + CL_SEED_BINS + 2 * CL_EXTENT_BINS)

__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of x, then every node of the walked path is pointed at it (an ancestor: atomicMin keeps parents decreasing).
__device__ __forceinline__ int cl_find(int* parent, int x) {
    int r = x, p;
    while ((p = cl_load(parent + r)) != r) r = p;
    while (x > r) {
        p = atomicMin(parent + x, r);
        if (p >= x) break;
        x = p;
    }
    return r;
}

__device__ __forceinline__ void cl_union(int* parent, int a, int b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;           // a was a root and now hangs below b
        a = old;                        // a had a parent already: that parent and b are still to be joined
    }
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_clusters_init_kernel(const int* __restrict__ dtotal, int cap, int* __restrict__ parent,
                                                                        int* __restrict__ acc) {
    const int M = min(dtotal[0], cap);
    for (int k = blockIdx.x * PXD_THREADS + threadIdx.x; k < M; k += gridDim.x * PXD_THREADS) {
        parent[k] = k;
        acc[k] = 0;
        acc[(long)cap + k] = 0;
        acc[2L * cap + k] = 0;
        acc[3L * cap + k] = INT_MAX;
        acc[4L * cap + k] = 0;
        acc[5L * cap + k] = INT_MAX;
        acc[6L * cap + k] = 0;
    }
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_clusters_link_kernel(const int* __restrict__ index, const int* __restrict__ dtotal, int cap,
                                                                        int HW, int W, int* parent) {
    const int M = min(dtotal[0], cap);
    for (int k = blockIdx.x * PXD_THREADS + threadIdx.x; k < M; k += gridDim.x * PXD_THREADS) {
        const int idx = index[k];
        int r, c;
        pxd_row_col(idx, HW, W, r, c);
        if (c > 0 && k > 0 && index[k - 1] == idx - 1) cl_union(parent, k, k - 1);
        if (r == 0) continue;
        const int up = idx - W;                     // the pixel above: same image, row r - 1
        int lo = k - W - 1 > 0 ? k - W - 1 : 0;
        lo += cl_lower_bound(index + lo, k - lo, up - 1);
        for (int j = lo; j < k && j < lo + 3; ++j) {
            const int d = index[j] - up;            // -1, 0, 1: up-left, up, up-right; larger: no neighbour
            if (d > 1) break;
            if (c + d >= 0 && c + d < W) cl_union(parent, k, j);
        }
    }
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_clusters_flatten_kernel(const int* __restrict__ index, const uint8_t* __restrict__ charge,
                                                                           const int* __restrict__ dtotal, int cap, int chunk, int HW, int W,
                                                                           int* parent, int* acc, int* __restrict__ slots) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * PXD_WAVES + (threadIdx.x >> 6);
    const long M = min(dtotal[0], cap);
    const long k0 = (long)g * chunk;
    const long k1 = k0 + chunk < M ? k0 + chunk : M;
    int roots = 0;
    for (long kk = k0 + lane; kk < k1; kk += 64) {
        const int k = (int)kk;
        const int root = cl_find(parent, k);
        __hip_atomic_store(parent + k, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        roots += (int)(root == k);
        const int q = (int)charge[k];
        int r, c;
        pxd_row_col(index[k], HW, W, r, c);
        atomicAdd(acc + root, 1);
        atomicAdd(acc + (long)cap + root, q);
        atomicMax(acc + 2L * cap + root, q);
        atomicMin(acc + 3L * cap + root, r);
        atomicMax(acc + 4L * cap + root, r);
        atomicMin(acc + 5L * cap + root, c);
        atomicMax(acc + 6L * cap + root, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) roots += __shfl_xor(roots, o, 64);
    if (lane == 0) slots[g] = roots;
}

// The prefix sum of pxd_common.h over the wave slots of the flatten launch (groups <= CL_MAX_BLOCKS: one tile); writes total.
__global__ __launch_bounds__(PXD_SCAN_THREADS) void pxd_clusters_scan_kernel(int* __restrict__ slots, int groups, int* __restrict__ total) {
    const int all = pxd_scan_slots(slots, groups);
    if (threadIdx.x == 0) total[0] = all;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_clusters_compact_kernel(const int* __restrict__ index, const int* __restrict__ dtotal, int cap,
                                                                           int chunk, const int* __restrict__ parent, const int* __restrict__ acc,
                                                                           const int* __restrict__ slots, int* __restrict__ rank,
                                                                           int* __restrict__ first, int* __restrict__ size, int* __restrict__ ccharge,
                                                                           uint8_t* __restrict__ seed, int* __restrict__ size_u,
                                                                           int* __restrict__ size_v) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * PXD_WAVES + (threadIdx.x >> 6);
    const long M = min(dtotal[0], cap);
    const long k0 = (long)g * chunk;
    const long k1 = k0 + chunk < M ? k0 + chunk : M;
    int run = slots[g];
    for (long kb = k0; kb < k1; kb += 64) {         // wave-uniform bounds
        const long kk = kb + lane;
        const int k = (int)kk;
        const bool is_root = kk < k1 && parent[k] == k;
        const unsigned long long m = __ballot(is_root);
        if (m == 0ull) continue;
        if (is_root) {                              // clusters <= digits <= capacity: the rank is inside every table
            const int j = run + __popcll(m & ((1ull << lane) - 1ull));
            rank[k] = j;
            first[j] = index[k];
            size[j] = acc[k];
            ccharge[j] = acc[(long)cap + k];
            seed[j] = (uint8_t)acc[2L * cap + k];
            size_u[j] = acc[4L * cap + k] - acc[3L * cap + k] + 1;
            size_v[j] = acc[6L * cap + k] - acc[5L * cap + k] + 1;
        }
        run += __popcll(m);
    }
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_clusters_label_kernel(const int* __restrict__ dtotal, int cap, const int* __restrict__ parent,
                                                                         const int* __restrict__ rank, const int* __restrict__ first,
                                                                         const int* __restrict__ total, int N, int HW, int* __restrict__ label,
                                                                         int* __restrict__ counts) {
    const int M = min(dtotal[0], cap);
    const int t0 = blockIdx.x * PXD_THREADS + threadIdx.x;
    for (int k = t0; k < M; k += gridDim.x * PXD_THREADS) label[k] = rank[parent[k]];
    const int T = total[0];
    for (int n = t0; n < N; n += gridDim.x * PXD_THREADS)       // (n + 1) * HW <= N * HW < 2^31
        counts[n] = cl_lower_bound(first, T, (n + 1) * HW) - cl_lower_bound(first, T, n * HW);
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_cluster_stats_kernel(const int* __restrict__ first, const int* __restrict__ size,
                                                                        const int* __restrict__ ccharge, const uint8_t* __restrict__ seed,
                                                                        const int* __restrict__ size_u, const int* __restrict__ size_v,
                                                                        const int* __restrict__ ctotal, const int* __restrict__ dtotal, int cap, int HW,
                                                                        int n_sensors, unsigned long long* __restrict__ tables,
                                                                        unsigned long long* __restrict__ overflow) {
    const int t0 = blockIdx.x * PXD_THREADS + threadIdx.x;
    if (t0 == 0 && dtotal[0] > cap) atomicAdd(overflow, 1ull);
    const int T = min(ctotal[0], cap);
    for (int j = t0; j < T; j += gridDim.x * PXD_THREADS) {
        unsigned long long* row = tables + (long)((first[j] / HW) % n_sensors) * CL_COLUMNS;
        atomicAdd(row + min(size[j], CL_SIZE_BINS) - 1, 1ull);
        atomicAdd(row + CL_SIZE_BINS + min(ccharge[j] >> 3, CL_CHARGE_BINS - 1), 1ull);
        atomicAdd(row + CL_SIZE_BINS + CL_CHARGE_BINS + (int)seed[j], 1ull);
        atomicAdd(row + CL_SIZE_BINS + CL_CHARGE_BINS + CL_SEED_BINS + min(size_u[j], CL_EXTENT_BINS) - 1, 1ull);
        atomicAdd(row + CL_SIZE_BINS + CL_CHARGE_BINS + CL_SEED_BINS + CL_EXTENT_BINS + min(size_v[j], CL_EXTENT_BINS) - 1, 1ull);
    }
}

extern "C" long ieagan_pxd_clusters_scratch(int N, int H, int W, long capacity) {
    if (N <= 0 || H <= 0 || W <= 0 || capacity < 0) return 0;
    const long cap = pxd_cap(capacity);
    return (2L + CL_ACC) * cap + (long)PXD_WAVES * cl_blocks(cap);
}

extern "C" int ieagan_pxd_clusters(const int* index, const unsigned char* charge, const int* digit_total, int N, int H, int W, long capacity,
                                   int* label, int* first, int* size, int* ccharge, unsigned char* seed, int* size_u, int* size_v, int* counts,
                                   int* total, int* scratch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pxd_check_geometry("pxd_clusters", N, H, W, true)) return rc;
    CHECK_ARG((double)H * W * 255.0 < 2147483648.0, "pxd_clusters: H * W * 255 = %d * %d * 255 does not fit the int32 cluster charge", H, W);
    CHECK_ARG(capacity >= 0, "pxd_clusters: capacity = %ld is negative", capacity);
    CHECK_ARG(digit_total != nullptr && ((uintptr_t)digit_total & 3u) == 0, "pxd_clusters: digit_total is NULL or misaligned");
    CHECK_ARG(capacity == 0 || (index != nullptr && charge != nullptr), "pxd_clusters: index / charge is NULL with capacity %ld", capacity);
    CHECK_ARG(capacity == 0 || (label != nullptr && first != nullptr && size != nullptr && ccharge != nullptr && seed != nullptr &&
                                size_u != nullptr && size_v != nullptr),
              "pxd_clusters: an output table is NULL with capacity %ld", capacity);
    CHECK_ARG((((uintptr_t)index | (uintptr_t)label | (uintptr_t)first | (uintptr_t)size | (uintptr_t)ccharge | (uintptr_t)size_u |
                (uintptr_t)size_v) & 3u) == 0, "pxd_clusters: an int32 array is not 4-byte aligned");
    CHECK_ARG(counts != nullptr && total != nullptr && (((uintptr_t)counts | (uintptr_t)total) & 3u) == 0,
              "pxd_clusters: counts / total is NULL or misaligned");
    CHECK_ARG(scratch != nullptr && ((uintptr_t)scratch & 3u) == 0,
              "pxd_clusters: scratch (ieagan_pxd_clusters_scratch int32 words) is NULL or misaligned");
    const int cap = pxd_cap(capacity);
    const int HW = H * W;
    const int B = cl_blocks(cap), chunk = cl_chunk(cap, B);
    int* parent = scratch;
    int* rank = scratch + (long)cap;
    int* acc = scratch + 2L * cap;
    int* slots = scratch + (2L + CL_ACC) * cap;
    ProfScope prof("pxd_clusters", 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_clusters_init_kernel, dim3(B), dim3(PXD_THREADS), 0, st, digit_total, cap, parent, acc);
    CHECK_LAUNCH("pxd_clusters init");
    hipLaunchKernelGGL(pxd_clusters_link_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, digit_total, cap, HW, W, parent);
    CHECK_LAUNCH("pxd_clusters link");
    hipLaunchKernelGGL(pxd_clusters_flatten_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, (const uint8_t*)charge, digit_total, cap, chunk, HW, W,
                       parent, acc, slots);
    CHECK_LAUNCH("pxd_clusters flatten");
    hipLaunchKernelGGL(pxd_clusters_scan_kernel, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, slots, B, total);
    CHECK_LAUNCH("pxd_clusters scan");
    hipLaunchKernelGGL(pxd_clusters_compact_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, digit_total, cap, chunk, (const int*)parent,
                       (const int*)acc, (const int*)slots, rank, first, size, ccharge, (uint8_t*)seed, size_u, size_v);
    CHECK_LAUNCH("pxd_clusters compact");
    hipLaunchKernelGGL(pxd_clusters_label_kernel, dim3(B), dim3(PXD_THREADS), 0, st, digit_total, cap, (const int*)parent, (const int*)rank,
                       (const int*)first, (const int*)total, N, HW, label, counts);
    CHECK_LAUNCH("pxd_clusters label");
    return 0;
}

extern "C" int ieagan_pxd_cluster_stats(const int* first, const int* size, const int* ccharge, const unsigned char* seed, const int* size_u,
                                        const int* size_v, const int* cluster_total, const int* digit_total, int N, int H, int W, int n_sensors,
                                        long capacity, unsigned long long* tables, unsigned long long* overflow, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pxd_check_geometry("pxd_cluster_stats", N, H, W, true)) return rc;
    CHECK_ARG(n_sensors > 0 && N % n_sensors == 0, "pxd_cluster_stats: N = %d is not a multiple of n_sensors = %d", N, n_sensors);
    CHECK_ARG(capacity >= 0, "pxd_cluster_stats: capacity = %ld is negative", capacity);
    CHECK_ARG(capacity == 0 || (first != nullptr && size != nullptr && ccharge != nullptr && seed != nullptr && size_u != nullptr &&
                                size_v != nullptr), "pxd_cluster_stats: a cluster table is NULL with capacity %ld", capacity);
    CHECK_ARG(cluster_total != nullptr && digit_total != nullptr, "pxd_cluster_stats: cluster_total / digit_total is NULL");
    CHECK_ARG(tables != nullptr && overflow != nullptr && (((uintptr_t)tables | (uintptr_t)overflow) & 7u) == 0,
              "pxd_cluster_stats: tables / overflow is NULL or not 8-byte aligned");
    const int cap = pxd_cap(capacity);
    ProfScope prof("pxd_cluster_stats", 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_cluster_stats_kernel, dim3(cl_blocks(cap)), dim3(PXD_THREADS), 0, st, first, size, ccharge, (const uint8_t*)seed, size_u,
                       size_v, cluster_total, digit_total, cap, H * W, n_sensors, tables, overflow);
    CHECK_LAUNCH("pxd_cluster_stats");
    return 0;
}
