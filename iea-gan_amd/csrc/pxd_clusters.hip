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
//   scan     one workgroup: exclusive prefix sum over the wave slots (ascending k), in place; writes total (pxd_scan_total_kernel).
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
    const int M = pxd_total(dtotal, cap);
    for (int k = pxd_grid_thread(); k < M; k += pxd_grid_threads()) {
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
    const int M = pxd_total(dtotal, cap);
    for (int k = pxd_grid_thread(); k < M; k += pxd_grid_threads()) {
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
    const PxdWaveRange w(pxd_total(dtotal, cap), chunk);
    int roots = 0;
    for (long kk = w.k0 + w.lane; kk < w.k1; kk += 64) {
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
    roots = pxd_wave_sum(roots);
    if (w.lane == 0) slots[w.g] = roots;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_clusters_compact_kernel(const int* __restrict__ index, const int* __restrict__ dtotal, int cap,
                                                                           int chunk, const int* __restrict__ parent, const int* __restrict__ acc,
                                                                           const int* __restrict__ slots, int* __restrict__ rank,
                                                                           int* __restrict__ first, int* __restrict__ size, int* __restrict__ ccharge,
                                                                           uint8_t* __restrict__ seed, int* __restrict__ size_u,
                                                                           int* __restrict__ size_v) {
    const PxdWaveRange w(pxd_total(dtotal, cap), chunk);
    int run = slots[w.g];
    for (long kb = w.k0; kb < w.k1; kb += 64) {
        const long kk = kb + w.lane;
        const int k = (int)kk;
        const bool is_root = kk < w.k1 && parent[k] == k;
        const unsigned long long m = __ballot(is_root);
        if (m == 0ull) continue;
        if (is_root) {                              // clusters <= digits <= capacity: the rank is inside every table
            const int j = run + pxd_ballot_rank(m, w.lane);
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
    const int M = pxd_total(dtotal, cap), T = pxd_total(total, cap);
    for (int k = pxd_grid_thread(); k < M; k += pxd_grid_threads()) label[k] = rank[parent[k]];
    for (int n = pxd_grid_thread(); n < N; n += pxd_grid_threads())         // (n + 1) * HW <= N * HW < 2^31
        counts[n] = cl_lower_bound(first, T, (n + 1) * HW) - cl_lower_bound(first, T, n * HW);
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_cluster_stats_kernel(const int* __restrict__ first, const int* __restrict__ size,
                                                                        const int* __restrict__ ccharge, const uint8_t* __restrict__ seed,
                                                                        const int* __restrict__ size_u, const int* __restrict__ size_v,
                                                                        const int* __restrict__ ctotal, const int* __restrict__ dtotal, int cap, int HW,
                                                                        int n_sensors, unsigned long long* __restrict__ tables,
                                                                        unsigned long long* __restrict__ overflow) {
    const int t0 = pxd_grid_thread();
    if (t0 == 0 && dtotal[0] > cap) atomicAdd(overflow, 1ull);
    const int T = pxd_total(ctotal, cap);
    for (int j = t0; j < T; j += pxd_grid_threads()) {
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
    const char* who = "pxd_clusters";
    if (int rc = pxd_check_geometry(who, N, H, W, true)) return rc;
    if (int rc = pxd_check_cluster_charge(who, H, W)) return rc;
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    if (int rc = pxd_check_totals(who, "digit_total", {digit_total})) return rc;
    if (int rc = pxd_check_arrays(who, "index / charge", "capacity", capacity, {index, charge})) return rc;
    if (int rc = pxd_check_arrays(who, "an output table", "capacity", capacity, {label, first, size, ccharge, seed, size_u, size_v})) return rc;
    if (int rc = pxd_check_aligned(who, "an int32 array", 4, {index, label, first, size, ccharge, size_u, size_v})) return rc;
    if (int rc = pxd_check_needed(who, "counts / total", 4, {counts, total})) return rc;
    if (int rc = pxd_check_needed(who, "scratch (ieagan_pxd_clusters_scratch int32 words)", 4, {scratch})) return rc;
    const int cap = pxd_cap(capacity);
    const int HW = H * W;
    const int B = cl_blocks(cap), chunk = cl_chunk(cap, B);
    int* parent = scratch;
    int* rank = scratch + (long)cap;
    int* acc = scratch + 2L * cap;
    int* slots = scratch + (2L + CL_ACC) * cap;
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_clusters_init_kernel, dim3(B), dim3(PXD_THREADS), 0, st, digit_total, cap, parent, acc);
    CHECK_LAUNCH("pxd_clusters init");
    hipLaunchKernelGGL(pxd_clusters_link_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, digit_total, cap, HW, W, parent);
    CHECK_LAUNCH("pxd_clusters link");
    hipLaunchKernelGGL(pxd_clusters_flatten_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, (const uint8_t*)charge, digit_total, cap, chunk, HW, W,
                       parent, acc, slots);
    CHECK_LAUNCH("pxd_clusters flatten");
    hipLaunchKernelGGL(pxd_scan_total_kernel<PXD_SCAN_THREADS>, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, slots, B, total);
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
    const char* who = "pxd_cluster_stats";
    if (int rc = pxd_check_geometry(who, N, H, W, true)) return rc;
    if (int rc = pxd_check_whole_events(who, N, n_sensors)) return rc;
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    if (int rc = pxd_check_arrays(who, "a cluster table", "capacity", capacity, {first, size, ccharge, seed, size_u, size_v})) return rc;
    if (int rc = pxd_check_totals(who, "cluster_total / digit_total", {cluster_total, digit_total})) return rc;
    if (int rc = pxd_check_needed(who, "tables / overflow", 8, {tables, overflow})) return rc;
    const int cap = pxd_cap(capacity);
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_cluster_stats_kernel, dim3(cl_blocks(cap)), dim3(PXD_THREADS), 0, st, first, size, ccharge, (const uint8_t*)seed, size_u,
                       size_v, cluster_total, digit_total, cap, H * W, n_sensors, tables, overflow);
    CHECK_LAUNCH("pxd_cluster_stats");
    return 0;
}
