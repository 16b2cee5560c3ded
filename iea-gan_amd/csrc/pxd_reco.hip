// Cluster reconstruction on top of pxd_clusters.hip: charge-weighted cluster positions after a seed / cluster-charge cut, and per-sensor
// position maps of the accepted clusters.  Input is one ieagan_pxd_digits + ieagan_pxd_clusters result (digit list, per-digit label, cluster
// table); every array stays in HBM.
//
//   moments   mu[j] = sum q_k * r_k,  mv[j] = sum q_k * c_k over the digits of cluster j (row r, column c inside the image), 64-bit unsigned
//   cut       cluster j is accepted iff seed[j] >= seed_cut && ccharge[j] >= charge_cut
//   accepted cluster a (cluster order kept): cluster[a] = j,  u[a] = (float)((double)mu[j] / (double)ccharge[j]),  v[a] likewise from mv
//   counts[n] accepted clusters with their first digit in image n;  total = A
//   maps      bin (mu * 25) / (ccharge * H), (mv * 48) / (ccharge * W) in 64-bit integers: count and summed charge per sensor and bin
//
// Four launches, the launch shape depends on the capacity alone (both totals are read on the device), kernel boundaries are the only
// global barriers:
//   init     wave g owns the clusters [g * chunk, (g + 1) * chunk): mu = mv = 0, the number of accepted clusters among them into the
//            wave's own slot; counts[n] = 0.
//   moments  wave g owns the digits [g * chunk, (g + 1) * chunk).  Digits ascend in flat index, so the 64 digits of a step fall into few
//            runs of equal label: a segmented sum over each run (shuffles), then one 64-bit integer atomic add per run and moment.
//   scan     pxd_scan_slots over the wave slots, in place; writes total.
//   compact  the partition of init: rank of an accepted cluster = base[slot] + accepted ones of the wave's earlier steps + accepted ones in
//            the lower lanes (ballot).  Writes cluster / u / v at the rank; counts[n] += accepted clusters of image n, one integer atomic
//            per image and step.  No atomic decides a position.
// Sums are integer adds, which commute exactly; numerator and denominator of a position are exact integers below 2^53 and the division is
// IEEE: two calls on the same clusters write the same bytes, and the host recipe in float64 reproduces u and v bit for bit.
#include "common.h"
#include "pxd_common.h"

#define PXD_MAP_U 25
#define PXD_MAP_V 48

typedef unsigned long long u64;

__device__ __forceinline__ bool reco_accept(const uint8_t* __restrict__ seed, const int* __restrict__ ccharge, int j, int seed_cut,
                                            int charge_cut) {
    return (int)seed[j] >= seed_cut && ccharge[j] >= charge_cut;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_reco_init_kernel(const uint8_t* __restrict__ seed, const int* __restrict__ ccharge,
                                                                    const int* __restrict__ ctotal, int cap, int chunk, int seed_cut,
                                                                    int charge_cut, int N, u64* __restrict__ mu, u64* __restrict__ mv,
                                                                    int* __restrict__ counts, int* __restrict__ slots) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * PXD_WAVES + (threadIdx.x >> 6);
    const long T = max(min(ctotal[0], cap), 0);
    const long j0 = (long)g * chunk;
    const long j1 = j0 + chunk < T ? j0 + chunk : T;
    int accepted = 0;
    for (long jj = j0 + lane; jj < j1; jj += 64) {
        const int j = (int)jj;
        mu[j] = 0ull;
        mv[j] = 0ull;
        accepted += (int)reco_accept(seed, ccharge, j, seed_cut, charge_cut);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) accepted += __shfl_xor(accepted, o, 64);
    if (lane == 0) slots[g] = accepted;
    for (int n = blockIdx.x * PXD_THREADS + threadIdx.x; n < N; n += gridDim.x * PXD_THREADS) counts[n] = 0;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_reco_moments_kernel(const int* __restrict__ index, const uint8_t* __restrict__ charge,
                                                                       const int* __restrict__ label, const int* __restrict__ dtotal,
                                                                       const int* __restrict__ ctotal, int cap, int chunk, int HW, int W,
                                                                       u64* __restrict__ mu, u64* __restrict__ mv) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * PXD_WAVES + (threadIdx.x >> 6);
    const long M = min(dtotal[0], cap);
    const int T = min(ctotal[0], cap);
    const long k0 = (long)g * chunk;
    const long k1 = k0 + chunk < M ? k0 + chunk : M;
    for (long kb = k0; kb < k1; kb += 64) {         // wave-uniform bounds
        const long kk = kb + lane;
        const int k = (int)kk;
        int lab = kk < k1 ? label[k] : -1;
        if ((unsigned)lab >= (unsigned)T) lab = -1;         // no digit, or not a row of the table: adds nothing
        u64 qr = 0ull, qc = 0ull;
        if (lab >= 0) {
            int r, c;
            pxd_row_col(index[k], HW, W, r, c);
            const u64 q = (u64)charge[k];
            qr = q * (u64)r;
            qc = q * (u64)c;
        }
        const PxdRun run = pxd_run(lab, lane);
        qr = pxd_run_sum(qr, lane, run.end);
        qc = pxd_run_sum(qc, lane, run.end);
        if (run.head && lab >= 0) {
            if (qr) atomicAdd(mu + lab, qr);
            if (qc) atomicAdd(mv + lab, qc);
        }
    }
}

// The prefix sum of pxd_common.h over the wave slots of the init launch (groups <= CL_MAX_BLOCKS: one tile); writes total.
__global__ __launch_bounds__(PXD_SCAN_THREADS) void pxd_reco_scan_kernel(int* __restrict__ slots, int groups, int* __restrict__ total) {
    const int all = pxd_scan_slots(slots, groups);
    if (threadIdx.x == 0) total[0] = all;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_reco_compact_kernel(const int* __restrict__ first, const int* __restrict__ ccharge,
                                                                       const uint8_t* __restrict__ seed, const int* __restrict__ ctotal,
                                                                       int cap, int chunk, int seed_cut, int charge_cut, int N, int HW,
                                                                       const u64* __restrict__ mu, const u64* __restrict__ mv,
                                                                       const int* __restrict__ slots, int* __restrict__ cluster,
                                                                       float* __restrict__ u, float* __restrict__ v, int* counts) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * PXD_WAVES + (threadIdx.x >> 6);
    const long T = max(min(ctotal[0], cap), 0);
    const long j0 = (long)g * chunk;
    const long j1 = j0 + chunk < T ? j0 + chunk : T;
    int run = slots[g];
    for (long jb = j0; jb < j1; jb += 64) {         // wave-uniform bounds
        const long jj = jb + lane;
        const int j = (int)jj;
        const bool ok = jj < j1 && reco_accept(seed, ccharge, j, seed_cut, charge_cut);
        const u64 m = __ballot(ok);
        if (m == 0ull) continue;
        int n = -1;
        if (ok) {                                   // accepted <= clusters <= capacity: the rank is inside every array
            const int a = run + __popcll(m & ((1ull << lane) - 1ull));
            const double q = (double)ccharge[j];
            cluster[a] = j;
            u[a] = (float)((double)mu[j] / q);
            v[a] = (float)((double)mv[j] / q);
            n = first[j] / HW;
        }
        run += __popcll(m);
        // `first` ascends with j: the accepted lanes of one image are neighbours, the lowest of them adds their number
        u64 rest = m;
        while (rest) {                              // wave-uniform
            const int src = __ffsll(rest) - 1;
            const int n0 = __shfl(n, src, 64);
            const u64 same = __ballot(ok && n == n0);
            if (lane == src && n0 >= 0 && n0 < N) atomicAdd(counts + n0, __popcll(same));
            rest &= ~same;
        }
    }
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_cluster_maps_kernel(const int* __restrict__ cluster, const int* __restrict__ atotal,
                                                                       const int* __restrict__ first, const int* __restrict__ ccharge,
                                                                       const u64* __restrict__ mu, const u64* __restrict__ mv,
                                                                       const int* __restrict__ ctotal, const int* __restrict__ dtotal, int cap,
                                                                       int H, int W, int n_sensors, u64* __restrict__ count,
                                                                       u64* __restrict__ charge, u64* __restrict__ overflow) {
    const int t0 = blockIdx.x * PXD_THREADS + threadIdx.x;
    if (t0 == 0 && dtotal[0] > cap) atomicAdd(overflow, 1ull);
    const int T = min(ctotal[0], cap);
    const int A = min(atotal[0], T);
    const int HW = H * W;
    for (int a = t0; a < A; a += gridDim.x * PXD_THREADS) {
        const int j = cluster[a];
        if ((unsigned)j >= (unsigned)T) continue;           // not a row of the table
        const int q = ccharge[j], f = first[j];
        if (q <= 0 || f < 0) continue;
        const u64 bu = mu[j] * PXD_MAP_U / ((u64)q * (u64)H);          // floor(u / H * 25) with u = mu / q <= H - 1: inside the grid
        const u64 bv = mv[j] * PXD_MAP_V / ((u64)q * (u64)W);
        if (bu >= PXD_MAP_U || bv >= PXD_MAP_V) continue;
        const long bin = ((long)((f / HW) % n_sensors) * PXD_MAP_U + (long)bu) * PXD_MAP_V + (long)bv;
        atomicAdd(count + bin, 1ull);
        atomicAdd(charge + bin, (u64)q);
    }
}

extern "C" long ieagan_pxd_cluster_positions_scratch(int N, int H, int W, long capacity) {
    if (N <= 0 || H <= 0 || W <= 0 || capacity < 0) return 0;
    return (long)PXD_WAVES * cl_blocks(pxd_cap(capacity));
}

extern "C" int ieagan_pxd_cluster_positions(const int* index, const unsigned char* charge, const int* label, const int* digit_total,
                                            const int* first, const int* ccharge, const unsigned char* seed, const int* cluster_total, int N,
                                            int H, int W, long capacity, int seed_cut, int charge_cut, unsigned long long* mu,
                                            unsigned long long* mv, int* cluster, float* u, float* v, int* counts, int* total, int* scratch,
                                            void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pxd_check_geometry("pxd_cluster_positions", N, H, W, true)) return rc;
    CHECK_ARG((double)H * W * 255.0 < 2147483648.0, "pxd_cluster_positions: H * W * 255 = %d * %d * 255 does not fit the int32 cluster charge", H, W);
    CHECK_ARG(capacity >= 0, "pxd_cluster_positions: capacity = %ld is negative", capacity);
    CHECK_ARG(seed_cut >= 0 && charge_cut >= 0, "pxd_cluster_positions: seed_cut = %d / charge_cut = %d is negative", seed_cut, charge_cut);
    CHECK_ARG(digit_total != nullptr && cluster_total != nullptr && (((uintptr_t)digit_total | (uintptr_t)cluster_total) & 3u) == 0,
              "pxd_cluster_positions: digit_total / cluster_total is NULL or misaligned");
    CHECK_ARG(capacity == 0 || (index != nullptr && charge != nullptr && label != nullptr),
              "pxd_cluster_positions: index / charge / label is NULL with capacity %ld", capacity);
    CHECK_ARG(capacity == 0 || (first != nullptr && ccharge != nullptr && seed != nullptr),
              "pxd_cluster_positions: a cluster table is NULL with capacity %ld", capacity);
    CHECK_ARG(capacity == 0 || (mu != nullptr && mv != nullptr && cluster != nullptr && u != nullptr && v != nullptr),
              "pxd_cluster_positions: an output array is NULL with capacity %ld", capacity);
    CHECK_ARG((((uintptr_t)index | (uintptr_t)label | (uintptr_t)first | (uintptr_t)ccharge | (uintptr_t)cluster | (uintptr_t)u | (uintptr_t)v) &
               3u) == 0, "pxd_cluster_positions: an int32 / fp32 array is not 4-byte aligned");
    CHECK_ARG((((uintptr_t)mu | (uintptr_t)mv) & 7u) == 0, "pxd_cluster_positions: mu / mv is not 8-byte aligned");
    CHECK_ARG(counts != nullptr && total != nullptr && (((uintptr_t)counts | (uintptr_t)total) & 3u) == 0,
              "pxd_cluster_positions: counts / total is NULL or misaligned");
    CHECK_ARG(scratch != nullptr && ((uintptr_t)scratch & 3u) == 0,
              "pxd_cluster_positions: scratch (ieagan_pxd_cluster_positions_scratch int32 words) is NULL or misaligned");
    const int cap = pxd_cap(capacity);
    const int HW = H * W;
    const int B = cl_blocks(cap), chunk = cl_chunk(cap, B);
    int* slots = scratch;
    ProfScope prof("pxd_cluster_positions", 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_reco_init_kernel, dim3(B), dim3(PXD_THREADS), 0, st, (const uint8_t*)seed, ccharge, cluster_total, cap, chunk, seed_cut,
                       charge_cut, N, mu, mv, counts, slots);
    CHECK_LAUNCH("pxd_cluster_positions init");
    hipLaunchKernelGGL(pxd_reco_moments_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, (const uint8_t*)charge, label, digit_total, cluster_total,
                       cap, chunk, HW, W, mu, mv);
    CHECK_LAUNCH("pxd_cluster_positions moments");
    hipLaunchKernelGGL(pxd_reco_scan_kernel, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, slots, B, total);
    CHECK_LAUNCH("pxd_cluster_positions scan");
    hipLaunchKernelGGL(pxd_reco_compact_kernel, dim3(B), dim3(PXD_THREADS), 0, st, first, ccharge, (const uint8_t*)seed, cluster_total, cap, chunk,
                       seed_cut, charge_cut, N, HW, (const u64*)mu, (const u64*)mv, (const int*)slots, cluster, u, v, counts);
    CHECK_LAUNCH("pxd_cluster_positions compact");
    return 0;
}

extern "C" int ieagan_pxd_cluster_maps(const int* cluster, const int* accepted_total, const int* first, const int* ccharge,
                                       const unsigned long long* mu, const unsigned long long* mv, const int* cluster_total,
                                       const int* digit_total, int N, int H, int W, int n_sensors, long capacity, unsigned long long* count,
                                       unsigned long long* charge, unsigned long long* overflow, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pxd_check_geometry("pxd_cluster_maps", N, H, W, true)) return rc;
    CHECK_ARG((double)H * W * 255.0 < 2147483648.0, "pxd_cluster_maps: H * W * 255 = %d * %d * 255 does not fit the int32 cluster charge", H, W);
    CHECK_ARG(n_sensors > 0 && N % n_sensors == 0, "pxd_cluster_maps: N = %d is not a multiple of n_sensors = %d", N, n_sensors);
    CHECK_ARG(capacity >= 0, "pxd_cluster_maps: capacity = %ld is negative", capacity);
    CHECK_ARG(capacity == 0 || (cluster != nullptr && first != nullptr && ccharge != nullptr && mu != nullptr && mv != nullptr),
              "pxd_cluster_maps: cluster / first / ccharge / mu / mv is NULL with capacity %ld", capacity);
    CHECK_ARG((((uintptr_t)cluster | (uintptr_t)first | (uintptr_t)ccharge) & 3u) == 0 && (((uintptr_t)mu | (uintptr_t)mv) & 7u) == 0,
              "pxd_cluster_maps: an int32 array is not 4-byte or mu / mv not 8-byte aligned");
    CHECK_ARG(accepted_total != nullptr && cluster_total != nullptr && digit_total != nullptr &&
              (((uintptr_t)accepted_total | (uintptr_t)cluster_total | (uintptr_t)digit_total) & 3u) == 0,
              "pxd_cluster_maps: accepted_total / cluster_total / digit_total is NULL or misaligned");
    CHECK_ARG(count != nullptr && charge != nullptr && overflow != nullptr &&
              (((uintptr_t)count | (uintptr_t)charge | (uintptr_t)overflow) & 7u) == 0,
              "pxd_cluster_maps: count / charge / overflow is NULL or not 8-byte aligned");
    const int cap = pxd_cap(capacity);
    ProfScope prof("pxd_cluster_maps", 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_cluster_maps_kernel, dim3(cl_blocks(cap)), dim3(PXD_THREADS), 0, st, cluster, accepted_total, first, ccharge,
                       (const u64*)mu, (const u64*)mv, cluster_total, digit_total, cap, H, W, n_sensors, (u64*)count, (u64*)charge, (u64*)overflow);
    CHECK_LAUNCH("pxd_cluster_maps");
    return 0;
}
