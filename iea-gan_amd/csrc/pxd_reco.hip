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
//   scan     pxd_scan_slots over the wave slots, in place; writes total (pxd_scan_total_kernel).
//   compact  the partition of init: rank of an accepted cluster = base[slot] + accepted ones of the wave's earlier steps + accepted ones in
//            the lower lanes (ballot).  Writes cluster / u / v at the rank; counts[n] += accepted clusters of image n, one integer atomic
//            per image and step.  No atomic decides a position.
// Sums are integer adds, which commute exactly; numerator and denominator of a position are exact integers below 2^53 and the division is
// IEEE: two calls on the same clusters write the same bytes, and the host recipe in float64 reproduces u and v bit for bit.
#include "common.h"
#include "pxd_common.h"

#define PXD_MAP_U 25
#define PXD_MAP_V 48

__device__ __forceinline__ bool reco_accept(const uint8_t* __restrict__ seed, const int* __restrict__ ccharge, int j, int seed_cut,
                                            int charge_cut) {
    return (int)seed[j] >= seed_cut && ccharge[j] >= charge_cut;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_reco_init_kernel(const uint8_t* __restrict__ seed, const int* __restrict__ ccharge,
                                                                    const int* __restrict__ ctotal, int cap, int chunk, int seed_cut,
                                                                    int charge_cut, int N, u64* __restrict__ mu, u64* __restrict__ mv,
                                                                    int* __restrict__ counts, int* __restrict__ slots) {
    const PxdWaveRange w(pxd_total(ctotal, cap), chunk);
    int accepted = 0;
    for (long jj = w.k0 + w.lane; jj < w.k1; jj += 64) {
        const int j = (int)jj;
        mu[j] = 0ull;
        mv[j] = 0ull;
        accepted += (int)reco_accept(seed, ccharge, j, seed_cut, charge_cut);
    }
    accepted = pxd_wave_sum(accepted);
    if (w.lane == 0) slots[w.g] = accepted;
    for (int n = pxd_grid_thread(); n < N; n += pxd_grid_threads()) counts[n] = 0;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_reco_moments_kernel(const int* __restrict__ index, const uint8_t* __restrict__ charge,
                                                                       const int* __restrict__ label, const int* __restrict__ dtotal,
                                                                       const int* __restrict__ ctotal, int cap, int chunk, int HW, int W,
                                                                       u64* __restrict__ mu, u64* __restrict__ mv) {
    const PxdWaveRange w(pxd_total(dtotal, cap), chunk);
    const int T = pxd_total(ctotal, cap), lane = w.lane;
    for (long kb = w.k0; kb < w.k1; kb += 64) {
        const int k = (int)(kb + lane);
        const int lab = pxd_digit_label(label, kb + lane, w.k1, T);         // -1 adds nothing
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

__global__ __launch_bounds__(PXD_THREADS) void pxd_reco_compact_kernel(const int* __restrict__ first, const int* __restrict__ ccharge,
                                                                       const uint8_t* __restrict__ seed, const int* __restrict__ ctotal,
                                                                       int cap, int chunk, int seed_cut, int charge_cut, int N, int HW,
                                                                       const u64* __restrict__ mu, const u64* __restrict__ mv,
                                                                       const int* __restrict__ slots, int* __restrict__ cluster,
                                                                       float* __restrict__ u, float* __restrict__ v, int* counts) {
    const PxdWaveRange w(pxd_total(ctotal, cap), chunk);
    const int lane = w.lane;
    int run = slots[w.g];
    for (long jb = w.k0; jb < w.k1; jb += 64) {
        const long jj = jb + lane;
        const int j = (int)jj;
        const bool ok = jj < w.k1 && reco_accept(seed, ccharge, j, seed_cut, charge_cut);
        const u64 m = __ballot(ok);
        if (m == 0ull) continue;
        int n = -1;
        if (ok) {                                   // accepted <= clusters <= capacity: the rank is inside every array
            const int a = run + pxd_ballot_rank(m, lane);
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
    const int t0 = pxd_grid_thread();
    if (t0 == 0 && dtotal[0] > cap) atomicAdd(overflow, 1ull);
    const int T = pxd_total(ctotal, cap);
    const int A = pxd_total(atotal, T);
    const int HW = H * W;
    for (int a = t0; a < A; a += pxd_grid_threads()) {
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
    const char* who = "pxd_cluster_positions";
    if (int rc = pxd_check_geometry(who, N, H, W, true)) return rc;
    if (int rc = pxd_check_cluster_charge(who, H, W)) return rc;
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    CHECK_ARG(seed_cut >= 0 && charge_cut >= 0, "%s: seed_cut = %d / charge_cut = %d is negative", who, seed_cut, charge_cut);
    if (int rc = pxd_check_totals(who, "digit_total / cluster_total", {digit_total, cluster_total})) return rc;
    if (int rc = pxd_check_arrays(who, "index / charge / label", "capacity", capacity, {index, charge, label})) return rc;
    if (int rc = pxd_check_arrays(who, "a cluster table", "capacity", capacity, {first, ccharge, seed})) return rc;
    if (int rc = pxd_check_arrays(who, "an output array", "capacity", capacity, {mu, mv, cluster, u, v})) return rc;
    if (int rc = pxd_check_aligned(who, "an int32 / fp32 array", 4, {index, label, first, ccharge, cluster, u, v})) return rc;
    if (int rc = pxd_check_aligned(who, "mu / mv", 8, {mu, mv})) return rc;
    if (int rc = pxd_check_needed(who, "counts / total", 4, {counts, total})) return rc;
    if (int rc = pxd_check_needed(who, "scratch (ieagan_pxd_cluster_positions_scratch int32 words)", 4, {scratch})) return rc;
    const int cap = pxd_cap(capacity);
    const int HW = H * W;
    const int B = cl_blocks(cap), chunk = cl_chunk(cap, B);
    int* slots = scratch;
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_reco_init_kernel, dim3(B), dim3(PXD_THREADS), 0, st, (const uint8_t*)seed, ccharge, cluster_total, cap, chunk, seed_cut,
                       charge_cut, N, mu, mv, counts, slots);
    CHECK_LAUNCH("pxd_cluster_positions init");
    hipLaunchKernelGGL(pxd_reco_moments_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, (const uint8_t*)charge, label, digit_total, cluster_total,
                       cap, chunk, HW, W, mu, mv);
    CHECK_LAUNCH("pxd_cluster_positions moments");
    hipLaunchKernelGGL(pxd_scan_total_kernel<PXD_SCAN_THREADS>, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, slots, B, total);
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
    const char* who = "pxd_cluster_maps";
    if (int rc = pxd_check_geometry(who, N, H, W, true)) return rc;
    if (int rc = pxd_check_cluster_charge(who, H, W)) return rc;
    if (int rc = pxd_check_whole_events(who, N, n_sensors)) return rc;
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    if (int rc = pxd_check_arrays(who, "cluster / first / ccharge / mu / mv", "capacity", capacity, {cluster, first, ccharge, mu, mv})) return rc;
    if (int rc = pxd_check_aligned(who, "an int32 array", 4, {cluster, first, ccharge})) return rc;
    if (int rc = pxd_check_aligned(who, "mu / mv", 8, {mu, mv})) return rc;
    if (int rc = pxd_check_totals(who, "accepted_total / cluster_total / digit_total", {accepted_total, cluster_total, digit_total})) return rc;
    if (int rc = pxd_check_needed(who, "count / charge / overflow", 8, {count, charge, overflow})) return rc;
    const int cap = pxd_cap(capacity);
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_cluster_maps_kernel, dim3(cl_blocks(cap)), dim3(PXD_THREADS), 0, st, cluster, accepted_total, first, ccharge,
                       (const u64*)mu, (const u64*)mv, cluster_total, digit_total, cap, H, W, n_sensors, (u64*)count, (u64*)charge, (u64*)overflow);
    CHECK_LAUNCH("pxd_cluster_maps");
    return 0;
}
