// Intra-event correlations: the per-event occupancy of every region of every sensor, its second moments over the events, and the rank
// transform that Spearman's coefficient needs.  A grid of RU x RV regions lies over every sensor; a digit at row r, column c of image n
// belongs to event e = n / S, sensor s = n % S and region ru = (r * RU) / H, rv = (c * RV) / W, all in integers, and counts for column
// k = (s * RU + ru) * RV + rv of R = S * RU * RV columns (1 <= RU <= H, 1 <= RV <= W, R <= 1024).
//
//   ieagan_pxd_region_counts   digit list of a batch -> x [E, R] int32, x[e, k] = the digits of event e in column k
//   ieagan_pxd_gram            gram [R, R] += x^T x and sum [R] += column sums of any int32 x [E, R], int64: the moments of the counts of an
//                              update and of the ranks of a result
//   ieagan_pxd_ranks           x [E, R] -> rank2 [E, R] int32, rank2[e, k] = 2 #{e' : x[e', k] < x[e, k]} + #{e' : x[e', k] == x[e, k]} + 1:
//                              twice the mid-rank (ties get the average rank), an integer
// The host forms cov_ij = n gram_ij - sum_i sum_j in exact integers and one float64 quotient per pair; no float exists on the device.
//
// Exact.  x <= H * W, so an entry of gram grows by at most (H * W)^2 an event: it cannot overflow below 2^63 / (H * W)^2 events, 2.5e8 at
// 250 x 768.  rank2 <= 2 E + 1 with E <= 65535 fits int32, and its Gram is at most E (2 E + 1)^2 < 2^51.  The counts are added with int32
// atomics, which commute; every entry of gram / sum has one writer (a plain 64-bit read-modify-write, successive calls are ordered by the
// stream); a rank is counted by one thread.  Two calls on the same input write the same bytes.
//
// Kernels.
//   counts   the launch partition of the digit-list kernels (cl_blocks / cl_chunk): one lane per digit below pxd_total.  Digits
//            ascend in flat index, so the 64 digits of a wave's step fall into few runs of equal (e, k): pxd_run / pxd_run_sum and one
//            atomicAdd per run.  x is zeroed by a launch of its own in front.
//   gram     thread (i, j): the lanes of a wave are 64 consecutive columns j (x[e, j] is one 256-byte access) and the wave holds GR_ROWS rows
//            i, whose x[e, i] its first GR_ROWS lanes load and every lane reads through readlane (uniform across the wave); a workgroup
//            holds GR_ROWS * PXD_WAVES rows.  GR_DEPTH rows e are loaded before the first is used.  Both triangles are computed: the
//            table is symmetric by construction.  The threads of row 0 also own sum[j].
//   ranks    lanes = 64 consecutive columns, a thread keeps RK_OWN events of its column in registers, a workgroup RK_OWN * PXD_WAVES events.
//            It streams all E rows once (a row is one 256-byte access per wave, the four waves of a workgroup read the same lines) and
//            adds (v < own) + (v <= own) per owned event: 2 less + equal.  O(E^2 R) compares, 3.2e10 at 10 000 events and R = 320.
//   Edge tiles (R no multiple of 64, E no multiple of the rows of a workgroup) are predicated: nothing is read or written out of range.
//
// Safe.  The digit total is clipped to [0, capacity] before it bounds a loop; a digit whose flat index is outside [0, N * H * W) is skipped,
// every other index gives e < E and k < R by the arithmetic above: inputs that break their contract give wrong numbers, never a wrong
// address.  The launchers refuse, before any launch, NULL or misaligned pointers, a geometry outside pxd_check_geometry, N % n_sensors != 0,
// regions outside the bounds above, a negative capacity and E outside 1 .. 65535.
#include "common.h"
#include "pxd_common.h"

#define CORR_MAX_COLUMNS 1024
#define CORR_MAX_EVENTS 65535
#define GR_ROWS 4               // rows i of a wave of the Gram kernel
#define GR_DEPTH 8              // rows e of x it loads before it uses the first
#define RK_OWN 16               // events a thread of the rank kernel owns
#define RK_DEPTH 4              // rows e' of x it loads before it uses the first

__global__ __launch_bounds__(PXD_THREADS) void pxd_corr_zero_kernel(int* __restrict__ x, long n) {
    for (long t = pxd_grid_thread(); t < n; t += pxd_grid_threads()) x[t] = 0;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_region_counts_kernel(const int* __restrict__ index, const int* __restrict__ dtotal, int cap,
                                                                        int chunk, long NHW, int HW, int H, int W, int S, int RU, int RV,
                                                                        int* __restrict__ x, u64* __restrict__ overflow) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && dtotal[0] > cap) atomicAdd(overflow, 1ull);
    const PxdWaveRange w(pxd_total(dtotal, cap), chunk);
    const int R = S * RU * RV, lane = w.lane;
    for (long kb = w.k0; kb < w.k1; kb += 64) {
        const long kk = kb + lane;
        int lab = -1;                               // no digit, or a flat index outside the batch
        if (kk < w.k1) {
            const int idx = index[kk];
            if (idx >= 0 && (long)idx < NHW) {
                int r, c;
                pxd_row_col(idx, HW, W, r, c);
                const int n = idx / HW;
                const int ru = (int)((long)r * RU / H), rv = (int)((long)c * RV / W);
                lab = (n / S) * R + ((n % S) * RU + ru) * RV + rv;          // < E * R <= 65535 * 1024
            }
        }
        const PxdRun run = pxd_run(lab, lane);
        const int cnt = pxd_run_sum(lab >= 0 ? 1 : 0, lane, run.end);
        if (run.head && lab >= 0) atomicAdd(x + lab, cnt);
    }
}

// grid (ceil(R / 64), ceil(R / (GR_ROWS * PXD_WAVES))): wave w of workgroup (bx, by) owns the rows i0 .. i0 + GR_ROWS - 1, lane l column j.
__global__ __launch_bounds__(PXD_THREADS) void pxd_gram_kernel(const int* __restrict__ x, int E, int R, i64* __restrict__ gram,
                                                               i64* __restrict__ sum) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = blockIdx.x * 64 + lane;
    const int i0 = (blockIdx.y * PXD_WAVES + wave) * GR_ROWS;
    if (i0 >= R) return;                            // wave-uniform
    const bool col = j < R;                         // a lane past the last column reads column 0 and stores nothing
    const int ri = min(i0 + (lane & (GR_ROWS - 1)), R - 1);         // lane t < GR_ROWS loads row i0 + t; a row past R reads row R - 1 and is not stored
    i64 acc[GR_ROWS] = {0, 0, 0, 0}, s = 0;
    const int* __restrict__ xi_p = x + ri;
    const int* __restrict__ xj_p = x + (col ? j : 0);
    int e = 0;
    for (; e + GR_DEPTH <= E; e += GR_DEPTH) {      // GR_DEPTH rows of loads in flight
        int xi[GR_DEPTH], xj[GR_DEPTH];
#pragma unroll
        for (int u = 0; u < GR_DEPTH; ++u) {
            xi[u] = xi_p[(long)(e + u) * R];
            xj[u] = xj_p[(long)(e + u) * R];
        }
#pragma unroll
        for (int u = 0; u < GR_DEPTH; ++u) {
            s += xj[u];
#pragma unroll
            for (int t = 0; t < GR_ROWS; ++t) acc[t] += (i64)__builtin_amdgcn_readlane(xi[u], t) * xj[u];
        }
    }
    for (; e < E; ++e) {
        const int xi = xi_p[(long)e * R], xj = xj_p[(long)e * R];
        s += xj;
#pragma unroll
        for (int t = 0; t < GR_ROWS; ++t) acc[t] += (i64)__builtin_amdgcn_readlane(xi, t) * xj;
    }
    if (!col) return;
#pragma unroll
    for (int t = 0; t < GR_ROWS; ++t)
        if (i0 + t < R) gram[(long)(i0 + t) * R + j] += acc[t];
    if (i0 == 0) sum[j] += s;
}

// grid (ceil(R / 64), ceil(E / (RK_OWN * PXD_WAVES))): lane l of wave w of workgroup (bx, by) owns column k and the events e0 .. e0 + RK_OWN - 1.
__global__ __launch_bounds__(PXD_THREADS) void pxd_ranks_kernel(const int* __restrict__ x, int E, int R, int* __restrict__ rank2) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.x * 64 + lane;
    const int e0 = (blockIdx.y * PXD_WAVES + wave) * RK_OWN;
    if (e0 >= E || k >= R) return;                  // a lane past the last column reads and writes nothing
    const int* __restrict__ xk = x + k;
    int own[RK_OWN], acc[RK_OWN];
#pragma unroll
    for (int t = 0; t < RK_OWN; ++t) {
        own[t] = xk[(long)min(e0 + t, E - 1) * R];  // an event past E repeats event E - 1 and is not stored
        acc[t] = 1;
    }
    int e = 0;
    for (; e + RK_DEPTH <= E; e += RK_DEPTH) {      // RK_DEPTH rows of loads in flight
        int v[RK_DEPTH];
#pragma unroll
        for (int u = 0; u < RK_DEPTH; ++u) v[u] = xk[(long)(e + u) * R];
#pragma unroll
        for (int u = 0; u < RK_DEPTH; ++u)
#pragma unroll
            for (int t = 0; t < RK_OWN; ++t) acc[t] += (v[u] < own[t] ? 1 : 0) + (v[u] <= own[t] ? 1 : 0);
    }
    for (; e < E; ++e) {
        const int v = xk[(long)e * R];
#pragma unroll
        for (int t = 0; t < RK_OWN; ++t) acc[t] += (v < own[t] ? 1 : 0) + (v <= own[t] ? 1 : 0);
    }
#pragma unroll
    for (int t = 0; t < RK_OWN; ++t)
        if (e0 + t < E) rank2[(long)(e0 + t) * R + k] = acc[t];
}

// x [E, R] of the two kernels over a table: 1 <= E <= 65535, 1 <= R <= 1024
static int corr_check_table(const char* who, const void* x, int E, int R) {
    CHECK_ARG(E >= 1 && E <= CORR_MAX_EVENTS, "%s: E = %d outside 1 .. %d", who, E, CORR_MAX_EVENTS);
    CHECK_ARG(R >= 1 && R <= CORR_MAX_COLUMNS, "%s: R = %d outside 1 .. %d", who, R, CORR_MAX_COLUMNS);
    return pxd_check_needed(who, "x", 4, {x});
}

extern "C" int ieagan_pxd_region_counts(const int* index, const int* digit_total, int N, int H, int W, int n_sensors, int RU, int RV,
                                        long capacity, int* x, unsigned long long* overflow, void* stream) {
    const char* who = "pxd_region_counts";
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pxd_check_geometry(who, N, H, W, true)) return rc;
    if (int rc = pxd_check_whole_events(who, N, n_sensors)) return rc;
    CHECK_ARG(RU >= 1 && RU <= H && RV >= 1 && RV <= W, "%s: regions %d x %d outside 1 .. %d x 1 .. %d", who, RU, RV, H, W);
    CHECK_ARG((long)n_sensors * RU * RV <= CORR_MAX_COLUMNS, "%s: R = %d * %d * %d columns exceed %d", who, n_sensors, RU, RV, CORR_MAX_COLUMNS);
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    if (int rc = pxd_check_totals(who, "digit_total", {digit_total})) return rc;
    if (int rc = pxd_check_arrays(who, "index", "capacity", capacity, {index})) return rc;
    if (int rc = pxd_check_aligned(who, "index", 4, {index})) return rc;
    if (int rc = pxd_check_needed(who, "x", 4, {x})) return rc;
    if (int rc = pxd_check_needed(who, "overflow", 8, {overflow})) return rc;
    const int cap = pxd_cap(capacity);
    const int B = cl_blocks(cap), chunk = cl_chunk(cap, B);
    const long cells = (long)(N / n_sensors) * n_sensors * RU * RV;
    // the digits read depend on the data and are not counted
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_corr_zero_kernel, dim3(cl_blocks(cells)), dim3(PXD_THREADS), 0, st, x, cells);
    CHECK_LAUNCH("pxd_region_counts zero");
    hipLaunchKernelGGL(pxd_region_counts_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, digit_total, cap, chunk, (long)N * H * W, H * W, H, W,
                       n_sensors, RU, RV, x, (u64*)overflow);
    CHECK_LAUNCH("pxd_region_counts");
    return 0;
}

extern "C" int ieagan_pxd_gram(const int* x, int E, int R, long long* gram, long long* sum, void* stream) {
    const char* who = "pxd_gram";
    hipStream_t st = (hipStream_t)stream;
    if (int rc = corr_check_table(who, x, E, R)) return rc;
    if (int rc = pxd_check_needed(who, "gram / sum", 8, {gram, sum})) return rc;
    const int rows = GR_ROWS * PXD_WAVES;
    ProfScope prof(who, 2.0 * E * R * R, 4.0 * E * R + 16.0 * R * R, st);
    hipLaunchKernelGGL(pxd_gram_kernel, dim3((R + 63) / 64, (R + rows - 1) / rows), dim3(PXD_THREADS), 0, st, x, E, R, (i64*)gram, (i64*)sum);
    CHECK_LAUNCH("pxd_gram");
    return 0;
}

extern "C" int ieagan_pxd_ranks(const int* x, int E, int R, int* rank2, void* stream) {
    const char* who = "pxd_ranks";
    hipStream_t st = (hipStream_t)stream;
    if (int rc = corr_check_table(who, x, E, R)) return rc;
    if (int rc = pxd_check_needed(who, "rank2", 4, {rank2})) return rc;
    CHECK_ARG(rank2 != x, "%s: rank2 must not be x", who);
    const int rows = RK_OWN * PXD_WAVES;
    ProfScope prof(who, 2.0 * E * E * R, 8.0 * E * R, st);
    hipLaunchKernelGGL(pxd_ranks_kernel, dim3((R + 63) / 64, (E + rows - 1) / rows), dim3(PXD_THREADS), 0, st, x, E, R, rank2);
    CHECK_LAUNCH("pxd_ranks");
    return 0;
}
