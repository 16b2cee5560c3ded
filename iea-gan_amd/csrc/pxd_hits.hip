// PXD hits on top of pxd_reco.hip: the position of every accepted cluster in the local frame of its sensor, in integer geometry units, with
// the head-tail estimate for wide clusters.  Input is one ieagan_pxd_digits + ieagan_pxd_clusters + ieagan_pxd_cluster_positions result and
// the pitch tables of a pxd.PXDGeometry; every array stays in HBM.
//
//   tables    per sensor type g and axis: pitch[g][k] of cell k and its doubled, centred centre x2[g][k] = 2 * sum(pitch[:k]) + pitch[k] -
//             sum(pitch) (int32; rows use the u tables, columns the v tables).  Type of a cluster: kind[(first / HW) % n_sensors].
//   moments   pu[j] = sum q_k * u_x2[r_k],  pv[j] = sum q_k * v_x2[c_k] over the digits of cluster j, 64-bit signed
//   extent    rows lo = row of `first` (digits ascend in raster order) .. lo + size_u - 1; columns v_start = min c_k .. v_start + size_v - 1
//   edges     qh = summed charge of the digits in the first row (column) of the extent, qt in the last
//   position  along one axis with s cells lo .. hi, Q = ccharge, m the moment, p the pitch:
//               s < head_tail (or head_tail == 0):  num = m,  den = 2 Q                                          centre of gravity
//               else  D = Q - qh - qt:  num = (x2[lo] + x2[hi]) D + 2 (qt p[hi] - qh p[lo]) (s - 2),  den = 4 D     head-tail
//             clamp in integers: 2 num < den (x2[lo] - p[lo]) -> num = x2[lo] - p[lo], den = 2;  2 num > den (x2[hi] + p[hi]) likewise
//             position = (float)((double)num / (double)den), geometry units.  |num| < 2^53: both conversions are exact and the one
//             division is IEEE, so the result is the correctly rounded quotient and there is nothing for -ffp-contract to contract.
//
// Four launches, the launch shape depends on the capacity alone (every total is read on the device), kernel boundaries are the only global
// barriers:
//   init      wave g owns the clusters [g * chunk, (g + 1) * chunk): moments and edge charges = 0, v_start = INT_MAX
//   moments   wave g owns the digits [g * chunk, (g + 1) * chunk): a segmented sum / minimum over each run of equal label (shuffles), then one
//             integer atomic per run and quantity: pu, pv, the u edge charges (their rows are known from `first` and size_u), min column
//   edges     the same walk once more, now that v_start is final: the v edge charges
//   hits      thread a owns accepted cluster a: the rule above, twice
// Sums are integer adds and minima, which commute exactly; no float is summed: two calls on the same input write the same bytes.
#include "common.h"
#include "pxd_common.h"

__global__ __launch_bounds__(PXD_THREADS) void pxd_hits_init_kernel(const int* __restrict__ ctotal, int cap, int chunk, i64* __restrict__ pu,
                                                                    i64* __restrict__ pv, int* __restrict__ v_start, int* __restrict__ qh_u,
                                                                    int* __restrict__ qt_u, int* __restrict__ qh_v, int* __restrict__ qt_v) {
    const PxdWaveRange w(pxd_total(ctotal, cap), chunk);
    for (long jj = w.k0 + w.lane; jj < w.k1; jj += 64) {
        const int j = (int)jj;
        pu[j] = 0ll;
        pv[j] = 0ll;
        v_start[j] = INT_MAX;
        qh_u[j] = qt_u[j] = qh_v[j] = qt_v[j] = 0;
    }
}

// The digit k of lane `lane` in the step at kb, or lab = -1: no digit, a label that is no row of the table, or a position outside the batch.
__device__ __forceinline__ int hits_digit(const int* __restrict__ index, const int* __restrict__ label, long kk, long k1, int T, long NHW,
                                          int HW, int W, int& r, int& c, int& idx) {
    const int lab = pxd_digit_label(label, kk, k1, T);
    if (lab < 0) return -1;
    idx = index[kk];
    if (idx < 0 || (long)idx >= NHW) return -1;
    pxd_row_col(idx, HW, W, r, c);
    return lab;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_hits_moments_kernel(
    const int* __restrict__ index, const uint8_t* __restrict__ charge, const int* __restrict__ label, const int* __restrict__ dtotal,
    const int* __restrict__ first, const int* __restrict__ size_u, const int* __restrict__ ctotal, const int* __restrict__ u_x2,
    const int* __restrict__ v_x2, const int* __restrict__ kind, int cap, int chunk, int N, int H, int W, int n_sensors, int K,
    i64* __restrict__ pu, i64* __restrict__ pv, int* __restrict__ v_start, int* __restrict__ qh_u, int* __restrict__ qt_u) {
    const PxdWaveRange w(pxd_total(dtotal, cap), chunk);
    const int T = pxd_total(ctotal, cap), lane = w.lane;
    const int HW = H * W;
    for (long kb = w.k0; kb < w.k1; kb += 64) {
        int r = 0, c = INT_MAX, idx = 0;
        const int lab = hits_digit(index, label, kb + lane, w.k1, T, (long)N * HW, HW, W, r, c, idx);
        i64 mu = 0ll, mv = 0ll;
        int head = 0, tail = 0;
        if (lab >= 0) {
            const int q = (int)charge[kb + lane];
            const int t = kind[(idx / HW) % n_sensors];
            if ((unsigned)t < (unsigned)K) {            // the tables are checked on the host; a type outside them adds nothing
                mu = (i64)q * (i64)u_x2[(long)t * H + r];
                mv = (i64)q * (i64)v_x2[(long)t * W + c];
            }
            const int lo = (first[lab] % HW) / W;
            head = r == lo ? q : 0;
            tail = r == lo + size_u[lab] - 1 ? q : 0;
        }
        const PxdRun run = pxd_run(lab, lane);
        mu = pxd_run_sum(mu, lane, run.end);
        mv = pxd_run_sum(mv, lane, run.end);
        head = pxd_run_sum(head, lane, run.end);
        tail = pxd_run_sum(tail, lane, run.end);
        c = pxd_run_reduce(c, lane, run.end, [](int a, int b) { return a < b ? a : b; });
        if (run.head && lab >= 0) {
            if (mu) atomicAdd((u64*)pu + lab, (u64)mu);         // two's complement: the unsigned add is the signed one
            if (mv) atomicAdd((u64*)pv + lab, (u64)mv);
            if (head) atomicAdd(qh_u + lab, head);
            if (tail) atomicAdd(qt_u + lab, tail);
            atomicMin(v_start + lab, c);
        }
    }
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_hits_edges_kernel(const int* __restrict__ index, const uint8_t* __restrict__ charge,
                                                                     const int* __restrict__ label, const int* __restrict__ dtotal,
                                                                     const int* __restrict__ size_v, const int* __restrict__ ctotal,
                                                                     const int* __restrict__ v_start, int cap, int chunk, int N, int H, int W,
                                                                     int* __restrict__ qh_v, int* __restrict__ qt_v) {
    const PxdWaveRange w(pxd_total(dtotal, cap), chunk);
    const int T = pxd_total(ctotal, cap), lane = w.lane;
    const int HW = H * W;
    for (long kb = w.k0; kb < w.k1; kb += 64) {
        int r = 0, c = 0, idx = 0;
        const int lab = hits_digit(index, label, kb + lane, w.k1, T, (long)N * HW, HW, W, r, c, idx);
        int head = 0, tail = 0;
        if (lab >= 0) {
            const int q = (int)charge[kb + lane], lo = v_start[lab];
            head = c == lo ? q : 0;
            tail = c == lo + size_v[lab] - 1 ? q : 0;
        }
        const PxdRun run = pxd_run(lab, lane);
        head = pxd_run_sum(head, lane, run.end);
        tail = pxd_run_sum(tail, lane, run.end);
        if (run.head && lab >= 0) {
            if (head) atomicAdd(qh_v + lab, head);
            if (tail) atomicAdd(qt_v + lab, tail);
        }
    }
}

// The position rule along one axis of `len` cells: cells lo .. lo + s - 1, total charge Q, moment m, edge charges qh / qt, the type's tables
// x2 / p.  Returns the position; sets `ht` when head-tail was used and `cl` when the result was clamped to the cluster's extent.
__device__ __forceinline__ float hits_axis(i64 m, i64 Q, int lo, int s, i64 qh, i64 qt, const int* __restrict__ x2, const int* __restrict__ p,
                                           int len, int head_tail, bool& ht, bool& cl) {
    ht = cl = false;
    if (lo < 0 || s < 1 || (long)lo + s > len) return 0.0f;          // no extent of this sensor: not a row of a consistent table
    const int hi = lo + s - 1;
    const i64 xlo = x2[lo], xhi = x2[hi], plo = p[lo], phi = p[hi];
    i64 num = m, den = 2 * Q;
    if (head_tail != 0 && s >= head_tail) {
        const i64 D = Q - qh - qt;
        num = (xlo + xhi) * D + 2 * (qt * phi - qh * plo) * (i64)(s - 2);
        den = 4 * D;
        ht = true;
    }
    if (2 * num < den * (xlo - plo)) {
        num = xlo - plo;
        den = 2;
        cl = true;
    } else if (2 * num > den * (xhi + phi)) {
        num = xhi + phi;
        den = 2;
        cl = true;
    }
    return (float)((double)num / (double)den);
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_hits_kernel(
    const int* __restrict__ cluster, const int* __restrict__ atotal, const int* __restrict__ first, const int* __restrict__ ccharge,
    const int* __restrict__ size_u, const int* __restrict__ size_v, const int* __restrict__ ctotal, const int* __restrict__ u_x2,
    const int* __restrict__ u_pitch, const int* __restrict__ v_x2, const int* __restrict__ v_pitch, const int* __restrict__ kind, int cap, int H,
    int W, int n_sensors, int K, int head_tail, const i64* __restrict__ pu, const i64* __restrict__ pv, const int* __restrict__ v_start,
    const int* __restrict__ qh_u, const int* __restrict__ qt_u, const int* __restrict__ qh_v, const int* __restrict__ qt_v, float* __restrict__ u,
    float* __restrict__ v, uint8_t* __restrict__ flags) {
    const int T = pxd_total(ctotal, cap);
    const int A = pxd_total(atotal, T);
    const int HW = H * W;
    for (int a = pxd_grid_thread(); a < A; a += pxd_grid_threads()) {
        const int j = cluster[a];
        float pos_u = 0.0f, pos_v = 0.0f;
        bool ht_u = false, ht_v = false, cl_u = false, cl_v = false;
        const int f = (unsigned)j < (unsigned)T ? first[j] : -1;
        const int t = f >= 0 ? kind[(f / HW) % n_sensors] : -1;
        if ((unsigned)t < (unsigned)K) {            // else: not a row of the table or not a type of the geometry, position 0 and no flag
            const i64 Q = ccharge[j];
            pos_u = hits_axis(pu[j], Q, (f % HW) / W, size_u[j], qh_u[j], qt_u[j], u_x2 + (long)t * H, u_pitch + (long)t * H, H, head_tail, ht_u,
                              cl_u);
            pos_v = hits_axis(pv[j], Q, v_start[j], size_v[j], qh_v[j], qt_v[j], v_x2 + (long)t * W, v_pitch + (long)t * W, W, head_tail, ht_v,
                              cl_v);
        }
        u[a] = pos_u;
        v[a] = pos_v;
        flags[a] = (uint8_t)((int)ht_u | (int)ht_v << 1 | (int)cl_u << 2 | (int)cl_v << 3);
    }
}

extern "C" long ieagan_pxd_hits_scratch(int N, int H, int W, long capacity) {
    (void)N, (void)H, (void)W, (void)capacity;
    return 0;           // every intermediate (moments, v_start, edge charges) is an output of the call
}

extern "C" int ieagan_pxd_hits(const int* index, const unsigned char* charge, const int* label, const int* digit_total, const int* first,
                               const int* ccharge, const int* size_u, const int* size_v, const int* cluster_total, const int* cluster,
                               const int* accepted_total, const int* u_x2, const int* u_pitch, const int* v_x2, const int* v_pitch,
                               const int* kind, int N, int H, int W, int n_sensors, int K, long capacity, int head_tail, long long* pu,
                               long long* pv, int* v_start, int* qh_u, int* qt_u, int* qh_v, int* qt_v, float* u, float* v,
                               unsigned char* flags, int* scratch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    (void)scratch;
    const char* who = "pxd_hits";
    if (int rc = pxd_check_geometry(who, N, H, W, true)) return rc;
    if (int rc = pxd_check_cluster_charge(who, H, W)) return rc;
    if (int rc = pxd_check_whole_events(who, N, n_sensors)) return rc;
    CHECK_ARG(K >= 1, "%s: K = %d sensor types", who, K);
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    CHECK_ARG(head_tail == 0 || head_tail >= 3, "%s: head_tail = %d is neither 0 (never) nor >= 3", who, head_tail);
    if (int rc = pxd_check_totals(who, "digit_total / cluster_total / accepted_total", {digit_total, cluster_total, accepted_total})) return rc;
    // the content of the tables (pitch 1 .. 4095, length < 2^20, kind < K) is checked on the host by pxd.PXDGeometry: the launcher cannot see
    // device memory.  The kernels never index a table with a type outside 0 .. K-1.
    if (int rc = pxd_check_needed(who, "a geometry table", 4, {u_x2, u_pitch, v_x2, v_pitch, kind})) return rc;
    if (int rc = pxd_check_arrays(who, "index / charge / label", "capacity", capacity, {index, charge, label})) return rc;
    if (int rc = pxd_check_arrays(who, "a cluster table or the accepted list", "capacity", capacity, {first, ccharge, size_u, size_v, cluster}))
        return rc;
    if (int rc = pxd_check_arrays(who, "an output array", "capacity", capacity, {pu, pv, v_start, qh_u, qt_u, qh_v, qt_v, u, v, flags})) return rc;
    if (int rc = pxd_check_aligned(who, "an int32 / fp32 array", 4,
                                   {index, label, first, ccharge, size_u, size_v, cluster, v_start, qh_u, qt_u, qh_v, qt_v, u, v}))
        return rc;
    if (int rc = pxd_check_aligned(who, "pu / pv", 8, {pu, pv})) return rc;
    const int cap = pxd_cap(capacity);
    const int B = cl_blocks(cap), chunk = cl_chunk(cap, B);
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_hits_init_kernel, dim3(B), dim3(PXD_THREADS), 0, st, cluster_total, cap, chunk, (i64*)pu, (i64*)pv, v_start, qh_u, qt_u,
                       qh_v, qt_v);
    CHECK_LAUNCH("pxd_hits init");
    hipLaunchKernelGGL(pxd_hits_moments_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, (const uint8_t*)charge, label, digit_total, first, size_u,
                       cluster_total, u_x2, v_x2, kind, cap, chunk, N, H, W, n_sensors, K, (i64*)pu, (i64*)pv, v_start, qh_u, qt_u);
    CHECK_LAUNCH("pxd_hits moments");
    hipLaunchKernelGGL(pxd_hits_edges_kernel, dim3(B), dim3(PXD_THREADS), 0, st, index, (const uint8_t*)charge, label, digit_total, size_v,
                       cluster_total, (const int*)v_start, cap, chunk, N, H, W, qh_v, qt_v);
    CHECK_LAUNCH("pxd_hits edges");
    hipLaunchKernelGGL(pxd_hits_kernel, dim3(B), dim3(PXD_THREADS), 0, st, cluster, accepted_total, first, ccharge, size_u, size_v, cluster_total,
                       u_x2, u_pitch, v_x2, v_pitch, kind, cap, H, W, n_sensors, K, head_tail, (const i64*)pu, (const i64*)pv,
                       (const int*)v_start, (const int*)qh_u, (const int*)qt_u, (const int*)qh_v, (const int*)qt_v, u, v, (uint8_t*)flags);
    CHECK_LAUNCH("pxd_hits");
    return 0;
}
