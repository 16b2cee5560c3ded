// Signal-hit matching under background: what became of every signal hit once background was laid over it.  Input are two ieagan_pxd_hits
// results over batches of the same [N, H, W] -- `s`, the signal, and `m`, the mixed events (in the intended use the signal with background
// laid over it, reconstructed) --, each with its own capacity; every array stays in HBM.  The join is pixel identity: a signal digit is FOUND
// when its flat index occurs in the mixed digit list, L is then the mixed label of that digit.
//
//   per signal cluster j   found = its found digits; lo / hi = smallest / largest L over them, -1 / -1 when found == 0; lo is the match
//   per mixed cluster k    signal_size / signal_charge = number and summed SIGNAL charge of the signal digits found in it (<= the mixed
//                          charge: min(qa + qb, 255) >= qa); n_signal = the signal clusters with lo == k
//   per signal hit h       (accepted signal cluster j = s_cluster[h]) mixed_hit = row of the mixed hit whose cluster is lo[j], or -1;
//                          flags: bit 0 MATCHED  found == size, lo == hi >= 0 and that mixed cluster is itself a hit
//                                 bit 1 CHANGED  MATCHED and the mixed cluster's size or charge differs from the signal's
//                                 bit 2 SHARED   n_signal[lo] >= 2
//                          du / dv = (float)((double)m_u[mixed_hit] - (double)s_u[h]), 0 when not MATCHED: one IEEE subtraction of two
//                          exactly converted values (nothing for -ffp-contract to contract), the host restatement gives the same bits
//
// Four launches, the launch shapes depend on the two capacities alone (every total is read on the device), kernel boundaries are the only
// global barriers:
//   init      per signal cluster found = 0, lo = INT_MAX, hi = -1; per mixed cluster signal_size = signal_charge = n_signal = 0 and the
//             inverse map inv[k] = -1 (mixed cluster -> mixed hit row, in scratch)
//   digits    one lane per signal digit below min(total, capacity): cl_lower_bound of its index in the mixed index list (about
//             log2(digits) = 18 dependent loads that hit L2; one wave per 64 digits of capacity, so the searches of the whole list are in
//             flight side by side), equality = found.  Then a segmented reduction over each run of equal signal label (shuffles) and one
//             atomicAdd(found), atomicMin(lo), atomicMax(hi) per run; the same over the runs of equal L for signal_size / signal_charge.
//   clusters  thread j: lo / hi of a signal cluster without a found digit become -1, the others add 1 to n_signal[lo]; thread a: mixed hit a
//             writes its row into inv[m_cluster[a]]
//   hits      thread h owns signal hit h: the rule above
// Sums are integer adds, minima and maxima, which commute exactly; no float is summed: two calls on the same input write the same bytes.
//
// Memory safety does not depend on the content of the inputs.  Every total is clipped to [0, capacity] of its side before it bounds a loop;
// the search probes m_index[mid] with 0 <= mid < Mm <= m_capacity only, whatever the list holds (an unsorted list gives a wrong position,
// still inside); a signal label is compared with the signal cluster total and L with the mixed cluster total before either indexes a
// table; lo / hi are written by this call alone, from range-checked L, and are checked again where they index; a cluster row of an accepted
// list and a hit row of the inverse map are checked against their totals before use.  Inputs that break their contract give wrong numbers,
// never a wrong address.
//
// ieagan_pxd_match_stats adds one such result into int64 tables per sensor (of the signal hit): five counters, two residual histograms and
// a purity histogram, with 64-bit integer atomics; see the bin rules at the kernel.
#include "common.h"
#include "pxd_common.h"

#define MT_MAX_BLOCKS 4096
#define MT_MATCHED 1
#define MT_CHANGED 2
#define MT_SHARED 4
#define MT_RES_BINS 64
#define MT_PURITY_BINS 32
#define MT_COLUMNS (5 + 2 * MT_RES_BINS + MT_PURITY_BINS)          // 165 int64 per sensor

// One wave per 64 entries of the capacity up to MT_MAX_BLOCKS workgroups (the reasoning of ov_blocks in pxd_overlay.hip: a production event
// is one step per wave, the dependent loads of all searches run side by side).
static inline int mt_blocks(long cap) { return pxd_blocks(cap, PXD_THREADS, MT_MAX_BLOCKS); }

__global__ __launch_bounds__(PXD_THREADS) void pxd_match_init_kernel(const int* __restrict__ s_ctotal, int s_cap, const int* __restrict__ m_ctotal,
                                                                     int m_cap, int* __restrict__ found, int* __restrict__ lo,
                                                                     int* __restrict__ hi, int* __restrict__ signal_size,
                                                                     int* __restrict__ signal_charge, int* __restrict__ n_signal,
                                                                     int* __restrict__ inv) {
    const int Ts = pxd_total(s_ctotal, s_cap), Tm = pxd_total(m_ctotal, m_cap);
    const long t0 = pxd_grid_thread(), step = pxd_grid_threads();
    for (long j = t0; j < Ts; j += step) {
        found[j] = 0;
        lo[j] = INT_MAX;
        hi[j] = -1;
    }
    for (long k = t0; k < Tm; k += step) {
        signal_size[k] = signal_charge[k] = n_signal[k] = 0;
        inv[k] = -1;
    }
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_match_digits_kernel(
    const int* __restrict__ s_index, const uint8_t* __restrict__ s_charge, const int* __restrict__ s_label, const int* __restrict__ s_dtotal,
    const int* __restrict__ s_ctotal, int s_cap, const int* __restrict__ m_index, const int* __restrict__ m_label,
    const int* __restrict__ m_dtotal, const int* __restrict__ m_ctotal, int m_cap, int chunk, int* __restrict__ found, int* __restrict__ lo,
    int* __restrict__ hi, int* __restrict__ signal_size, int* __restrict__ signal_charge) {
    const PxdWaveRange w(pxd_total(s_dtotal, s_cap), chunk);
    const int lane = w.lane, Mm = pxd_total(m_dtotal, m_cap);
    const int Ts = pxd_total(s_ctotal, s_cap), Tm = pxd_total(m_ctotal, m_cap);
    for (long kb = w.k0; kb < w.k1; kb += 64) {
        const long kk = kb + lane;
        const int lab = pxd_digit_label(s_label, kk, w.k1, Ts);
        int L = -1, q = 0;
        if (lab >= 0) {
            const int idx = s_index[kk];
            const int p = cl_lower_bound(m_index, Mm, idx);     // 0 <= p <= Mm, every probe below Mm
            if (p < Mm && m_index[p] == idx) {
                L = m_label[p];
                if ((unsigned)L >= (unsigned)Tm) L = -1;        // not a row of the mixed table: counts as not found
            }
            if (L >= 0) q = (int)s_charge[kk];
        }
        // the runs of equal signal label: found, lo, hi
        const PxdRun rs = pxd_run(lab, lane);
        const int n = pxd_run_sum(L >= 0 ? 1 : 0, lane, rs.end);
        const int l_min = pxd_run_reduce(L >= 0 ? L : INT_MAX, lane, rs.end, [](int a, int b) { return a < b ? a : b; });
        const int l_max = pxd_run_reduce(L, lane, rs.end, [](int a, int b) { return a > b ? a : b; });
        if (rs.head && lab >= 0 && n > 0) {
            atomicAdd(found + lab, n);
            atomicMin(lo + lab, l_min);
            atomicMax(hi + lab, l_max);
        }
        // the runs of equal mixed label (-1: not found): the signal digits and the signal charge inside a mixed cluster
        const PxdRun rm = pxd_run(L, lane);
        const int cnt = pxd_run_sum(L >= 0 ? 1 : 0, lane, rm.end);
        const int qsum = pxd_run_sum(q, lane, rm.end);
        if (rm.head && L >= 0) {
            atomicAdd(signal_size + L, cnt);
            atomicAdd(signal_charge + L, qsum);
        }
    }
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_match_clusters_kernel(const int* __restrict__ s_ctotal, int s_cap,
                                                                         const int* __restrict__ m_ctotal, int m_cap,
                                                                         const int* __restrict__ m_cluster, const int* __restrict__ m_atotal,
                                                                         const int* __restrict__ found, int* __restrict__ lo,
                                                                         int* __restrict__ hi, int* __restrict__ n_signal,
                                                                         int* __restrict__ inv) {
    const int Ts = pxd_total(s_ctotal, s_cap), Tm = pxd_total(m_ctotal, m_cap);
    const int Am = pxd_total(m_atotal, Tm);
    const long t0 = pxd_grid_thread(), step = pxd_grid_threads();
    for (long j = t0; j < Ts; j += step) {
        const int l = lo[j];
        if (found[j] <= 0 || (unsigned)l >= (unsigned)Tm) lo[j] = hi[j] = -1;
        else atomicAdd(n_signal + l, 1);
    }
    for (long a = t0; a < Am; a += step) {
        const int k = m_cluster[a];
        if ((unsigned)k < (unsigned)Tm) inv[k] = (int)a;         // the accepted list names a cluster once: one writer per row
    }
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_match_hits_kernel(
    const int* __restrict__ s_cluster, const int* __restrict__ s_atotal, const int* __restrict__ s_size, const int* __restrict__ s_ccharge,
    const int* __restrict__ s_ctotal, int s_cap, const float* __restrict__ s_u, const float* __restrict__ s_v, const int* __restrict__ m_size,
    const int* __restrict__ m_ccharge, const int* __restrict__ m_ctotal, const int* __restrict__ m_atotal, int m_cap,
    const float* __restrict__ m_u, const float* __restrict__ m_v, const int* __restrict__ found, const int* __restrict__ lo,
    const int* __restrict__ hi, const int* __restrict__ n_signal, const int* __restrict__ inv, int* __restrict__ mixed_hit,
    uint8_t* __restrict__ flags, float* __restrict__ du, float* __restrict__ dv) {
    const int Ts = pxd_total(s_ctotal, s_cap), Tm = pxd_total(m_ctotal, m_cap);
    const int As = pxd_total(s_atotal, Ts), Am = pxd_total(m_atotal, Tm);
    const long t0 = pxd_grid_thread(), step = pxd_grid_threads();
    for (long h = t0; h < As; h += step) {
        const int j = s_cluster[h];
        int mh = -1, fl = 0;
        float ru = 0.0f, rv = 0.0f;
        const int l = (unsigned)j < (unsigned)Ts ? lo[j] : -1;
        if ((unsigned)l < (unsigned)Tm) {
            mh = inv[l];
            if ((unsigned)mh >= (unsigned)Am) mh = -1;
            const int size = s_size[j];
            if (found[j] == size && hi[j] == l && mh >= 0) {
                fl |= MT_MATCHED;
                if (m_size[l] != size || m_ccharge[l] != s_ccharge[j]) fl |= MT_CHANGED;
                ru = (float)((double)m_u[mh] - (double)s_u[h]);
                rv = (float)((double)m_v[mh] - (double)s_v[h]);
            }
            if (n_signal[l] >= 2) fl |= MT_SHARED;
        }
        mixed_hit[h] = mh;
        flags[h] = (uint8_t)fl;
        du[h] = ru;
        dv[h] = rv;
    }
}

// bin = clamp(floor(r / w) + 32, 0, 63): one IEEE division and a floor in float64, the clamp before the conversion (a NaN goes to bin 0).
__device__ __forceinline__ int mt_residual_bin(double r, double w) {
    const double b = floor(r / w) + (double)(MT_RES_BINS / 2);
    return b >= (double)(MT_RES_BINS - 1) ? MT_RES_BINS - 1 : b > 0.0 ? (int)b : 0;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_match_stats_kernel(
    const int* __restrict__ s_cluster, const int* __restrict__ s_atotal, const int* __restrict__ s_first, const int* __restrict__ s_ctotal,
    const int* __restrict__ s_dtotal, int s_cap, const float* __restrict__ s_u, const float* __restrict__ s_v,
    const int* __restrict__ m_ccharge, const int* __restrict__ m_ctotal, const int* __restrict__ m_atotal, const int* __restrict__ m_dtotal,
    int m_cap, const float* __restrict__ m_u, const float* __restrict__ m_v, const int* __restrict__ lo, const int* __restrict__ signal_charge,
    const int* __restrict__ mixed_hit, const uint8_t* __restrict__ flags, int N, int H, int W, int n_sensors, double w, u64* __restrict__ table,
    u64* __restrict__ overflow) {
    const long t0 = pxd_grid_thread(), step = pxd_grid_threads();
    if (t0 == 0 && (s_dtotal[0] > s_cap || m_dtotal[0] > m_cap)) atomicAdd(overflow, 1ull);
    const int Ts = pxd_total(s_ctotal, s_cap), Tm = pxd_total(m_ctotal, m_cap);
    const int As = pxd_total(s_atotal, Ts), Am = pxd_total(m_atotal, Tm);
    const int HW = H * W;
    for (long h = t0; h < As; h += step) {
        const int j = s_cluster[h];
        if ((unsigned)j >= (unsigned)Ts) continue;          // not a row of the table
        const int f = s_first[j];
        if (f < 0 || (long)f >= (long)N * HW) continue;
        u64* __restrict__ row = table + (long)((f / HW) % n_sensors) * MT_COLUMNS;
        const int fl = (int)flags[h];
        const bool matched = fl & MT_MATCHED;
        atomicAdd(row + 0, 1ull);
        atomicAdd(row + (matched ? 1 : 4), 1ull);
        if (!matched) continue;
        if (fl & MT_SHARED) atomicAdd(row + 3, 1ull);
        const int mh = mixed_hit[h];
        if ((fl & MT_CHANGED) && (unsigned)mh < (unsigned)Am) {
            atomicAdd(row + 2, 1ull);
            atomicAdd(row + 5 + mt_residual_bin((double)m_u[mh] - (double)s_u[h], w), 1ull);
            atomicAdd(row + 5 + MT_RES_BINS + mt_residual_bin((double)m_v[mh] - (double)s_v[h], w), 1ull);
        }
        const int l = lo[j];
        if ((unsigned)l >= (unsigned)Tm) continue;
        const i64 qm = m_ccharge[l], qs = signal_charge[l];
        if (qm <= 0 || qs < 0) continue;
        const i64 b = (i64)MT_PURITY_BINS * qs / qm;
        atomicAdd(row + 5 + 2 * MT_RES_BINS + (int)(b < MT_PURITY_BINS - 1 ? b : MT_PURITY_BINS - 1), 1ull);
    }
}

extern "C" long ieagan_pxd_match_scratch(int N, int H, int W, long capacity) {
    if (N <= 0 || H <= 0 || W <= 0 || capacity < 0) return 0;
    return (long)pxd_cap(capacity);             // the inverse map: one word per mixed cluster
}

// One side: `names` are its capacity, totals, arrays and 4-byte arrays in the error texts.
static int mt_check_side(const char* who, const char* const names[4], long capacity, PxdPtrs totals, PxdPtrs i32) {
    if (int rc = pxd_check_capacity(who, names[0], capacity)) return rc;
    if (int rc = pxd_check_totals(who, names[1], totals)) return rc;
    if (int rc = pxd_check_arrays(who, names[2], "capacity", capacity, i32)) return rc;
    return pxd_check_aligned(who, names[3], 4, i32);
}
static const char* const MT_SIGNAL[4] = {"signal_capacity", "a total of the signal side", "an array of the signal side",
                                         "an int32 / fp32 array of the signal side"};
static const char* const MT_MIXED[4] = {"mixed_capacity", "a total of the mixed side", "an array of the mixed side",
                                        "an int32 / fp32 array of the mixed side"};

extern "C" int ieagan_pxd_match(const int* s_index, const unsigned char* s_charge, const int* s_label, const int* s_digit_total,
                                const int* s_size, const int* s_ccharge, const int* s_cluster_total, const int* s_cluster,
                                const int* s_accepted_total, const float* s_u, const float* s_v, const int* m_index, const int* m_label,
                                const int* m_digit_total, const int* m_size, const int* m_ccharge, const int* m_cluster_total,
                                const int* m_cluster, const int* m_accepted_total, const float* m_u, const float* m_v, int N, int H, int W,
                                long s_capacity, long m_capacity, int* found, int* lo, int* hi, int* signal_size, int* signal_charge,
                                int* n_signal, int* mixed_hit, unsigned char* flags, float* du, float* dv, int* scratch, void* stream) {
    const char* who = "pxd_match";
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pxd_check_geometry(who, N, H, W, true)) return rc;
    if (int rc = mt_check_side(who, MT_SIGNAL, s_capacity, {s_digit_total, s_cluster_total, s_accepted_total},
                               {s_index, s_label, s_size, s_ccharge, s_cluster, s_u, s_v, found, lo, hi, mixed_hit, du, dv}))
        return rc;
    if (int rc = pxd_check_arrays(who, "s_charge / flags", "capacity", s_capacity, {s_charge, flags})) return rc;
    if (int rc = mt_check_side(who, MT_MIXED, m_capacity, {m_digit_total, m_cluster_total, m_accepted_total},
                               {m_index, m_label, m_size, m_ccharge, m_cluster, m_u, m_v, signal_size, signal_charge, n_signal}))
        return rc;
    CHECK_ARG(pxd_all_aligned({scratch}, 4) && (m_capacity == 0 || scratch != nullptr),
              "%s: scratch (ieagan_pxd_match_scratch int32 words) is NULL or misaligned", who);
    const int s_cap = pxd_cap(s_capacity), m_cap = pxd_cap(m_capacity);
    const int B = mt_blocks(s_cap > m_cap ? s_cap : m_cap), chunk = cl_chunk(s_cap, B);
    int* inv = scratch;
    // the digits read depend on the data and are not counted
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_match_init_kernel, dim3(B), dim3(PXD_THREADS), 0, st, s_cluster_total, s_cap, m_cluster_total, m_cap, found, lo, hi,
                       signal_size, signal_charge, n_signal, inv);
    CHECK_LAUNCH("pxd_match init");
    hipLaunchKernelGGL(pxd_match_digits_kernel, dim3(B), dim3(PXD_THREADS), 0, st, s_index, (const uint8_t*)s_charge, s_label, s_digit_total,
                       s_cluster_total, s_cap, m_index, m_label, m_digit_total, m_cluster_total, m_cap, chunk, found, lo, hi, signal_size,
                       signal_charge);
    CHECK_LAUNCH("pxd_match digits");
    hipLaunchKernelGGL(pxd_match_clusters_kernel, dim3(B), dim3(PXD_THREADS), 0, st, s_cluster_total, s_cap, m_cluster_total, m_cap, m_cluster,
                       m_accepted_total, (const int*)found, lo, hi, n_signal, inv);
    CHECK_LAUNCH("pxd_match clusters");
    hipLaunchKernelGGL(pxd_match_hits_kernel, dim3(B), dim3(PXD_THREADS), 0, st, s_cluster, s_accepted_total, s_size, s_ccharge, s_cluster_total,
                       s_cap, s_u, s_v, m_size, m_ccharge, m_cluster_total, m_accepted_total, m_cap, m_u, m_v, (const int*)found, (const int*)lo,
                       (const int*)hi, (const int*)n_signal, (const int*)inv, mixed_hit, (uint8_t*)flags, du, dv);
    CHECK_LAUNCH("pxd_match hits");
    return 0;
}

extern "C" int ieagan_pxd_match_stats(const int* s_cluster, const int* s_accepted_total, const int* s_first, const int* s_cluster_total,
                                      const int* s_digit_total, const float* s_u, const float* s_v, const int* m_ccharge,
                                      const int* m_cluster_total, const int* m_accepted_total, const int* m_digit_total, const float* m_u,
                                      const float* m_v, const int* lo, const int* signal_charge, const int* mixed_hit,
                                      const unsigned char* flags, int N, int H, int W, int n_sensors, long s_capacity, long m_capacity,
                                      int residual_bin, unsigned long long* table, unsigned long long* overflow, void* stream) {
    const char* who = "pxd_match_stats";
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pxd_check_geometry(who, N, H, W, true)) return rc;
    if (int rc = pxd_check_whole_events(who, N, n_sensors)) return rc;
    CHECK_ARG(residual_bin >= 1, "%s: residual_bin = %d is not >= 1", who, residual_bin);
    if (int rc = mt_check_side(who, MT_SIGNAL, s_capacity, {s_digit_total, s_cluster_total, s_accepted_total},
                               {s_cluster, s_first, s_u, s_v, lo, mixed_hit}))
        return rc;
    if (int rc = pxd_check_arrays(who, "flags", "capacity", s_capacity, {flags})) return rc;
    if (int rc = mt_check_side(who, MT_MIXED, m_capacity, {m_digit_total, m_cluster_total, m_accepted_total},
                               {m_ccharge, m_u, m_v, signal_charge}))
        return rc;
    if (int rc = pxd_check_needed(who, "table / overflow", 8, {table, overflow})) return rc;
    const int s_cap = pxd_cap(s_capacity), m_cap = pxd_cap(m_capacity);
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_match_stats_kernel, dim3(cl_blocks(s_cap)), dim3(PXD_THREADS), 0, st, s_cluster, s_accepted_total, s_first,
                       s_cluster_total, s_digit_total, s_cap, s_u, s_v, m_ccharge, m_cluster_total, m_accepted_total, m_digit_total, m_cap, m_u,
                       m_v, lo, signal_charge, mixed_hit, (const uint8_t*)flags, N, H, W, n_sensors, (double)residual_bin, (u64*)table,
                       (u64*)overflow);
    CHECK_LAUNCH("pxd_match_stats");
    return 0;
}
