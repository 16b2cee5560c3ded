// PXD space points and inner / outer-layer hit doublets on top of pxd_hits.hip: the hits of a batch placed in a global frame by a placement
// given as data (pxd.PXDPlacement), then paired across the two layers of one event under an azimuth window and a beam-line window.
// Declared in include/ieagan_pxd_tracking.h.  Every array stays in HBM; every decision is made in integers.
//
//   units     sub-units of 1 / 16 geometry unit.  lu = (int)rintf(u * 16.0f): one exact fp32 multiply and one round to nearest even, the
//             last float of the chain.
//   point     X_c = origin[s][c] + ((u_axis[s][c] * lu + v_axis[s][c] * lv + 2^29) >> 30) for c = x, y, z: Q30 axes, |axis| <= 2^30,
//             |lu|, |lv| < 2^23, so the sum stays below 2^54 and the shift is an arithmetic int64 shift.  r = floor(sqrt(x^2 + y^2)):
//             x^2 + y^2 < 2^47 is exact in a double, the double root is corrected by +-1 with integer tests.  The sensor of a hit is
//             (first[cluster[a]] / HW) % S, its role layer[s] (0 inner, 1 outer, -1 ignored).  The placement is checked on the host to keep
//             every corner of every sensor below 2^23 sub-units.
//   offsets   hits are stored image by image (clusters are numbered by their first digit), so the exclusive prefix of the per-image
//             accepted counts gives the rows of image n as [offsets[n], offsets[n + 1]) and those of event e as [offsets[e S], offsets[(e + 1) S]).
//   doublet   inner hit a (role 0) and outer hit b (role 1) of one event, in int64:
//               pairs[s_a][s_b] != 0
//               dot = x_a x_b + y_a y_b > 0  and  |x_a y_b - y_a x_b| << 12 <= tan_q12 * dot           |cross|, dot < 2^47: both sides < 2^63
//               r_b > r_a  and  |z_a r_b - z_b r_a| <= z0_sub * (r_b - r_a)                              both sides < 2^48
//
// Kernels.
//   points    one thread per hit row below the accepted total (pxd_total); offsets: one workgroup scans the N counts.
//   count     workgroup b owns up to DB_TILE = 256 consecutive rows of one event: event e gets the workgroups from B_e = offsets[e S] / 256 + e
//             on (B_e ascends strictly, and B_{e+1} - B_e >= ceil(rows of e / 256)), a workgroup finds its event by bisection over B.  The
//             launch has capacity / 256 + E + 1 workgroups: its shape depends on the capacity and N alone.  A thread keeps x, y, z, r and
//             the sensor of its row in registers; the workgroup streams the rows of its event through LDS in tiles of 256 records of 16
//             bytes (x, y, z, r | sensor << 24; a record that cannot pair with the workgroup has r = 0 and fails r_b > r_a), one record per
//             thread, and every thread tests every record of a tile, read by all lanes from one address (a broadcast).  The test is
//             predicated adds, no divergent branch.  pairs lies in LDS as a bit table.  A tile without a record of role 1 that some inner
//             sensor of the workgroup pairs with is skipped (__syncthreads_or: uniform); a workgroup without an inner row leaves after
//             its loads.  Writes partners[row] (0 for a row that is not inner), the wave's number into its slot, and adds it to
//             event_doublets[e] (int32 atomics, which commute; zeroed by a launch in front).  The outer rows of an event come sensor by
//             sensor, so a thread also keeps the doublets of the current outer sensor and adds them to pair_doublets[s_a][s_b] when the
//             sensor of the records changes (the same records for every thread: the branch is uniform) and after the last tile.
//   scan      pxd_scan_total_kernel over the wave slots: bases and the total.
//   fill      the count pass again.  Workgroups, waves and lanes ascend with the rows, and a thread meets the outer rows in ascending order:
//             its doublets go to base[wave] + partners of the lower lanes + k, k = 0, 1, ...: ascending (inner, outer), one writer per
//             address, no sort, no atomic.  Positions at or beyond doublet_capacity are not written.
//   stats     one launch of 64-bit integer atomics into the accumulator's table; it reads partners, event_doublets and pair_doublets, never
//             the list, so the statistics do not depend on doublet_capacity.
// Two calls on the same input write the same bytes.
//
// Safe.  The accepted total is clipped to the capacity and every offset to [0, total], an event's end to its start; a sensor is compared
// with S before it indexes pairs (idx < S * S <= 65025 bits); the bisection probes offsets[e S] with e < E only; a list position is compared
// with doublet_capacity as an unsigned number.  A total beyond capacity, a sensor outside 0 .. S-1 and offsets that do not ascend give
// wrong numbers, never a wrong address.
#include "common.h"
#include "pxd_common.h"

#define DB_TILE PXD_THREADS
#define DB_MAX_SENSORS 255
#define DB_BIT_WORDS ((DB_MAX_SENSORS * DB_MAX_SENSORS + 31) / 32)
#define DB_PARTNER_BINS 64
#define DB_EVENT_BINS 251
#define DB_COUNTERS 5           // events, inner hits, outer hits, doublets, sum n_in * n_out

// floor(sqrt(s)) for 0 <= s < 2^52: the double root is within 1 of it.
__device__ __forceinline__ int db_isqrt(i64 s) {
    i64 q = (i64)sqrt((double)s);
    q -= q * q > s ? 1 : 0;
    q += (q + 1) * (q + 1) <= s ? 1 : 0;
    return (int)q;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_space_points_kernel(
    const int* __restrict__ cluster, const int* __restrict__ atotal, const int* __restrict__ first, const int* __restrict__ ctotal,
    const float* __restrict__ u, const float* __restrict__ v, const int* __restrict__ origin, const int* __restrict__ u_axis,
    const int* __restrict__ v_axis, const int* __restrict__ layer, int cap, int HW, int S, int* __restrict__ x, int* __restrict__ y,
    int* __restrict__ z, int* __restrict__ r, int* __restrict__ sensor, int8_t* __restrict__ role) {
    const int T = pxd_total(ctotal, cap);
    const int A = pxd_total(atotal, T);
    for (int a = pxd_grid_thread(); a < A; a += pxd_grid_threads()) {
        const int j = cluster[a];
        const int f = (unsigned)j < (unsigned)T ? first[j] : -1;
        int s = -1, ro = -1, X[3] = {0, 0, 0}, rr = 0;
        if (f >= 0) {                               // else: not a row of the table, a point at the origin that plays no role
            s = (f / HW) % S;
            const int l = layer[s];
            ro = l == 0 || l == 1 ? l : -1;
            const i64 lu = (i64)(int)rintf(u[a] * 16.0f), lv = (i64)(int)rintf(v[a] * 16.0f);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                X[c] = (int)((i64)origin[3 * s + c] + (((i64)u_axis[3 * s + c] * lu + (i64)v_axis[3 * s + c] * lv + (1ll << 29)) >> 30));
            rr = db_isqrt((i64)X[0] * X[0] + (i64)X[1] * X[1]);
        }
        x[a] = X[0];
        y[a] = X[1];
        z[a] = X[2];
        r[a] = rr;
        sensor[a] = s;
        role[a] = (int8_t)ro;
    }
}

// offsets [N + 1] = exclusive prefix of counts [N] (negative counts as 0), by one workgroup of PXD_SCAN_THREADS threads.
__global__ __launch_bounds__(PXD_SCAN_THREADS) void pxd_offsets_kernel(const int* __restrict__ counts, int N, int* __restrict__ offsets) {
    __shared__ int wsum[PXD_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int n0 = 0; n0 < N; n0 += PXD_SCAN_THREADS) {
        const int n = n0 + tid;
        const int c = n < N ? max(counts[n], 0) : 0;
        const int incl = pxd_wave_scan(c, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = 0, tile = 0;
#pragma unroll
        for (int k = 0; k < PXD_SCAN_THREADS / 64; ++k) {
            const int s = wsum[k];
            before += k < wave ? s : 0;
            tile += s;
        }
        if (n < N) offsets[n] = carry + before + incl - c;
        carry += tile;
        __syncthreads();
    }
    if (tid == 0) offsets[N] = carry;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_doublets_init_kernel(int* __restrict__ event_doublets, int E, int* __restrict__ pair_doublets,
                                                                        int SS) {
    for (int e = pxd_grid_thread(); e < E; e += pxd_grid_threads()) event_doublets[e] = 0;
    for (int k = pxd_grid_thread(); k < SS; k += pxd_grid_threads()) pair_doublets[k] = 0;
}

// An offset as a row: clipped to [0, A].
__device__ __forceinline__ int db_row(const int* __restrict__ offsets, long n, int A) { return max(min(offsets[n], A), 0); }

// FILL = false: the count pass (partners, slots, event_doublets, pair_doublets); FILL = true: the fill pass (inner, outer), slots hold the bases.
template <bool FILL>
__global__ __launch_bounds__(PXD_THREADS) void pxd_doublets_kernel(
    const int* __restrict__ x, const int* __restrict__ y, const int* __restrict__ z, const int* __restrict__ r, const int* __restrict__ sensor,
    const int8_t* __restrict__ role, const int* __restrict__ offsets, const int* __restrict__ atotal, const uint8_t* __restrict__ pairs, int cap,
    int E, int S, int tan_q12, int z0_sub, int capD, int* partners, int* __restrict__ event_doublets, int* __restrict__ pair_doublets, int* slots,
    int* __restrict__ inner, int* __restrict__ outer) {
    __shared__ int4 tile[DB_TILE];
    __shared__ unsigned bits[DB_BIT_WORDS];
    __shared__ unsigned reach[8];           // bit s_b: some inner sensor of this workgroup pairs with the outer sensor s_b
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int A = pxd_total(atotal, cap);
    // the event of this workgroup: the last e with B_e = row(offsets[e S]) / DB_TILE + e <= b (uniform)
    int e_lo = 0, e_hi = E;
    while (e_lo < e_hi) {
        const int mid = (e_lo + e_hi) >> 1;
        if (db_row(offsets, (long)mid * S, A) / DB_TILE + mid <= b) e_lo = mid + 1;
        else e_hi = mid;
    }
    const int e = e_lo - 1;
    int lo = 0, hi = 0, row = -1;
    if (e >= 0) {
        lo = db_row(offsets, (long)e * S, A);
        hi = max(db_row(offsets, (long)(e + 1) * S, A), lo);
        const long mine = (long)lo + (long)(b - (lo / DB_TILE + e)) * DB_TILE + tid;
        if (mine < hi) row = (int)mine;
    }
    int xa = 0, ya = 0, za = 0, ra = 0, sa = -1;
    bool is_inner = false;
    if (row >= 0) {
        xa = x[row], ya = y[row], za = z[row], ra = r[row], sa = sensor[row];
        is_inner = role[row] == 0 && (unsigned)sa < (unsigned)S;
    }
    if (!__syncthreads_or(is_inner)) {          // uniform: nothing to pair in this workgroup
        if (!FILL) {
            if (row >= 0) partners[row] = 0;
            if (lane == 0) slots[b * PXD_WAVES + wave] = 0;
        }
        return;
    }
    const int SS = S * S;
    for (int w = tid; w < (SS + 31) / 32; w += PXD_THREADS) {
        unsigned word = 0u;
        for (int k = 0; k < 32; ++k) {
            const int idx = w * 32 + k;
            word |= idx < SS && pairs[idx] != 0 ? 1u << k : 0u;
        }
        bits[w] = word;
    }
    if (tid < 8) reach[tid] = 0u;
    __syncthreads();
    const unsigned rowbase = is_inner ? (unsigned)(sa * S) : 0u;
    {   // rows come sensor by sensor: the first lane of a run of one inner sensor adds that sensor's row of pairs to reach
        const int key = is_inner ? sa : -1;
        const int before = __shfl_up(key, 1, 64);
        if (is_inner && (lane == 0 || before != key)) {
            for (int w = 0; w < 8; ++w) {
                unsigned word = 0u;
                for (int k = 0; k < 32; ++k) {
                    const int sb = w * 32 + k;
                    const unsigned idx = rowbase + (unsigned)sb;
                    word |= sb < S && ((bits[idx >> 5] >> (idx & 31u)) & 1u) ? 1u << k : 0u;
                }
                if (word) atomicOr(&reach[w], word);
            }
        }
    }
    __syncthreads();
    int base = 0;
    if (FILL) {
        const int my = row >= 0 ? partners[row] : 0;
        base = slots[b * PXD_WAVES + wave] + pxd_wave_scan(my, lane) - my;
    }
    const i64 tan = tan_q12, z0 = z0_sub;
    int cnt = 0, run_sb = 0, run_cnt = 0;           // count pass: the doublets with the outer sensor run_sb that are not yet in pair_doublets
    for (int t0 = lo; t0 < hi; t0 += DB_TILE) {         // uniform
        const int rb_row = t0 + tid;
        int4 rec = make_int4(0, 0, 0, 0);
        bool relevant = false;
        if (rb_row < hi) {
            const int sb = sensor[rb_row];
            if (role[rb_row] == 1 && (unsigned)sb < (unsigned)S && ((reach[sb >> 5] >> (sb & 31)) & 1u)) {
                relevant = true;
                rec = make_int4(x[rb_row], y[rb_row], z[rb_row], (r[rb_row] & 0xFFFFFF) | sb << 24);
            }
        }
        tile[tid] = rec;
        if (!__syncthreads_or(relevant)) continue;      // uniform; nobody has read the tile
        const int nrec = min(DB_TILE, hi - t0);
#pragma unroll 4
        for (int j = 0; j < nrec; ++j) {
            const int4 q = tile[j];
            const int rb = q.w & 0xFFFFFF;
            const int sb = (int)((unsigned)q.w >> 24);
            const unsigned idx = rowbase + (unsigned)sb;
            const unsigned allowed = (bits[idx >> 5] >> (idx & 31u)) & 1u;
            const i64 dot = (i64)xa * q.x + (i64)ya * q.y;
            const i64 cross = (i64)xa * q.y - (i64)ya * q.x;
            const i64 across = cross < 0 ? -cross : cross;
            const int dr = rb - ra;
            const i64 rz = (i64)za * rb - (i64)q.z * ra;
            const i64 arz = rz < 0 ? -rz : rz;
            const bool ok = (allowed != 0u) & is_inner & (dot > 0) & ((across << 12) <= tan * dot) & (dr > 0) & (arz <= z0 * (i64)dr);
            if (FILL) {
                if (ok) {
                    const int pos = base + cnt;
                    if ((unsigned)pos < (unsigned)capD) {
                        inner[pos] = row;
                        outer[pos] = t0 + j;
                    }
                }
            }
            cnt += ok ? 1 : 0;
            if (!FILL) {
                if (sb != run_sb) {             // uniform: every thread reads the same record
                    if (run_cnt) atomicAdd(pair_doublets + rowbase + run_sb, run_cnt);
                    run_cnt = 0;
                    run_sb = sb;
                }
                run_cnt += ok ? 1 : 0;
            }
        }
        __syncthreads();                                // the next tile overwrites this one
    }
    if (!FILL) {
        if (run_cnt) atomicAdd(pair_doublets + rowbase + run_sb, run_cnt);
        if (row >= 0) partners[row] = cnt;
        const int all = pxd_wave_sum(cnt);
        if (lane == 0) {
            slots[b * PXD_WAVES + wave] = all;
            if (all) atomicAdd(event_doublets + e, all);
        }
    }
}

// The bin of pxd.pxd_bin_index for an integer v >= 0.
__device__ __forceinline__ int db_event_bin(int v) { return v < 1 ? 0 : v < 7 ? 1 : 2 + min(v - 7, 248); }

__global__ __launch_bounds__(PXD_THREADS) void pxd_doublet_stats_kernel(
    const int8_t* __restrict__ role, const int* __restrict__ offsets, const int* __restrict__ atotal,
    const int* __restrict__ dtotal, const int* __restrict__ layer, const int* __restrict__ partners, const int* __restrict__ event_doublets,
    const int* __restrict__ pair_doublets, int cap, int E, int S, u64* __restrict__ tables, u64* __restrict__ overflow) {
    const int t0 = pxd_grid_thread();
    if (t0 == 0 && dtotal[0] > cap) atomicAdd(overflow, 1ull);
    const int A = pxd_total(atotal, cap);
    u64* pair = tables + DB_COUNTERS;
    u64* part = pair + (long)S * S;
    u64* spec = part + DB_PARTNER_BINS;
    for (int a = t0; a < A; a += pxd_grid_threads())
        if (role[a] == 0) atomicAdd(part + min(max(partners[a], 0), DB_PARTNER_BINS - 1), 1ull);
    for (int k = t0; k < S * S; k += pxd_grid_threads()) {
        const int c = pair_doublets[k];
        if (c > 0) atomicAdd(pair + k, (u64)c);
    }
    for (int e = t0; e < E; e += pxd_grid_threads()) {
        u64 n_in = 0, n_out = 0;
        for (int s = 0; s < S; ++s) {
            const int c = max(db_row(offsets, (long)e * S + s + 1, A) - db_row(offsets, (long)e * S + s, A), 0);
            const int l = layer[s];
            n_in += l == 0 ? c : 0;
            n_out += l == 1 ? c : 0;
        }
        const int d = max(event_doublets[e], 0);
        atomicAdd(tables + 0, 1ull);
        atomicAdd(tables + 1, n_in);
        atomicAdd(tables + 2, n_out);
        atomicAdd(tables + 3, (u64)d);
        atomicAdd(tables + 4, n_in * n_out);
        atomicAdd(spec + db_event_bin(d), 1ull);
    }
}

static inline int db_groups(int cap, int E) { return cap / DB_TILE + E + 1; }

static int db_check_shape(const char* who, int N, int n_sensors) {
    CHECK_ARG(N > 0 && N <= 65535, "%s: N = %d outside 1 .. 65535", who, N);
    CHECK_ARG(n_sensors >= 1 && n_sensors <= DB_MAX_SENSORS, "%s: n_sensors = %d outside 1 .. %d", who, n_sensors, DB_MAX_SENSORS);
    return pxd_check_whole_events(who, N, n_sensors);
}

extern "C" int ieagan_pxd_space_points(const int* cluster, const int* accepted_total, const int* first, const int* cluster_total,
                                       const int* counts, const float* u, const float* v, const int* origin, const int* u_axis,
                                       const int* v_axis, const int* layer, int N, int H, int W, int n_sensors, long capacity, int* x, int* y,
                                       int* z, int* r, int* sensor, signed char* role, int* offsets, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const char* who = "pxd_space_points";
    if (int rc = pxd_check_geometry(who, N, H, W, true)) return rc;
    if (int rc = db_check_shape(who, N, n_sensors)) return rc;
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    if (int rc = pxd_check_totals(who, "accepted_total / cluster_total", {accepted_total, cluster_total})) return rc;
    if (int rc = pxd_check_needed(who, "a placement table", 4, {origin, u_axis, v_axis, layer})) return rc;
    if (int rc = pxd_check_needed(who, "counts / offsets", 4, {counts, offsets})) return rc;
    if (int rc = pxd_check_arrays(who, "cluster / first / u / v", "capacity", capacity, {cluster, first, u, v})) return rc;
    if (int rc = pxd_check_arrays(who, "an output array", "capacity", capacity, {x, y, z, r, sensor, role})) return rc;
    if (int rc = pxd_check_aligned(who, "an int32 / fp32 array", 4, {cluster, first, u, v, x, y, z, r, sensor})) return rc;
    const int cap = pxd_cap(capacity);
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_space_points_kernel, dim3(cl_blocks(cap)), dim3(PXD_THREADS), 0, st, cluster, accepted_total, first, cluster_total, u, v,
                       origin, u_axis, v_axis, layer, cap, H * W, n_sensors, x, y, z, r, sensor, (int8_t*)role);
    CHECK_LAUNCH("pxd_space_points");
    hipLaunchKernelGGL(pxd_offsets_kernel, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, counts, N, offsets);
    CHECK_LAUNCH("pxd_space_points offsets");
    return 0;
}

extern "C" long ieagan_pxd_doublets_scratch(int N, int n_sensors, long capacity) {
    if (N <= 0 || n_sensors <= 0 || capacity < 0) return 0;
    return (long)PXD_WAVES * db_groups(pxd_cap(capacity), N / n_sensors);
}

extern "C" int ieagan_pxd_doublets(const int* x, const int* y, const int* z, const int* r, const int* sensor, const signed char* role,
                                   const int* offsets, const int* accepted_total, const unsigned char* pairs, int N, int n_sensors,
                                   long capacity, int tan_q12, int z0_sub, long doublet_capacity, int* partners, int* event_doublets,
                                   int* pair_doublets, int* total, int* inner, int* outer, int* scratch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const char* who = "pxd_doublets";
    if (int rc = db_check_shape(who, N, n_sensors)) return rc;
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    if (int rc = pxd_check_capacity(who, "doublet_capacity", doublet_capacity)) return rc;
    CHECK_ARG(tan_q12 >= 1 && tan_q12 <= 32768, "%s: tan_q12 = %d outside 1 .. 32768", who, tan_q12);
    CHECK_ARG(z0_sub >= 0 && z0_sub < (1 << 23), "%s: z0_sub = %d outside 0 .. 2^23 - 1", who, z0_sub);
    if (int rc = pxd_check_totals(who, "accepted_total", {accepted_total})) return rc;
    if (int rc = pxd_check_needed(who, "offsets / event_doublets / pair_doublets / total", 4, {offsets, event_doublets, pair_doublets, total})) return rc;
    CHECK_ARG(pairs != nullptr, "%s: pairs is NULL", who);
    if (int rc = pxd_check_needed(who, "scratch (ieagan_pxd_doublets_scratch int32 words)", 4, {scratch})) return rc;
    if (int rc = pxd_check_arrays(who, "a space-point array", "capacity", capacity, {x, y, z, r, sensor, role})) return rc;
    if (int rc = pxd_check_arrays(who, "partners", "capacity", capacity, {partners})) return rc;
    if (int rc = pxd_check_arrays(who, "inner / outer", "doublet_capacity", doublet_capacity, {inner, outer})) return rc;
    if (int rc = pxd_check_aligned(who, "an int32 array", 4, {x, y, z, r, sensor, partners, inner, outer})) return rc;
    const int cap = pxd_cap(capacity), capD = pxd_cap(doublet_capacity), E = N / n_sensors;
    const int G = db_groups(cap, E);
    int* slots = scratch;
    {
        ProfScope prof("pxd_doublets count", 0.0, 0.0, st);
        hipLaunchKernelGGL(pxd_doublets_init_kernel, dim3(cl_blocks(E)), dim3(PXD_THREADS), 0, st, event_doublets, E, pair_doublets,
                           n_sensors * n_sensors);
        CHECK_LAUNCH("pxd_doublets init");
        hipLaunchKernelGGL(pxd_doublets_kernel<false>, dim3(G), dim3(PXD_THREADS), 0, st, x, y, z, r, sensor, (const int8_t*)role, offsets,
                           accepted_total, (const uint8_t*)pairs, cap, E, n_sensors, tan_q12, z0_sub, capD, partners, event_doublets, pair_doublets,
                           slots, inner, outer);
        CHECK_LAUNCH("pxd_doublets count");
        hipLaunchKernelGGL(pxd_scan_total_kernel<PXD_SCAN_THREADS>, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, slots, G, total);
        CHECK_LAUNCH("pxd_doublets scan");
    }
    ProfScope prof("pxd_doublets fill", 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_doublets_kernel<true>, dim3(G), dim3(PXD_THREADS), 0, st, x, y, z, r, sensor, (const int8_t*)role, offsets, accepted_total,
                       (const uint8_t*)pairs, cap, E, n_sensors, tan_q12, z0_sub, capD, partners, event_doublets, pair_doublets, slots, inner, outer);
    CHECK_LAUNCH("pxd_doublets fill");
    return 0;
}

extern "C" int ieagan_pxd_doublet_stats(const signed char* role, const int* offsets, const int* accepted_total,
                                        const int* digit_total, const int* layer, const int* partners, const int* event_doublets,
                                        const int* pair_doublets, int N, int n_sensors, long capacity, unsigned long long* tables,
                                        unsigned long long* overflow, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const char* who = "pxd_doublet_stats";
    if (int rc = db_check_shape(who, N, n_sensors)) return rc;
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    if (int rc = pxd_check_totals(who, "accepted_total / digit_total", {accepted_total, digit_total})) return rc;
    if (int rc = pxd_check_needed(who, "offsets / layer / event_doublets / pair_doublets", 4, {offsets, layer, event_doublets, pair_doublets})) return rc;
    if (int rc = pxd_check_needed(who, "tables / overflow", 8, {tables, overflow})) return rc;
    if (int rc = pxd_check_arrays(who, "role / partners", "capacity", capacity, {role, partners})) return rc;
    if (int rc = pxd_check_aligned(who, "partners", 4, {partners})) return rc;
    const int cap = pxd_cap(capacity), E = N / n_sensors;
    const long most = cap > E ? cap : E;
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_doublet_stats_kernel, dim3(cl_blocks(most)), dim3(PXD_THREADS), 0, st, (const int8_t*)role, offsets, accepted_total,
                       digit_total, layer, partners, event_doublets, pair_doublets, cap, E, n_sensors, (u64*)tables, (u64*)overflow);
    CHECK_LAUNCH("pxd_doublet_stats");
    return 0;
}
