// Background overlay: E pairs of events of two sparse event stores (the store of pxd_events.hip: pos int32 strictly ascending inside an event,
// charge uint8 in 1 .. 255, offsets int64, ids read on the device, an id outside the store is an empty event) are added pixel by pixel in
// the sparse format.  Output event e is the union of the positions of A[a_ids[e]] and B[b_ids[e]], ascending; a position in one list keeps
// its charge, a position in both gets min(qa + qb, 255) -- the ADC's saturation.  The events lie back to back, out_offsets [E + 1] int64
// holds their starts and the total, the true numbers whatever the capacity; only digits with output index < capacity are written.
//
// This is a merge of sorted lists: the work is proportional to the digits (about 0.8 MB for two production events at 1 % occupancy), no
// pixel of the 7.7 MB dense images is touched, no LDS tile of pixels, no atomic.  Four launches, the launch shapes depend on (E, capacity)
// alone, kernel boundaries are the only global barriers:
//   sum     one workgroup: U[e] = sum over e' < e of (na + nb), the running sum of the INPUT digits of the pairs, int32 [E + 1] in scratch.
//           The event ranges are clipped to [0, D] as in pxd_events_kernel, and the sum is clipped at 2^31 - 1: a call merges fewer than
//           2^31 input digits, beyond that the tail is cut (no address depends on it).  Thread i owns a contiguous run of events, so any
//           E <= 65535 is one pass of a 1024-thread scan.
//   count   the merged index space [0, U[E]) is cut into one contiguous range per wave of the launch (`chunk` digits, a multiple of 64,
//           computed from U[E] on the device: the launch has OV_BLOCKS(capacity) workgroups, about one wave per 64 digits of capacity up
//           to OV_MAX_BLOCKS, so that a production pair is one step per wave and the dependent loads of the searches run side by side on
//           the whole chip -- cl_blocks' one wave per 256 digits would run four searches in a row on 60 % of the CUs).  Lane of
//           merged index t: its pair e by a search in U (kept from step to step), its co-rank (i, j), i + j = t - U[e], by the merge-path
//           binary search with ties resolved A before B, its item A[i] or B[j].  A B item is DROPPED iff i > 0 && A[i-1] == B[j]: its twin
//           lies directly in front of it in the merged order, and the test reads the lists, not the neighbouring lane, so it holds across
//           steps and waves.  A ballot counts the kept items, one slot per wave.
//   scan    one workgroup: exclusive prefix sum over the wave slots (pxd_scan_slots, tiled beyond 1024 workgroups); writes the total to
//           out_offsets[E] and to every trailing empty pair.
//   write   the partition of count again: output index = base of the wave + kept items of its earlier steps + kept items in the lower
//           lanes (ballot).  An A item with a twin B[j] == A[i] takes min(qa + qb, 255).  The first item of a pair is always kept (a B
//           item at i == 0 has nothing in front of it): its lane's output index is out_offsets of its pair and of the empty pairs
//           directly in front of it, written by the wave together.
// Exactly one writer per output element and per offset, integers only: two calls write the same bytes.
//
// Memory safety does not depend on the content of the stores: event ranges are clipped to [0, D]; the merge-path search probes A[mid] with
// mid < na and B[d - mid - 1] with max(0, d - nb) <= mid < min(d, na), both inside their ranges whatever the lists hold; A[i-1] / B[j] are
// read under i > 0 / j < nb; an output index is compared with the capacity before the store.  Stores that break their contract (unsorted or
// duplicate positions) give wrong digits, never a wrong address.  The co-rank search is about log2(na + nb) = 17 rounds of two independent
// loads for a production pair; they hit L2 (the lists are 0.6 MB) and every wave of the launch has its round in flight at once.
#include "common.h"
#include "pxd_common.h"

#define OV_MAX_BLOCKS 4096          // 4 tiles of pxd_scan_slots at the most
static inline int ov_blocks(long cap) { return pxd_blocks(cap, PXD_THREADS, OV_MAX_BLOCKS); }

struct OvStore {
    const int* pos;
    const uint8_t* charge;
    const long* offsets;
    long D;
    int n_events;
    const int* ids;
};

// The digits [d0, d0 + n) of event ids[e], clipped to [0, D] whatever offsets holds; an id outside the store is an empty event.
__device__ __forceinline__ void ov_range(const OvStore& s, int e, long& d0, int& n) {
    const int id = s.ids[e];
    long a = 0, b = 0;
    if (id >= 0 && id < s.n_events) {
        a = s.offsets[id];
        b = s.offsets[id + 1];
    }
    a = a < 0 ? 0 : a > s.D ? s.D : a;
    b = b < a ? a : b > s.D ? s.D : b;
    if (b - a > (long)INT_MAX) b = a + INT_MAX;
    d0 = a;
    n = (int)(b - a);
}

// U[0] = 0, U[e + 1] = min(sum over e' <= e of (na + nb), INT_MAX).
__global__ __launch_bounds__(PXD_SCAN_THREADS) void pxd_overlay_sum_kernel(OvStore A, OvStore B, int E, int* __restrict__ U) {
    __shared__ long wsum[PXD_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (E + PXD_SCAN_THREADS - 1) / PXD_SCAN_THREADS;         // <= 64
    const int e0 = tid * per < E ? tid * per : E, e1 = e0 + per < E ? e0 + per : E;
    long mine = 0;
    for (int e = e0; e < e1; ++e) {
        long d0;
        int na, nb;
        ov_range(A, e, d0, na);
        ov_range(B, e, d0, nb);
        mine += (long)na + nb;
    }
    const long incl = pxd_wave_scan(mine, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    long run = incl - mine;
    for (int k = 0; k < wave; ++k) run += wsum[k];
    if (tid == 0) U[0] = 0;
    for (int e = e0; e < e1; ++e) {
        long d0;
        int na, nb;
        ov_range(A, e, d0, na);
        ov_range(B, e, d0, nb);
        run += (long)na + nb;
        U[e + 1] = run > (long)INT_MAX ? INT_MAX : (int)run;
    }
}

// One item of the merged order.
struct OvItem {
    int e;              // its pair
    int pos;
    int q;              // WRITE only: the charge, summed and saturated when the position is in both lists
    bool kept;          // false: outside the range, or a B item whose twin A[i-1] stands in front of it
    bool first;         // the first item of its pair
};

// The item of merged index t < U[E]; `e` is the lane's pair of the step before (any value in [0, E)), looked up again only when t left it.
template <bool WRITE>
__device__ __forceinline__ OvItem ov_item(const OvStore& A, const OvStore& B, int E, const int* __restrict__ U, int t, int e) {
    if (!(U[e] <= t && t < U[e + 1])) {                 // the last pair with U[e] <= t: the entries of U[1 .. E] that are <= t
        int lo = 0, hi = E;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (U[mid + 1] <= t) lo = mid + 1;
            else hi = mid;
        }
        e = lo < E - 1 ? lo : E - 1;                    // t < U[E]: lo <= E - 1 already
    }
    const int d = t - U[e];
    long a0, b0;
    int na, nb;
    ov_range(A, e, a0, na);
    ov_range(B, e, b0, nb);
    OvItem it;
    it.e = e;
    it.pos = it.q = 0;
    it.kept = it.first = false;
    if ((long)d >= (long)na + nb) return it;            // U was summed over these very ranges; kept so that no read below rests on that
    const int* __restrict__ pa = A.pos + a0;
    const int* __restrict__ pb = B.pos + b0;
    // merge path: i = the A items among the first d of the merged order, A before B on a tie.  0 <= d < na + nb (U may be clipped: then
    // d is only smaller).  Every probe: 0 <= mid < hi <= na and 0 <= d - mid - 1 <= nb - 1.
    int lo = d - nb > 0 ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pa[mid] <= pb[d - mid - 1]) lo = mid + 1;
        else hi = mid;
    }
    const int i = lo, j = d - lo;                       // 0 <= i <= na, 0 <= j <= nb, and i < na or j < nb
    it.first = d == 0;
    const int vb = j < nb ? pb[j] : 0;
    const bool from_a = i < na && (j >= nb || pa[i] <= vb);
    if (from_a) {
        it.pos = pa[i];
        it.kept = true;
        if (WRITE) {
            int q = (int)A.charge[a0 + i];
            if (j < nb && vb == it.pos) q += (int)B.charge[b0 + j];
            it.q = q > 255 ? 255 : q;
        }
    } else {                                            // j < nb here
        it.pos = vb;
        it.kept = !(i > 0 && pa[i - 1] == vb);
        if (WRITE) it.q = (int)B.charge[b0 + j];
    }
    return it;
}

// Merged indices per wave of a launch of `waves` waves: a multiple of 64, the same in count and write.
__device__ __forceinline__ long ov_chunk(int total, int waves) {
    const long c = ((long)total + waves - 1) / waves;
    return c < 64 ? 64 : (c + 63) / 64 * 64;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_overlay_count_kernel(OvStore A, OvStore B, int E, const int* __restrict__ U,
                                                                        int* __restrict__ slots) {
    const PxdWaveRange w(U[E], ov_chunk(U[E], gridDim.x * PXD_WAVES));
    int kept = 0, e = 0;
    for (long kb = w.k0; kb < w.k1; kb += 64) {
        const long t = kb + w.lane;
        bool keep = false;
        if (t < w.k1) {
            const OvItem it = ov_item<false>(A, B, E, U, (int)t, e);
            e = it.e;
            keep = it.kept;
        }
        kept += __popcll(__ballot(keep));
    }
    if (w.lane == 0) slots[w.g] = kept;                 // every slot of the launch, also of a wave without a range
}

// The prefix sum of pxd_common.h over the wave slots of the count launch; the total goes to out_offsets[E] and to the trailing empty pairs
// (those with U[e] == U[E]: no item of the merged order lies at or behind their start, so the write pass does not reach them).
__global__ __launch_bounds__(PXD_SCAN_THREADS) void pxd_overlay_scan_kernel(int* __restrict__ slots, int groups, int E,
                                                                            const int* __restrict__ U, long* __restrict__ out_offsets) {
    const int all = pxd_scan_slots(slots, groups);
    const int M = U[E];
    for (int e = threadIdx.x; e <= E; e += PXD_SCAN_THREADS)
        if (U[e] == M) out_offsets[e] = all;
}

__global__ __launch_bounds__(PXD_THREADS) void pxd_overlay_write_kernel(OvStore A, OvStore B, int E, const int* __restrict__ U,
                                                                        const int* __restrict__ slots, int cap, int* __restrict__ out_pos,
                                                                        uint8_t* __restrict__ out_charge, long* __restrict__ out_offsets) {
    const PxdWaveRange w(U[E], ov_chunk(U[E], gridDim.x * PXD_WAVES));
    const int lane = w.lane;
    int run = slots[w.g], e = 0;
    for (long kb = w.k0; kb < w.k1; kb += 64) {
        const long t = kb + lane;
        OvItem it;
        it.e = e;
        it.pos = it.q = 0;
        it.kept = it.first = false;
        if (t < w.k1) it = ov_item<true>(A, B, E, U, (int)t, e);
        e = it.e;
        const unsigned long long m = __ballot(it.kept);
        const int o = run + pxd_ballot_rank(m, lane);
        if (it.kept && o < cap) {                       // 0 <= o: the kept items in front of this one
            out_pos[o] = it.pos;
            out_charge[o] = (uint8_t)it.q;
        }
        run += __popcll(m);
        // the starts of the pairs that begin in this step: pair e of a first item (kept, so o is its index) and the empty pairs directly in
        // front of it, [f, e) with U[f] == ... == U[e] == t; f = the first entry of U[0 .. E] that is >= t
        const int f = it.first ? cl_lower_bound(U, it.e, (int)t) : it.e;
        unsigned long long firsts = __ballot(it.first);
        while (firsts) {                                // wave-uniform
            const int src = __ffsll(firsts) - 1;
            firsts &= firsts - 1;
            const int pf = __shfl(f, src, 64), pe = __shfl(it.e, src, 64), po = __shfl(o, src, 64);
            for (int k = pf + lane; k <= pe; k += 64) out_offsets[k] = po;
        }
    }
}

extern "C" long ieagan_pxd_event_overlay_scratch(int E, long capacity) {
    if (E <= 0 || capacity < 0) return 0;
    return (long)E + 1 + (long)PXD_WAVES * ov_blocks(pxd_cap(capacity));
}

// One store; `names` are its arguments in the error texts: pos / charge, pos, offsets, ids.
static int ov_check_store(const char* who, const char* side, const char* const names[4], const int* pos, const unsigned char* charge,
                          const long* offsets, long digits, int events, const int* ids) {
    CHECK_ARG(digits >= 0 && events >= 0, "%s: %s_digits = %ld / %s_events = %d is negative", who, side, digits, side, events);
    if (int rc = pxd_check_arrays(who, names[0], "digits", digits, {pos, charge})) return rc;
    if (int rc = pxd_check_aligned(who, names[1], 4, {pos})) return rc;
    if (int rc = pxd_check_arrays(who, names[2], "events", events, {offsets})) return rc;
    if (int rc = pxd_check_aligned(who, names[2], 8, {offsets})) return rc;
    return pxd_check_totals(who, names[3], {ids});
}

extern "C" int ieagan_pxd_event_overlay(const int* a_pos, const unsigned char* a_charge, const long* a_offsets, long a_digits, int a_events,
                                        const int* a_ids, const int* b_pos, const unsigned char* b_charge, const long* b_offsets, long b_digits,
                                        int b_events, const int* b_ids, int E, int S, int H, int W, long capacity, int* out_pos,
                                        unsigned char* out_charge, long* out_offsets, int* scratch, void* stream) {
    const char* who = "pxd_event_overlay";
    hipStream_t st = (hipStream_t)stream;
    static const char* const a_names[4] = {"a_pos / a_charge", "a_pos", "a_offsets", "a_ids"};
    static const char* const b_names[4] = {"b_pos / b_charge", "b_pos", "b_offsets", "b_ids"};
    if (int rc = ov_check_store(who, "a", a_names, a_pos, a_charge, a_offsets, a_digits, a_events, a_ids)) return rc;
    if (int rc = ov_check_store(who, "b", b_names, b_pos, b_charge, b_offsets, b_digits, b_events, b_ids)) return rc;
    CHECK_ARG(E > 0 && E <= 65535, "%s: E = %d pairs outside 1 .. 65535", who, E);
    if (int rc = pxd_check_geometry(who, S, H, W, true)) return rc;         // S * H * W < 2^31: the positions of an event fit int32
    if (int rc = pxd_check_capacity(who, "capacity", capacity)) return rc;
    if (int rc = pxd_check_arrays(who, "out_pos / out_charge", "capacity", capacity, {out_pos, out_charge})) return rc;
    if (int rc = pxd_check_aligned(who, "out_pos", 4, {out_pos})) return rc;
    if (int rc = pxd_check_needed(who, "out_offsets", 8, {out_offsets})) return rc;
    if (int rc = pxd_check_needed(who, "scratch (ieagan_pxd_event_overlay_scratch int32 words)", 4, {scratch})) return rc;
    const int cap = pxd_cap(capacity);
    const int Bk = ov_blocks(cap);
    const OvStore A = {a_pos, (const uint8_t*)a_charge, a_offsets, a_digits, a_events, a_ids};
    const OvStore B = {b_pos, (const uint8_t*)b_charge, b_offsets, b_digits, b_events, b_ids};
    int* U = scratch;
    int* slots = scratch + E + 1;
    // the digits read and written depend on the data and are not counted
    ProfScope prof(who, 0.0, 0.0, st);
    hipLaunchKernelGGL(pxd_overlay_sum_kernel, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, A, B, E, U);
    CHECK_LAUNCH("pxd_event_overlay sum");
    hipLaunchKernelGGL(pxd_overlay_count_kernel, dim3(Bk), dim3(PXD_THREADS), 0, st, A, B, E, (const int*)U, slots);
    CHECK_LAUNCH("pxd_event_overlay count");
    hipLaunchKernelGGL(pxd_overlay_scan_kernel, dim3(1), dim3(PXD_SCAN_THREADS), 0, st, slots, Bk, E, (const int*)U, out_offsets);
    CHECK_LAUNCH("pxd_event_overlay scan");
    hipLaunchKernelGGL(pxd_overlay_write_kernel, dim3(Bk), dim3(PXD_THREADS), 0, st, A, B, E, (const int*)U, (const int*)slots, cap, out_pos,
                       (uint8_t*)out_charge, out_offsets);
    CHECK_LAUNCH("pxd_event_overlay write");
    return 0;
}
