// Sparse event store -> network input: E events of PXD digits that live on the device (what produce.py / pxd_digits.hip write) are
// expanded straight into the tensors the dense path builds from uint8 event files, without a dense uint8 image in HBM in between:
//   ingest   fp32 [E*S, 1, H + 2 pad, W], what ieagan_event_ingest (aug_optim.hip) gives on the dense uint8 images of those events.  The
//            float expression is the one of event_ingest_kernel, in its order, so the two agree bit for bit.
//   dense    uint8 [E*S, H, W], the images every pxd.PXD* accumulator takes.
//
// Store: pos int32 [D] = (sensor * H + ucell) * W + vcell of a digit inside its event, strictly ascending inside an event; charge uint8 [D],
// each > 0; offsets int64 [n_events + 1].  event_ids int32 [E] is read on the device: output images [e * S, (e + 1) * S) are event
// event_ids[e]; an id outside [0, n_events) is an empty event (background only) and offsets is not read for it.
//
// One kernel, two epilogues.  Grid (P, E*S), the partition of pxd_common.h: workgroup (p, n) owns a contiguous range of the OUTPUT elements
// of image n.  An output image is its source image shifted by pad * W elements (the padding rows are contiguous, above and below), so an
// output range is a source pixel range plus charge 0 outside [0, H*W).  The workgroup walks its range in tiles of PXD_CHUNK elements:
//   1. the tile's digits are pos[lo, hi), two lower bounds inside the event's [offsets[id], offsets[id + 1]) -- the second one only over
//      the next `tile length` digits, more cannot lie in the tile when pos ascends strictly.  cl_lower_bound's result, found by the whole
//      workgroup (ev_lower_bound): 3 + 2 rounds of one load each instead of 17 + 12 dependent loads for a production event, which was
//      most of the kernel's time;
//   2. a uint8 LDS tile is zeroed, (barrier), the charges are placed in it, (barrier);
//   3. every output element of the tile is computed from the LDS tile and stored exactly once: scalar head up to the first 16-byte
//      boundary, 16-byte vector stores, scalar tail (PxdSpan).  The LDS tile starts at the misalignment of the output address, so the LDS
//      reads of a vector are aligned too.
// No global memory is filled and then overwritten; the padding rows fall out of the same walk.
//
// Memory safety does not depend on the content of the store: the event's digit range is clipped to [0, D), a digit is placed only after its
// position has been checked against the tile it is placed in, and nothing but the workgroup's own output range is written.  A store that
// breaks its contract (unsorted or duplicate digits) gives wrong pixels, never a wrong address.  Plain vector loads, stores and LDS: no
// atomics, no float reduction, no scratch memory; two calls write the same bytes.
#include "common.h"
#include "pxd_common.h"

#define EV_TILE_PAD 16          // the LDS tile starts at the output address' offset inside its 16 bytes: at most 15 elements

// cl_lower_bound(a, n, v) -- the number of entries of the ascending a[0, n) below v -- by the whole workgroup.  A round: thread t probes
// a[lo + (t + 1) * step - 1], the 256 probes cut [lo, lo + len) into 257 pieces of at most `step` entries, and the number c of probes
// below v (ballot per wave, one LDS slot per wave, one barrier) says which piece holds the answer: [lo + c * step, + step - 1 entries).
// len shrinks by a factor of 257 a round.  Every thread of the workgroup calls it with the same arguments and gets the result.  `round`
// counts the calls' rounds and picks one of two slot sets, so that a round needs one barrier only.  Every index read lies inside [0, n)
// whatever a holds: a probe beyond lo + len is not read, and c counts read probes only, so lo + c * step <= lo + len.
__device__ __forceinline__ int ev_lower_bound(const int* __restrict__ a, int n, int v, int (&slots)[2][PXD_WAVES], int& round) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo = 0, len = n;
    while (len > 0) {                                                       // workgroup-uniform
        const int step = len / (PXD_THREADS + 1) + 1;
        const long i = (long)(tid + 1) * step - 1;                          // < len + 256
        const unsigned long long below = __ballot(i < len && a[lo + i] < v);
        if (lane == 0) slots[round & 1][wave] = __popcll(below);
        __syncthreads();
        int c = 0;
#pragma unroll
        for (int k = 0; k < PXD_WAVES; ++k) c += slots[round & 1][k];
        ++round;
        const int rest = len - c * step;
        lo += c * step;
        len = step - 1 < rest ? step - 1 : rest;
    }
    return lo;
}

// The two epilogues: V output elements per 16-byte store, and how one / V charges become output elements.
struct EvIngest {
    using Out = float;
    static constexpr int V = 4;
    const float* noise;             // fp32, laid out like the output, or NULL
    float scale;
    bool noise_vec;                 // noise and out share their offset inside 16 bytes: float4 loads of the noise
    // event_ingest_kernel (aug_optim.hip): v = inside ? logf(q + 1) * inv_log256 : 0;  if (noise) v += scale * noise;  (v - 0.5) / 0.5
    __device__ __forceinline__ float value(unsigned q, bool inside, float u) const {
        const float inv_log256 = 0.18033688011112042f;      // 1 / ln(256)
        float v = 0.f;
        if (inside) v = logf((float)q + 1.f) * inv_log256;
        // `v += scale * noise[i]` there is one fused multiply-add (the library is built with -ffp-contract=fast, the addend comes out of a
        // branch); written out here, because the vector form of this epilogue would otherwise be split into a packed multiply and an add
        if (noise) v = __builtin_fmaf(scale, u, v);
        return (v - 0.5f) / 0.5f;
    }
    // one element: global element index g (into out and noise), charge q
    __device__ __forceinline__ void one(float* out, long g, unsigned q, bool inside) const { out[g] = value(q, inside, noise ? noise[g] : 0.f); }
    // V elements at a 16-byte aligned output address; lds is 4-byte aligned; in[k]: element k lies in the source rows
    __device__ __forceinline__ void vec(float* out, long g, const uint8_t* lds, const bool (&in)[4]) const {
        const unsigned w = *reinterpret_cast<const unsigned*>(lds);
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        if (noise) {
            if (noise_vec) u = *reinterpret_cast<const float4*>(noise + g);
            else u = make_float4(noise[g], noise[g + 1], noise[g + 2], noise[g + 3]);
        }
        float4 r;
        r.x = value(w & 255u, in[0], u.x);
        r.y = value((w >> 8) & 255u, in[1], u.y);
        r.z = value((w >> 16) & 255u, in[2], u.z);
        r.w = value(w >> 24, in[3], u.w);
        *reinterpret_cast<float4*>(out + g) = r;
    }
};
struct EvDense {
    using Out = uint8_t;
    static constexpr int V = 16;
    __device__ __forceinline__ void one(uint8_t* out, long g, unsigned q, bool) const { out[g] = (uint8_t)q; }
    __device__ __forceinline__ void vec(uint8_t* out, long g, const uint8_t* lds, const bool (&)[16]) const {
        *reinterpret_cast<uint4*>(out + g) = *reinterpret_cast<const uint4*>(lds);
    }
};

// HW: pixels of a source image; OHW: elements of an output image = HW + 2 * shift, shift = pad * W; chunk: output elements per workgroup.
template <typename Epi>
__global__ __launch_bounds__(PXD_THREADS) void pxd_events_kernel(const int* __restrict__ pos, const uint8_t* __restrict__ charge,
                                                                 const long* __restrict__ offsets, long D, const int* __restrict__ event_ids,
                                                                 int n_events, int S, int HW, int OHW, int shift, int chunk,
                                                                 typename Epi::Out* __restrict__ out, Epi epi) {
    using T = typename Epi::Out;
    constexpr int V = Epi::V;
    __shared__ __attribute__((aligned(16))) uint8_t tile[PXD_CHUNK + EV_TILE_PAD];
    __shared__ int slots[2][PXD_WAVES];
    int round = 0;
    const int tid = threadIdx.x, n = blockIdx.y, p = blockIdx.x;
    const int r0 = (long)p * chunk < OHW ? p * chunk : OHW;
    const int r1 = OHW - r0 > chunk ? r0 + chunk : OHW;
    if (r0 >= r1) return;                                                   // workgroup-uniform
    const int e = n / S, sensor = n - e * S;
    const int id = event_ids[e];
    long d0 = 0, d1 = 0;
    if (id >= 0 && id < n_events) {
        d0 = offsets[id];
        d1 = offsets[id + 1];
    }
    d0 = d0 < 0 ? 0 : d0 > D ? D : d0;                                      // whatever offsets holds, pos / charge are read inside [0, D)
    d1 = d1 < d0 ? d0 : d1 > D ? D : d1;
    if (d1 - d0 > (long)INT_MAX) d1 = d0 + INT_MAX;                         // a valid event has fewer than S * H * W < 2^31 digits
    const int* __restrict__ epos = pos + d0;
    const uint8_t* __restrict__ echg = charge + d0;
    const int nd = (int)(d1 - d0);
    const int pbase = sensor * HW;                                          // S * HW < 2^31 (launcher)
    T* __restrict__ img = out + (long)n * OHW;

    for (int t0 = r0; t0 < r1; t0 += PXD_CHUNK) {
        const int len = r1 - t0 > PXD_CHUNK ? PXD_CHUNK : r1 - t0;
        const PxdSpan<T, V, int> sp(img + t0, len);
        const int a = (int)(((uintptr_t)(img + t0) & 15u) / sizeof(T));     // element t0 + k of the image sits at tile[a + k]
        // 1. the digits of the source pixels [s0, s1) of this sensor
        const int s0 = t0 - shift > 0 ? t0 - shift : 0;
        const int s1 = t0 - shift + len < HW ? t0 - shift + len : HW;
        for (int i = tid; i < (PXD_CHUNK + EV_TILE_PAD) / 16; i += PXD_THREADS) reinterpret_cast<uint4*>(tile)[i] = make_uint4(0u, 0u, 0u, 0u);
        int lo = 0, hi = 0;
        if (s0 < s1 && nd > 0) {                                            // workgroup-uniform
            lo = ev_lower_bound(epos, nd, pbase + s0, slots, round);
            const int m = nd - lo < len ? nd - lo : len;
            hi = lo + ev_lower_bound(epos + lo, m, pbase + s1, slots, round);
        }
        // 2. the tile is zeroed (above), place
        __syncthreads();
        for (int i = lo + tid; i < hi; i += PXD_THREADS) {
            const int s = (int)((unsigned)epos[i] - (unsigned)pbase);       // source pixel of this sensor; any int32 may stand in pos
            if (s >= s0 && s < s1) tile[a + (s + shift - t0)] = echg[i];    // s0 <= s < s1  =>  0 <= s + shift - t0 < len
        }
        __syncthreads();
        // 3. every output element once.  Element t0 + k lies in the source rows iff shift <= t0 + k < shift + HW.
        const int in0 = shift - t0, in1 = shift + HW - t0;
        const long g0 = (long)n * OHW + t0;
        if (tid < sp.head) epi.one(out, g0 + tid, tile[a + tid], tid >= in0 && tid < in1);
        for (int i = tid; i < sp.nvec; i += PXD_THREADS) {
            const int k = sp.head + i * V;
            bool in[V];
#pragma unroll
            for (int j = 0; j < V; ++j) in[j] = k + j >= in0 && k + j < in1;
            epi.vec(out, g0 + k, tile + a + k, in);
        }
        if (sp.tail0 + tid < len) {
            const int k = sp.tail0 + tid;
            epi.one(out, g0 + k, tile[a + k], k >= in0 && k < in1);
        }
        __syncthreads();                                                    // the tile is zeroed again by the next step
    }
}

// The checks and the launch of both entry points; `who` is the entry point's name in the error text.
template <typename Epi>
static int pxd_events_launch(const char* who, const int* pos, const unsigned char* charge, const long* offsets, long n_digits, int n_events,
                             const int* event_ids, int E, int S, int H, int W, int pad, typename Epi::Out* out, Epi epi, double noise_bytes,
                             hipStream_t st) {
    CHECK_ARG(n_digits >= 0 && n_events >= 0, "%s: n_digits = %ld / n_events = %d is negative", who, n_digits, n_events);
    CHECK_ARG(n_digits == 0 || (pos != nullptr && charge != nullptr), "%s: pos / charge is NULL with %ld digits", who, n_digits);
    CHECK_ARG(((uintptr_t)pos & 3u) == 0, "%s: pos is not 4-byte aligned", who);
    CHECK_ARG(n_events == 0 || offsets != nullptr, "%s: offsets is NULL with %d events", who, n_events);
    CHECK_ARG(((uintptr_t)offsets & 7u) == 0, "%s: offsets is not 8-byte aligned", who);
    CHECK_ARG(event_ids != nullptr && ((uintptr_t)event_ids & 3u) == 0, "%s: event_ids is NULL or misaligned", who);
    CHECK_ARG(E > 0 && S > 0, "%s: E = %d events of S = %d sensors", who, E, S);
    CHECK_ARG((double)E * S <= 65535.0, "%s: E * S = %d * %d images outside 1 .. 65535", who, E, S);
    if (int rc = pxd_check_geometry(who, S, H, W, true)) return rc;         // S * H * W < 2^31: the positions of an event fit int32
    CHECK_ARG(pad >= 0 && ((double)H + 2.0 * pad) * W < 2147483648.0 - 64.0 * PXD_MAX_PARTS, "%s: pad = %d rows do not fit the int32 element index of an output image", who, pad);
    CHECK_ARG(out != nullptr && ((uintptr_t)out & (sizeof(typename Epi::Out) - 1)) == 0, "%s: out is NULL or misaligned", who);
    const int N = E * S, HW = H * W, shift = pad * W, OHW = HW + 2 * shift;
    const int P = pxd_parts(N, OHW);
    long chunk = ((long)OHW + P - 1) / P;
    chunk = (chunk + 15) / 16 * 16;
    // the digits of the E events (5 bytes each) and the two binary searches depend on the data and are not counted
    const double out_bytes = (double)N * OHW * sizeof(typename Epi::Out);
    ProfScope prof(who, 0.0, out_bytes + noise_bytes, st);
    hipLaunchKernelGGL(pxd_events_kernel<Epi>, dim3(P, N), dim3(PXD_THREADS), 0, st, pos, (const uint8_t*)charge, offsets, n_digits, event_ids,
                       n_events, S, HW, OHW, shift, (int)chunk, out, epi);
    CHECK_LAUNCH(who);
    return 0;
}

extern "C" int ieagan_pxd_event_ingest(const int* pos, const unsigned char* charge, const long* offsets, long n_digits, int n_events,
                                       const int* event_ids, int E, int S, int H, int W, int pad, const float* noise, float scale, float* out,
                                       void* stream) {
    CHECK_ARG(((uintptr_t)noise & 3u) == 0, "pxd_event_ingest: noise is not 4-byte aligned");
    CHECK_ARG(scale == scale, "pxd_event_ingest: scale is NaN");
    EvIngest epi;
    epi.noise = noise;
    epi.scale = scale;
    epi.noise_vec = (((uintptr_t)noise ^ (uintptr_t)out) & 15u) == 0;
    const double noise_bytes = noise ? 4.0 * E * S * ((double)H + 2.0 * pad) * W : 0.0;
    return pxd_events_launch<EvIngest>("pxd_event_ingest", pos, charge, offsets, n_digits, n_events, event_ids, E, S, H, W, pad, out, epi,
                                       noise_bytes, (hipStream_t)stream);
}

extern "C" int ieagan_pxd_event_dense(const int* pos, const unsigned char* charge, const long* offsets, long n_digits, int n_events,
                                      const int* event_ids, int E, int S, int H, int W, unsigned char* out, void* stream) {
    return pxd_events_launch<EvDense>("pxd_event_dense", pos, charge, offsets, n_digits, n_events, event_ids, E, S, H, W, 0, (uint8_t*)out,
                                      EvDense(), 0.0, (hipStream_t)stream);
}
