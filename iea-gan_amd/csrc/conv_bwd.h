// What the fused whole-backward kernels (conv1x1_bwd.hip, conv3x3_bwd.hip) share: the LDS tables of the BatchNorm prologue and the effgrad
// term, effgrad on load, the prologue backward of one 16-byte chunk, the block-end flush of the per-image BatchNorm accumulators and, on
// the host, the persistent-block plan, the descriptor checks and the workspace / slots queries.  Each kernel file keeps its own tiling,
// staging and MFMA loops.  conv1x1_bwd keeps its BatchNorm table staging, prologue backward and block-end fold in place (see prologue_bwd8).
#pragma once
#include "conv_common.h"

typedef const __attribute__((address_space(3))) float* lds_cf;
typedef const __attribute__((address_space(3))) f32x4* lds_cf4;

// ------------------------------------------------------------------------------------------------------------------------- device
// Two rows of C floats into a block-resident LDS table: dst[0, C) = r0, dst[hi, hi + C) = k1 * r1.  (The BatchNorm table of image n: scale /
// shift; the effgrad table of its event: dsum / 2 dsumsq.)  The caller's next block barrier publishes it.
__device__ __forceinline__ void stage_rows(float* dst, int hi, const float* r0, const float* r1, int C, float k1 = 1.f) {
    for (int i = threadIdx.x; i < C; i += 256) {
        dst[i] = r0[i];
        dst[hi + i] = k1 * r1[i];
    }
}
__device__ __forceinline__ void stage_bn_rows(float* aff_s, const SrcDesc& s, int n, int C) {
    stage_rows(aff_s, C, s.scale + (long)n * s.aff_nstride, s.shift + (long)n * s.aff_nstride, C);
}
__device__ __forceinline__ void stage_eff_rows(float* eff_s, const float* dstat, int n, int n_per_event, int C) {
    const int ev = (n_per_event > 0) ? n / n_per_event : 0;
    stage_rows(eff_s, C, dstat + (long)ev * 2 * C, dstat + (long)ev * 2 * C + C, C, 2.f);
}

// effgrad on load: g + dsum[c] + y * 2 dsumsq[c] over one 16-byte chunk; dsl = this chunk's entry of the LDS table {dsum[C], 2 dsumsq[C]}
__device__ __forceinline__ bf16x8 effgrad8(bf16x8 g, bf16x8 y, const float* dsl, int C) {
    const f32x4 d0 = *(lds_cf4)(dsl), d1 = *(lds_cf4)(dsl + 4), q0 = *(lds_cf4)(dsl + C), q1 = *(lds_cf4)(dsl + C + 4);
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = f2bf(bf2f(g[i]) + (i < 4 ? d0[i & 3] : d1[i & 3]) + bf2f(y[i]) * (i < 4 ? q0[i & 3] : q1[i & 3]));
    return o;
}

// Backward of the fused prologue relu(x * scale + shift) (AFF) / relu(x) over one chunk: v = da on entry, dx on exit; xv = the raw input;
// affl = this chunk's entry of the LDS table {scale[C], shift[C]}.  AFF: s1 += d (-> d shift), s2 += d * x (-> d scale).
// conv1x1_bwd has its own copy of this loop (run-time ReLU flag) and of the fold of bn_acc_flush: the file is built with
// -ffp-contract=fast, and with the helpers in that kernel the compiler fused other s2 += d * x into FMAs than before, which moves the
// last bits of its bn_acc.  A change of the arithmetic here has to be made there too.
template <bool AFF>
__device__ __forceinline__ void prologue_bwd8(float (&v)[8], bf16x8 xv, const float* affl, int C, float (&s1)[8], float (&s2)[8]) {
    f32x4 c0 = {1.f, 1.f, 1.f, 1.f}, c1 = c0, h0 = {0.f, 0.f, 0.f, 0.f}, h1 = h0;
    if (AFF) {
        c0 = *(lds_cf4)(affl);
        c1 = *(lds_cf4)(affl + 4);
        h0 = *(lds_cf4)(affl + C);
        h1 = *(lds_cf4)(affl + C + 4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float xf = bf2f(xv[i]);
        const float sc = i < 4 ? c0[i & 3] : c1[i & 3], sh = i < 4 ? h0[i & 3] : h1[i & 3];
        const float d = !((AFF ? xf * sc + sh : xf) > 0.f) ? 0.f : v[i];
        if (AFF) {
            s1[i] += d;
            s2[i] += d * xf;
            v[i] = d * sc;
        } else {
            v[i] = d;
        }
    }
}

// Block end: the per-image BatchNorm accumulators (sum d, sum d * x).  The lanes that share a chunk are folded through LDS (stats_fold), the
// four waves in a fixed order, then one add per channel and block into slot bid % R of image n.  R = bn_slots == blocks per image makes it
// one adder per address (bit-reproducible); 0: BNB_REPL replicas.  sx: 4 * STATS_SX_FLOATS floats that are free now; free again on return.
template <int C>
__device__ __forceinline__ void bn_acc_flush(float (&s1)[8], float (&s2)[8], float* red /*[4][C][2]*/, float* sx, float* bn_acc, int bn_slots, int n, int bid) {
    const int wave = threadIdx.x >> 6, t = threadIdx.x;
    stats_fold<C / 16>(s1, s2, red, sx + wave * STATS_SX_FLOATS, wave);
    __syncthreads();
    if (t < C) {
        float x1 = 0.f, x2 = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
            x1 += red[(wv * C + t) * 2 + 0];
            x2 += red[(wv * C + t) * 2 + 1];
        }
        const int R = bn_slots > 0 ? bn_slots : BNB_REPL;
        float* st = bn_acc + ((long)n * R + bid % R) * 2 * C;
        atomicAdd(st + t, x1);
        atomicAdd(st + C + t, x2);
    }
    __syncthreads();
}

// --------------------------------------------------------------------------------------------------------------------------- host
// ONE round of persistent blocks: every resident slot (256 CUs x blocks per CU) gets one block, whole blocks per image (a block's BatchNorm
// accumulators belong to one image).  tpi tiles per image -> tpb tiles per block (a multiple of round_to, at least min_tpb), bpi blocks per
// image.  (A grid of 1040 blocks on 512 slots ran three rounds, the last one 3 % full.)
struct PersistentPlan {
    int tpb, bpi, nblk;
};
static inline PersistentPlan persistent_plan(int tpi, int N, int blocks_per_cu, int min_tpb, int round_to) {
    int bpi = 256 * blocks_per_cu / N;
    if (bpi < 1) bpi = 1;
    int tpb = cdiv(cdiv(tpi, bpi), round_to) * round_to;
    if (tpb < min_tpb) tpb = min_tpb;
    bpi = cdiv(tpi, tpb);
    return {tpb, bpi, bpi * N};
}

// the descriptor checks both launchers make
static inline int bwd_common_checks(const char* name, const SrcDesc& src, const void* y, const float* dstat, int N, int n_per_event, int Cg, int Cout, int Cin) {
    CHECK_ARG(Cg >= Cout && Cg % 8 == 0 && src.Cx >= Cin && src.Cx % 8 == 0, "%s: bad channel strides", name);
    CHECK_ARG((src.scale == nullptr) == (src.shift == nullptr), "%s: scale / shift must come together", name);
    CHECK_ARG((y == nullptr) == (dstat == nullptr), "%s: the effgrad operands y / dstat must come together", name);
    CHECK_ARG(n_per_event >= 0 && (n_per_event == 0 || N % n_per_event == 0), "%s: N is not a whole number of events", name);
    return 0;
}

// *_workspace (slab elements; 0 = none or a refused descriptor) and *_slots (blocks per image, or the plan's error code).
// plan(descriptor, Plan&) -> 0 or an error code.
template <class Plan, class Desc, class PlanFn>
static inline long bwd_plan_query(const Desc* d, PlanFn plan, bool slots) {
    Plan p;
    if (d == nullptr) return slots ? IEAGAN_EINVAL : 0;
    const int rc = plan(*d, p);
    if (slots) return rc != 0 ? rc : p.bpi;
    return rc != 0 ? 0 : p.ws_elems;
}
