// What the 3x3 tile kernels share (conv3x3_halo in conv_igemm.hip, conv3x3_lds / conv3x3_lds_fp8, conv3x3_ws, conv3x3_ws64): persistent
// blocks walk runs of output tiles inside one statistics group and stage the transformed input halo of a tile in LDS.  This header owns
// the walk (block -> tile run -> tile origin), the halo source addressing and the unconditional request, the prologue of one 16-byte chunk,
// the chunk swizzle and the K loop of the unpadded LDS images, the epilogue's pixel mapping, and on the host side the launch plan, the
// LDS reservation and the prologue -> template-argument dispatch.  Tile shapes, thresholds and launch bounds stay with the kernels.
#pragma once
#include "conv_common.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------------------------------- the tile walk
// XCD-aware order: blocks b and b+8 share an XCD (and its L2), so each XCD gets a contiguous run of tiles -- neighbouring tiles then
// share their halo rows / weights through one L2.  gy > 1 (conv3x3_lds, C = 128: four blocks of 32 couts per tile run): the n-tile
// column is the fast index, so the blocks that read the same halos run side by side on one XCD (conv1x1_stream.hip).
// A block stays inside ONE event (tpe tiles, bpe blocks per event): its statistics go to that event's accumulators with a single
// flush at the end (a flush inside the tile loop costs the C = 16 / 32 variants 40-60 spilled VGPRs).
struct TileRun {
    int column, bid, event, t0, t1;          // n-tile column, renumbered block (without the column), its event and tiles [t0, t1)
};
__device__ __forceinline__ TileRun tile_run(int nblk, int gy, int bpe, int tpe, int tpb) {
    TileRun r;
    const int bid = xcd_block_order(blockIdx.x, nblk * gy);
    r.column = bid % gy;
    r.bid = bid / gy;
    r.event = r.bid / bpe;
    r.t0 = r.event * tpe + (r.bid - r.event * bpe) * tpb;
    r.t1 = min(r.t0 + tpb, (r.event + 1) * tpe);
    return r;
}

template <int TH, int TW>
__device__ __forceinline__ void tile_origin(int t, int tiles_w, int tiles_h, int& n, int& h0, int& w0) {
    n = t / (tiles_w * tiles_h);
    const int trem = t - n * tiles_w * tiles_h;
    h0 = (trem / tiles_w) * TH;
    w0 = (trem % tiles_w) * TW;
}

// --------------------------------------------------------------------------------------------------------------- halo requests
// 16-byte chunk cc of the source pixel behind conv-resolution pixel (n, hh, ww), which must lie inside the image (RS = 1: nearest x2
// up-sample of a half-resolution source).
template <int RS>
__device__ __forceinline__ const bf16x8* halo_src_chunk(const SrcDesc& s, int n, int hh, int ww, int cc) {
    const int sh_ = (RS == 1) ? (hh >> 1) : hh, sw_ = (RS == 1) ? (ww >> 1) : ww;
    return (const bf16x8*)((const bf16*)s.x + (((long)n * s.Hs + sh_) * s.Ws + sw_) * s.Cx + cc * 8);
}

// Raw chunks tid + j * NTHR, j < NB, of the (TOT / (AW * CH)) x AW-pixel halo with origin (h0 - 1, w0 - 1) -> raw[j]; okmask = the mask of
// the chunks that exist (inside the halo and inside the image -- the rest is the zero padding ring, see prologue_chunk).
// The loads are UNCONDITIONAL (coordinates clamped into the image, the chunk index into the halo).  Under a per-lane condition the
// compiler cannot count the younger loads of another register set behind these and drains the counter -- vmcnt(0) -- before the first
// use, which leaves one tile in flight where two were requested.  For the same reason a caller puts no branch or join between a
// request and its use, and past a block's last tile requests that tile again and drops it.
// (Chunks that are consumed before anything else is requested -- conv3x3_halo, the 4-wave conv3x3_lds, the fp8 kernel -- are loaded
//  under their guard at the call site.  okmask is a reference on purpose: with the mask as a return value the compiler issues all
//  NB address computations ahead of the loads, 20 to 40 more VGPRs in the ws64 kernels.)
template <int RS, int CH, int AW, int TOT, int NTHR, int NB>
__device__ __forceinline__ void halo_request(const SrcDesc& s, int H, int W, int n, int h0, int w0, int tid, bf16x8 (&raw)[NB], unsigned& okmask) {
    okmask = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int idx = min(tid + j * NTHR, TOT - 1);
        const int hp = idx / CH, cc = idx - hp * CH;
        const int hh = h0 - 1 + hp / AW, ww = w0 - 1 + hp % AW;
        raw[j] = *halo_src_chunk<RS>(s, n, min(max(hh, 0), H - 1), min(max(ww, 0), W - 1), cc);
        if (tid + j * NTHR < TOT && hh >= 0 && hh < H && ww >= 0 && ww < W) okmask |= 1u << j;
    }
}

// Prologue of one requested chunk: per-(n, c) affine (BatchNorm apply) and ReLU in fp32, rounded back to bf16; zero where the chunk
// does not exist (conv padding is applied AFTER the activation).  scale / shift: the 8 values of this chunk's channels in LDS -- rows of
// the block-wide table (stage_aff) or of a producer wave's private copy; not read unless AFF.
template <bool AFF, bool RELU>
__device__ __forceinline__ bf16x8 prologue_chunk(const bf16x8& raw, bool ok, const float* scale, const float* shift) {
    if (!ok) return zero8();
    if (!AFF && !RELU) return raw;
    if (!AFF) return relu8(raw);
    const f32x8 sc = lds_load8(scale), sh = lds_load8(shift);
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float v = bf2f(raw[i]) * sc[i] + sh[i];
        if (RELU) v = fmaxf(v, 0.f);
        o[i] = f2bf(v);
    }
    return o;
}

// ------------------------------------------------------------------------------------------------- unpadded, swizzled LDS images
// 16-byte chunk swizzle of an LDS image with CPR chunks per row.  Rows are CPR*16 bytes apart, so the 16 lanes of a fragment
// read (same chunk of 16 consecutive rows) would hit only one or two of the sixteen 16-byte bank slots.  The chunk index is
// XOR-ed with a per-row key:  CPR % 16 == 8 -> the row parity already selects one half of the slots, permute the low 3 chunk
// bits with key = (r >> 1) & 7;  CPR % 16 == 0 -> permute 4 bits with key = r & 15.  `r` only has to enumerate the 16 rows of
// a fragment read bijectively: the weight image uses the row index, the halo image the COLUMN of the pixel inside its halo row
// (16 consecutive pixels of a row), which keeps every read address = per-lane register + compile-time immediate.
// (CPR % 16 == 4, the fp8 images of 64-channel rows: two row bits select a quarter of the slots, key = (r >> 2) & 3 permutes 2 bits.)
template <int CPR>
__device__ __forceinline__ int swz_key(int r) {
    static_assert(CPR % 16 == 8 || CPR % 16 == 0 || CPR % 16 == 4, "swizzle derived for rows of 4, 8 or 16 (mod 16) chunks");
    return (CPR % 16 == 8) ? ((r >> 1) & 7) : (CPR % 16 == 4 ? ((r >> 2) & 3) : (r & 15));
}
template <int CPR>
__device__ __forceinline__ int swz(int key, int chunk) {
    constexpr int G = (CPR % 16 == 8) ? 8 : (CPR % 16 == 4 ? 4 : 16);
    return (chunk & ~(G - 1)) | ((chunk ^ key) & (G - 1));
}
// byte offset of chunk `chunk` of row `row` in an image whose rows hold CPR chunks; `r` enumerates the rows of a fragment read
template <int CPR>
__device__ __forceinline__ int swz_offset(int row, int r, int chunk) { return (row * CPR + swz<CPR>(swz_key<CPR>(r), chunk)) * 16; }

// bf16 images: weights [NT*16 rows][9*CIN/8 chunks], halo [rows][AW pixels][CIN/8 chunks].  A wave owns m-tiles mt0 .. mt0+MTW-1 (16 pixels
// of one tile row each, MPR per tile row).  Fragment addresses = per-lane register (swizzled chunk offset) + immediate (tap / k-step /
// n-tile displacement):
//   A: pixel (row mt/MPR + dy, col (mt%MPR)*16 + lr + dx) of the halo, chunk cq*4 + lg of its CIN/8 chunks
//   B: weight row nt*16 + lr, chunk ks*4 + lg
template <int CIN, int MTW, int MPR, int AW>
__device__ __forceinline__ void lds_frag_offsets(int mt0, int lr, int lg, int (&offA)[MTW][3][CIN / 32], int (&offB)[CIN / 32]) {
    constexpr int CH = CIN / 8, WCH = 9 * CIN / 8, NV = CIN / 32;          // NV: swizzle variants of the chunk index
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
        const int mt = mt0 + m;
        const int col = (mt % MPR) * 16 + lr;
        const int base = ((mt / MPR) * AW + col) * CH * 16;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int v = 0; v < NV; ++v) offA[m][dx][v] = base + swz<CH>(swz_key<CH>(col + dx), v * 4 + lg) * 16;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) offB[v] = lr * WCH * 16 + swz<WCH>(swz_key<WCH>(lr), v * 4 + lg) * 16;
}

// acc = the wave's MTW x NT output tiles over all 9*CIN/32 k-steps, fragments requested one step ahead of their MFMAs.  conv3x3_lds and
// conv3x3_ws64 both run THIS loop: every output element accumulates over the same k-steps in the same order in either kernel.
template <int CIN, int NT, int MTW, int AW>
__device__ __forceinline__ void kloop_swizzled(const char* hsm, const char* wsm, const int (&offA)[MTW][3][CIN / 32], const int (&offB)[CIN / 32],
                                               f32x4 (&acc)[MTW][NT]) {
    constexpr int CH = CIN / 8, WCH = 9 * CIN / 8, NV = CIN / 32, KS = 9 * CIN / 32;
#pragma unroll
    for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[m][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto lda = [&](int ks, bf16x8(&x)[MTW]) {
        const int tap = (ks * 32) / CIN, cq = ((ks * 32) % CIN) / 32;
        const int imm = ((tap / 3) * AW + (tap % 3)) * CH * 16;
#pragma unroll
        for (int m = 0; m < MTW; ++m) x[m] = *(const bf16x8*)(hsm + offA[m][tap % 3][cq] + imm);
    };
    auto ldb = [&](int ks, bf16x8(&b)[NT]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = *(const bf16x8*)(wsm + offB[ks % NV] + nt * 16 * WCH * 16 + (ks / NV) * NV * 64);
    };
    bf16x8 aq[2][MTW], bq[2][NT];
    lda(0, aq[0]);
    ldb(0, bq[0]);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks + 1 < KS) {
            lda(ks + 1, aq[(ks + 1) & 1]);
            ldb(ks + 1, bq[(ks + 1) & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);      // requests first, then this step's MFMAs: keeps the compiler from hoisting more loads
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq[ks & 1][m], bq[ks & 1][nt], acc[m][nt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ------------------------------------------------------------------------------------------------------------------- epilogue
// Pixel functor of conv_epilogue for two consecutive m-tiles mt, mt + 1 (mt even) of a tile at (n, h0, w0) whose rows hold MPR m-tiles:
// wave-local row 0..31 -> pixel.  MPR == 1: one m-tile of each of two tile rows; otherwise 32 consecutive pixels of one tile row.
// FULL: H and W are whole multiples of the tile -- every pixel exists, so the epilogue's stores (and mask requests) are unconditional
// and the compiler can COUNT them when a prefetched chunk is consumed, instead of draining the counter, stores included.
template <int MPR, bool FULL>
struct tile_pix {
    int n, hb, wb, H, W;
    __device__ __forceinline__ tile_pix(int n_, int h0, int w0, int mt, int H_, int W_) : n(n_), hb(h0 + mt / MPR), wb(w0 + (mt % MPR) * 16), H(H_), W(W_) {}
    __device__ __forceinline__ bool operator()(int row, long& m, int& nn, int& h, int& w) const {
        nn = n;
        h = (MPR == 1) ? hb + (row >> 4) : hb;
        w = (MPR == 1) ? wb + (row & 15) : wb + row;
        m = ((long)n * H + h) * W + w;
        return FULL ? true : (h < H && w < W);
    }
};

// ----------------------------------------------------------------------------------------------------------------------- host
// Launch plan of a tile kernel: statistics groups are events of n_per_event images (forward: per-event BatchNorm statistics;
// BatchNorm-backward epilogue: every image its own group), without statistics the whole batch is one group.  A group has tpe tiles and
// is walked by bpe blocks of up to tpb consecutive tiles.  Every launcher brings its own tiles-per-block rule:
//   tile_split        tiles per block given, kept inside 1 .. tpe (conv3x3_halo, on its tile_grid)
//   tile_plan         ONE round of `slots` resident blocks over the whole launch, gy n-tile columns included (conv3x3_lds, fp8)
//   tile_plan_events  `slots` resident blocks shared out among the events, at least min_tpb tiles each (conv3x3_ws, conv3x3_ws64)
struct TilePlan {
    int tiles_w, tiles_h, ntiles, n_events, tpe, tpb, bpe, nblk;
};
static inline TilePlan tile_grid(const ConvArgs& a, int TH, int TW) {
    TilePlan p;
    p.tiles_w = (a.W + TW - 1) / TW, p.tiles_h = (a.H + TH - 1) / TH;
    p.ntiles = a.N * p.tiles_w * p.tiles_h;
    p.n_events = (a.stats != nullptr && a.n_per_event > 0) ? a.N / a.n_per_event : 1;
    p.tpe = p.ntiles / p.n_events;
    return p;
}
static inline TilePlan tile_split(TilePlan p, int tpb) {
    p.tpb = tpb < 1 ? 1 : (tpb > p.tpe ? p.tpe : tpb);
    p.bpe = (p.tpe + p.tpb - 1) / p.tpb;
    p.nblk = p.bpe * p.n_events;
    return p;
}
static inline TilePlan tile_plan(const ConvArgs& a, int TH, int TW, int gy, int slots) {
    const TilePlan g = tile_grid(a, TH, TW);
    return tile_split(g, (g.ntiles * gy + slots - 1) / slots);
}
static inline TilePlan tile_plan_events(const ConvArgs& a, int TH, int TW, int slots, int min_tpb) {
    const TilePlan g = tile_grid(a, TH, TW);
    const int bpe = slots / g.n_events < 1 ? 1 : slots / g.n_events;
    const int tpb = (g.tpe + bpe - 1) / bpe;
    return tile_split(g, tpb < min_tpb ? min_tpb : tpb);
}

// Dynamic LDS above the default limit has to be reserved once per kernel: one flag per kernel instantiation.
template <auto KERN>
static int reserve_lds(size_t bytes, const char* name) {
    static bool done = false;
    if (!done) {
        if (hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
            ieagan_set_error("%s: cannot reserve %zu bytes of LDS", name, bytes);
            return IEAGAN_ELAUNCH;
        }
        done = true;
    }
    return 0;
}

// Prologue of a launch -> template arguments: f(AFF, RELU, RS, BNB) as std::integral_constants.  BNB (the BatchNorm-backward epilogue)
// exists with the plain same-resolution prologue only -- a dgrad launch has none (conv_gather_launch checks that) -- so every (AFF, RELU)
// pair is instantiated with BNB = false, and (false, false, 0) with both.  A launcher writes its refusals in front of the call and
// answers the combinations it refuses with `if constexpr` inside f, so that they are not instantiated either.
template <int RS, typename F>
static int dispatch_prologue_rs(const ConvArgs& a, F f) {
    using T = std::true_type;
    using N = std::false_type;
    const std::integral_constant<int, RS> rs;
    const bool aff = a.src.scale != nullptr, relu = a.src.relu != 0;
    if (aff && relu) return f(T(), T(), rs, N());
    if (aff) return f(T(), N(), rs, N());
    if (relu) return f(N(), T(), rs, N());
    if constexpr (RS == 0) {
        if (a.bnb_scale != nullptr) return f(N(), N(), rs, T());
    }
    return f(N(), N(), rs, N());
}
template <typename F>
static int dispatch_prologue(const ConvArgs& a, F f) {       // a.src.rs is 0 or 1 (the 3x3 tile kernels)
    return a.src.rs == 0 ? dispatch_prologue_rs<0>(a, f) : dispatch_prologue_rs<1>(a, f);
}
