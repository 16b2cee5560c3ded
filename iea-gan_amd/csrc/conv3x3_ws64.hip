// conv3x3_ws64: the 3x3 convolutions with Cin = Cout = 64 on the large maps (64x192, 32x96) as a wave-specialised kernel.
//
// conv3x3_lds runs the phases of a tile one after the other in all eight waves of its one block per CU (barrier -> halo to LDS ->
// barrier -> K loop -> barrier -> epilogue through LDS buffers that alias the halo -> stores): the MFMA pipe idles while the block
// stages and stores, the memory system sees no stores during the K loop.  Here the block keeps the LDS images of conv3x3_lds
// (weights and halo UNPADDED with the XOR chunk swizzle) and the roles of conv3x3_ws:
//   * waves 4..7 (producers) move all the data: two tiles of raw halo chunks in flight in registers, prologue (BatchNorm apply /
//     ReLU / nearest x2 up-sample / zero padding) and the LDS write of tile t+1 into the other halo buffer, AND the second half of
//     the shared epilogue of tile t-1 (transpose buffer -> bias / ReLU mask / BatchNorm backward / statistics -> stores), while
//   * waves 0..3 (consumers) run the K loop of tile t and put their accumulators into the transpose buffers -- they never wait for
//     global memory.  A consumer owns two 16-pixel m-tiles (two rows of the 8x16-pixel tile) x 4 n-tiles: the per-wave register
//     tile, K order and fragment mapping of conv3x3_lds, so every output element accumulates in the same order and the outputs
//     are bit-identical.  The transpose buffers alias nothing.
//     (With the whole epilogue in the consumers the kernel only tied conv3x3_lds: four waves then pay the store / mask latency
//      that eight waves shared before -- 64x192 at N = 40: 47.8 vs 47.8 us with BatchNorm prologue, 71.4 vs 61.1 us BatchNorm-backward dgrad.)
// Two block barriers per tile (around the hand-over of the accumulators), no flag or spin-wait anywhere.  LDS: weights 73.7 KB + 2 x 23.0 KB halo + 4 x 8.7 KB epilogue +
// 4 KB of static rows = 155 KB, one persistent block per CU.
#include "common.h"
#include "conv_args.h"
#include "conv3x3_tile.h"

#define W64_H 8
#define W64_W 16

constexpr int W64_CIN = 64, W64_NT = 4, W64_NCW = 4;
constexpr int W64_K = 9 * W64_CIN, W64_WCH = W64_K / 8, W64_CH = W64_CIN / 8;
constexpr int W64_AW = W64_W + 2, W64_AH = W64_H + 2;
constexpr int W64_W_BYTES = W64_NT * 16 * W64_K * 2;
constexpr int W64_HALO_BYTES = W64_AH * W64_AW * W64_CIN * 2;
constexpr int W64_EPI_BYTES = W64_NCW * EpiLds<W64_NT>::FLOATS * 4;
constexpr int W64_LDS_BYTES = W64_W_BYTES + 2 * W64_HALO_BYTES + W64_EPI_BYTES;
static_assert(W64_NCW * STATS_SX_FLOATS * 4 <= W64_EPI_BYTES, "the statistics fold scratch reuses the epilogue buffers");
static_assert(W64_LDS_BYTES + 4 * 1024 <= 160 * 1024, "LDS image + static rows must fit one CU");

// FULL: H % 8 == 0 and W % 16 == 0 -- stores and mask requests are unconditional, so the compiler can count them.
// MPF: the launch has a ReLU mask / BatchNorm input (a.mask != nullptr): its chunks are requested one tile ahead.
template <bool AFF, bool RELU, int RS, bool BNB, bool MPF, bool FULL>
__global__ __launch_bounds__(512, 1) void conv3x3_ws64_kernel(ConvArgs a, int tiles_w, int tiles_h, int tpe, int tpb, int nblk, int bpe) {
    constexpr int CIN = W64_CIN, NT = W64_NT, NCW = W64_NCW, AW = W64_AW, CH = W64_CH, WCH = W64_WCH, K = W64_K;
    constexpr int KS = K / 32;
    constexpr int TOT = W64_AH * AW * CH;                    // 16-byte chunks of one halo
    constexpr int PF = (TOT + 255) / 256;                    // chunks per producer thread and tile
    constexpr int HALO_BYTES = W64_HALO_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    __shared__ float red[NCW * NT * 16 * 2];
    __shared__ __attribute__((aligned(32))) float aff_all[4 * 2 * CIN];      // per producer wave: [0, 64) scale, [64, 128) shift of its current image
    char* wsm = smem_all;                                    // [64][72 chunks], swizzled
    char* halo0 = smem_all + W64_W_BYTES;                    // two halo buffers [10][18][8 chunks], swizzled
    float* epi_all = (float*)(halo0 + 2 * HALO_BYTES);       // NCW x EpiLds<NT>::FLOATS (later: the statistics fold scratch)

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool consumer = wave < NCW;
    const int lr = lane & 15, lg = lane >> 4;
    const int H = a.H, W = a.W;
    const TileRun run = tile_run(nblk, 1, bpe, tpe, tpb);
    const int t0 = run.t0, t1 = run.t1, ntl = t1 - t0;
    if (ntl <= 0) return;                                    // the whole block, before any barrier

    // weights -> LDS once per block (all 8 waves)
#pragma unroll 3
    for (int idx = threadIdx.x; idx < NT * 16 * WCH; idx += 512) {
        const int row = idx / WCH, kc = idx - row * WCH;
        *(bf16x8*)(wsm + swz_offset<WCH>(row, row, kc)) = *(const bf16x8*)((const bf16*)a.w + (long)row * a.Kpad + kc * 8);
    }

    auto tile_coords = [&](int t, int& n, int& h0, int& w0) { tile_origin<W64_H, W64_W>(t, tiles_w, tiles_h, n, h0, w0); };

    // The two roles are separate loops: their register live ranges do not overlap and the kernel is allocated max(producer,
    // consumer) registers.  Both execute the same barriers: one after the preamble, two per tile, one for the statistics flush.
    if (!consumer) {
        // -------------------------------------------------------------------------------------- producers
        const int ptid = threadIdx.x - NCW * 64;
        bf16x8 rawA[PF], rawB[PF];
        unsigned okA = 0, okB = 0;
        float* aff_w = aff_all + (wave & 3) * 2 * CIN;
        int aff_n = -1;
        auto load_tile = [&](int t, bf16x8(&raw)[PF], unsigned& okmask) __attribute__((always_inline)) {
            int n, h0, w0;
            tile_coords(t, n, h0, w0);
            halo_request<RS, CH, AW, TOT, 256>(a.src, H, W, n, h0, w0, ptid, raw, okmask);
        };
        auto store_tile = [&](int t, const bf16x8(&raw)[PF], unsigned okmask, char* dst) __attribute__((always_inline)) {
            int n, h0, w0;
            tile_coords(t, n, h0, w0);
            if (AFF && n != aff_n) {       // this wave's private copy of image n's scale / shift rows (wave-ordered LDS: no block barrier)
                wave_fence();
                aff_w[lane] = a.src.scale[(long)n * a.src.aff_nstride + lane];
                aff_w[CIN + lane] = a.src.shift[(long)n * a.src.aff_nstride + lane];
                wave_fence();
                aff_n = n;
            }
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int idx = ptid + j * 256;
                if (idx >= TOT) continue;
                const int hp = idx / CH, cc = idx - hp * CH;
                *(bf16x8*)(dst + swz_offset<CH>(hp, hp % AW, cc)) = prologue_chunk<AFF, RELU>(raw[j], okmask & (1u << j), aff_w + cc * 8, aff_w + CIN + cc * 8);
            }
        };
        // ---- the epilogue of tile r-1 runs HERE, next to the consumers' K loop of tile r: the consumers only put their accumulators
        // into the transpose buffers, this wave finishes the buffer of consumer wave - 4 (bias, ReLU mask / BatchNorm backward,
        // statistics partials, 16-byte stores).  The mask chunks of a tile are requested one step ahead of their use.
        const int wl = wave - NCW;
        const float* epi = epi_all + wl * EpiLds<NT>::FLOATS;
        constexpr int CPP = NT * 2, EIT = (32 * CPP) / 64;
        const int ecc = lane % CPP;
        float s1[8], s2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s1[i] = s2[i] = 0.f;
        float bias_r[8];
        load_bias8<NT>(a, 0, bias_r);
        bf16x8 mk_cur[EIT], mk_nxt[EIT];
        int bnb_n = -1;
        // (the launcher sends launches with a residual operand to conv3x3_lds: with the pointers known to be null the residual paths of
        //  the shared epilogue, and the waits they would put in front of the stores, are not compiled in)
        ConvArgs ae = a;
        ae.ra = nullptr;
        ae.rb = nullptr;
        if (!MPF) ae.mask = nullptr;
        auto mask_request = [&](int t, bf16x8(&mk)[EIT]) __attribute__((always_inline)) {
            int n, h0, w0;
            tile_coords(t, n, h0, w0);
#pragma unroll
            for (int it = 0; it < EIT; ++it) {
                const int row = (it * 64 + lane) / CPP;
                const int hh = h0 + 2 * wl + (row >> 4), ww = w0 + (row & 15);
                if (FULL) {
                    mk[it] = *(const bf16x8*)((const bf16*)a.mask + (((long)n * H + hh) * W + ww) * CIN + ecc * 8);
                } else {
                    mk[it] = zero8();
                    if (hh < H && ww < W) mk[it] = *(const bf16x8*)((const bf16*)a.mask + (((long)n * H + hh) * W + ww) * CIN + ecc * 8);
                }
            }
        };
        auto finish = [&](int t) __attribute__((always_inline)) {
            int n, h0, w0;
            tile_coords(t, n, h0, w0);
            if (BNB && n != bnb_n) {       // this wave's private copy of image n's BatchNorm-backward rows (a BNB launch has no prologue rows)
                wave_fence();
                aff_w[lane] = a.bnb_scale[(long)n * a.bnb_nstride + lane];
                aff_w[CIN + lane] = a.bnb_shift[(long)n * a.bnb_nstride + lane];
                wave_fence();
                bnb_n = n;
            }
            const tile_pix<1, FULL> pix(n, h0, w0, 2 * wl, H, W);       // one m-tile of each of consumer wl's two tile rows
            if constexpr (BNB) conv_epilogue_finish<true, NT>(ae, epi, 0, pix, s1, s2, bias_r, mk_cur, aff_w);
            else if constexpr (MPF) conv_epilogue_finish<false, NT>(ae, epi, 0, pix, s1, s2, bias_r, mk_cur);
            else conv_epilogue_finish<false, NT>(ae, epi, 0, pix, s1, s2, bias_r, nullptr);
        };
        // step r (next to the consumers' K loop of tile r): tile r+1 -> the other halo buffer, tile r+3 requested into the register
        // set that has just been drained (past the block's last tile the last tile is requested again and never stored), the mask
        // of tile r requested, tile r-1 finished.  Everything before the first of the step's two barriers; between them the
        // consumers put tile r into the transpose buffers.
        auto step = [&](int r, bf16x8(&raw)[PF], unsigned& okmask) __attribute__((always_inline)) {
            if (r + 1 < ntl) store_tile(t0 + r + 1, raw, okmask, halo0 + ((r + 1) & 1) * HALO_BYTES);
            load_tile(t0 + min(r + 3, ntl - 1), raw, okmask);
            if (r > 0) {
                if (MPF) mask_request(t0 + r, mk_nxt);
                finish(t0 + r - 1);
                if (MPF) {
#pragma unroll
                    for (int i = 0; i < EIT; ++i) mk_cur[i] = mk_nxt[i];
                }
            }
            __syncthreads();              // the transpose buffers are free
            __syncthreads();              // tile r is in them; the halo of tile r+1 is in place
        };
        load_tile(t0, rawA, okA);
        store_tile(t0, rawA, okA, halo0);
        load_tile(t0 + min(1, ntl - 1), rawB, okB);           // set B: odd tiles
        load_tile(t0 + min(2, ntl - 1), rawA, okA);           // set A: even tiles
        if (MPF) mask_request(t0, mk_cur);
        __syncthreads();
        step(0, rawB, okB);                         // tile 1 is odd -> set B
        for (int r = 1; r < ntl; r += 2) {
            step(r, rawA, okA);                     // tile r+1 is even -> set A
            if (r + 1 >= ntl) break;
            step(r + 1, rawB, okB);
        }
        finish(t1 - 1);
        if (a.stats != nullptr) {
            stats_fold<NT>(s1, s2, red, epi_all + wl * EpiLds<NT>::FLOATS, wl);       // (this wave's own transpose buffer as fold scratch)
            __syncthreads();
        }
        return;
    }

    // ------------------------------------------------------------------------------------------ consumers
    // the per-wave register tile, fragment mapping and K loop of conv3x3_lds: two m-tiles (tile rows 2*wave, 2*wave + 1) x 4 n-tiles
    int offA[2][3][CIN / 32], offB[CIN / 32];
    lds_frag_offsets<CIN, 2, 1, AW>(2 * wave, lr, lg, offA, offB);
    float* epi = epi_all + wave * EpiLds<NT>::FLOATS;
    __syncthreads();
    for (int r = 0; r < ntl; ++r) {
        const char* hsm = halo0 + (r & 1) * HALO_BYTES;
        f32x4 acc[2][NT];
        kloop_swizzled<CIN, NT, 2, AW>(hsm, wsm, offA, offB, acc);
        __syncthreads();                  // the data-movement waves have finished tile r-1: the transpose buffers are free
        conv_epilogue_put<NT>(acc, epi);
        __syncthreads();                  // tile r handed over; the halo of tile r+1 is in place
    }
    if (a.stats != nullptr) {
        __syncthreads();                  // the partials of the data-movement waves are folded into red[]
        stats_add<NT, NCW>(a, 0, red, run.bid, run.event);
    }
}

template <bool AFF, bool RELU, int RS, bool BNB, bool MPF, bool FULL>
static int ws64_launch_f(const ConvArgs& a, hipStream_t st) {
    // one persistent block per CU; a block's tiles stay inside one event.  A block stages 73.7 KB of weights, as much as three halos:
    // at least 4 tiles for them
    const TilePlan p = tile_plan_events(a, W64_H, W64_W, 256, 4);
    CONV_PLAN_POINT(p.bpe, 1)
    constexpr auto kern = conv3x3_ws64_kernel<AFF, RELU, RS, BNB, MPF, FULL>;
    if (reserve_lds<kern>(W64_LDS_BYTES, "conv3x3_ws64") != 0) return IEAGAN_ELAUNCH;
    hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(512), (size_t)W64_LDS_BYTES, st, a, p.tiles_w, p.tiles_h, p.tpe, p.tpb, p.nblk, p.bpe);
    return 1;
}

template <bool AFF, bool RELU, int RS, bool BNB, bool MPF>
static int ws64_launch_c(const ConvArgs& a, hipStream_t st) {
    if (a.H % W64_H == 0 && a.W % W64_W == 0) return ws64_launch_f<AFF, RELU, RS, BNB, MPF, true>(a, st);
    return ws64_launch_f<AFF, RELU, RS, BNB, MPF, false>(a, st);
}

// Tiles (8x16 pixels) from which a launch goes to this kernel, chosen by same-box alternation against conv3x3_lds at N = 40 (DESIGN
// section 3, profiles/conv3x3_ws64.json): 64x192 (3840 tiles, 15 per block) is faster in every variant; at 32x96 (960 tiles, 4 per block)
// the forms without a BatchNorm prologue are faster (bare-ReLU forward, ReLU-mask and BatchNorm-backward dgrad) while the two with it
// only tie -- the prologue makes the data-movement waves, not the K loop, the longer side of a step -- and stay on conv3x3_lds.
#ifndef W64_MIN_TILES
#define W64_MIN_TILES 512
#endif
#ifndef W64_MIN_TILES_AFF
#define W64_MIN_TILES_AFF 2048
#endif

// 1 = launched, 0 = not applicable (the caller goes on to conv3x3_lds), < 0 = error
int conv3x3_ws64_launch(const ConvArgs& a, hipStream_t st) {
    if (a.flags & (IEAGAN_CONV_NO_WS64 | IEAGAN_CONV_FP8)) return 0;
    if (a.taps != 9 || a.Cin != 64 || a.Cout != 64 || (a.src.rs != 0 && a.src.rs != 1) || a.Kpad != 9 * 64 || a.src.Cx % 8 != 0) return 0;
    if (a.H < W64_H || a.W < W64_W || a.ra != nullptr || a.rb != nullptr) return 0;
    const long tiles = (long)a.N * ((a.W + W64_W - 1) / W64_W) * ((a.H + W64_H - 1) / W64_H);
    if (tiles < (a.src.scale != nullptr ? W64_MIN_TILES_AFF : W64_MIN_TILES) && !(a.flags & IEAGAN_CONV_FORCE_WS64)) return 0;
    if (a.mask != nullptr) {               // a masked epilogue belongs to a dgrad launch: plain same-resolution prologue, mask chunks prefetched
        if (a.src.scale != nullptr || a.src.relu != 0 || a.src.rs != 0) return 0;
        return a.bnb_scale != nullptr ? ws64_launch_c<false, false, 0, true, true>(a, st) : ws64_launch_c<false, false, 0, false, true>(a, st);
    }
    return dispatch_prologue(a, [&](auto AFF, auto RELU, auto RS, auto BNB) {
        if constexpr (BNB()) return 0;     // (the BatchNorm-backward epilogue has its input as mask: taken above)
        else return ws64_launch_c<AFF(), RELU(), RS(), false, false>(a, st);
    });
}
