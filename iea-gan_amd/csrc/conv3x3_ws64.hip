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
#include "conv_common.h"

#define W64_H 8
#define W64_W 16

// same swizzle as conv3x3_lds.hip (rows of 8 or 72 chunks: CPR % 16 == 8)
__device__ __forceinline__ int w64_swz(int r, int chunk) { return (chunk & ~7) | ((chunk ^ ((r >> 1) & 7)) & 7); }

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
    int bid = blockIdx.x;
    {   // XCD-aware order: each XCD (blocks b, b+8, ...) walks a contiguous run of tiles
        const int q = nblk / 8, r = nblk % 8, xcd = bid % 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
    }
    const int event = bid / bpe;
    const int t0 = event * tpe + (bid - event * bpe) * tpb;
    const int t1 = min(t0 + tpb, (event + 1) * tpe);
    const int ntl = t1 - t0;
    if (ntl <= 0) return;                                    // the whole block, before any barrier

    // weights -> LDS once per block (all 8 waves)
#pragma unroll 3
    for (int idx = threadIdx.x; idx < NT * 16 * WCH; idx += 512) {
        const int row = idx / WCH, kc = idx - row * WCH;
        *(bf16x8*)(wsm + (row * WCH + w64_swz(row, kc)) * 16) = *(const bf16x8*)((const bf16*)a.w + (long)row * a.Kpad + kc * 8);
    }

    auto tile_coords = [&](int t, int& n, int& h0, int& w0) {
        n = t / (tiles_w * tiles_h);
        const int trem = t - n * tiles_w * tiles_h;
        h0 = (trem / tiles_w) * W64_H;
        w0 = (trem % tiles_w) * W64_W;
    };

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
            okmask = 0;
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                // unconditional loads (coordinates clamped into the image, the padding ring zeroed by okmask in store_tile), so that
                // the compiler can count the younger loads of the other register set instead of draining the counter
                const int idx = min(ptid + j * 256, TOT - 1);
                const int hp = idx / CH, cc = idx - hp * CH;
                const int hh = h0 - 1 + hp / AW, ww = w0 - 1 + hp % AW;
                const int hc = min(max(hh, 0), H - 1), wc = min(max(ww, 0), W - 1);
                const int sh_ = (RS == 1) ? (hc >> 1) : hc, sw_ = (RS == 1) ? (wc >> 1) : wc;
                raw[j] = *(const bf16x8*)((const bf16*)a.src.x + (((long)n * a.src.Hs + sh_) * a.src.Ws + sw_) * a.src.Cx + cc * 8);
                if (ptid + j * 256 < TOT && hh >= 0 && hh < H && ww >= 0 && ww < W) okmask |= 1u << j;
            }
        };
        auto store_tile = [&](int t, const bf16x8(&raw)[PF], unsigned okmask, char* dst) __attribute__((always_inline)) {
            int n, h0, w0;
            tile_coords(t, n, h0, w0);
            if (AFF && n != aff_n) {       // this wave's private copy of image n's scale / shift rows (wave-ordered LDS: no block barrier)
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                aff_w[lane] = a.src.scale[(long)n * a.src.aff_nstride + lane];
                aff_w[CIN + lane] = a.src.shift[(long)n * a.src.aff_nstride + lane];
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                aff_n = n;
            }
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int idx = ptid + j * 256;
                if (idx >= TOT) continue;
                const int hp = idx / CH, cc = idx - hp * CH;
                bf16x8 o = zero8();
                if (okmask & (1u << j)) {
                    if (!AFF && RELU) {
                        o = relu8(raw[j]);
                    } else if (AFF) {
                        const f32x8 sc = *(const f32x8*)(aff_w + cc * 8), sh = *(const f32x8*)(aff_w + CIN + cc * 8);
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            float v = bf2f(raw[j][i]);
                            v = v * sc[i] + sh[i];
                            if (RELU) v = fmaxf(v, 0.f);
                            o[i] = f2bf(v);
                        }
                    } else {
                        o = raw[j];
                    }
                }
                *(bf16x8*)(dst + (hp * CH + w64_swz(hp % AW, cc)) * 16) = o;
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
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                aff_w[lane] = a.bnb_scale[(long)n * a.bnb_nstride + lane];
                aff_w[CIN + lane] = a.bnb_shift[(long)n * a.bnb_nstride + lane];
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                bnb_n = n;
            }
            auto pix = [&](int row, long& m, int& nn, int& h, int& w) -> bool {      // one m-tile of each of consumer wl's two tile rows
                nn = n;
                h = h0 + 2 * wl + (row >> 4);
                w = w0 + (row & 15);
                m = ((long)n * H + h) * W + w;
                return FULL ? true : (h < H && w < W);
            };
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
    // Fragment addresses = per-lane register (swizzled chunk offset) + immediate (tap / k-step / n-tile displacement):
    //   A: pixel (row 2*wave + m + dy, col lr + dx) of the halo, chunk cq*4 + lg of its 8 chunks
    //   B: weight row nt*16 + lr, chunk ks*4 + lg
    constexpr int NV = CH / 4;
    int offA[2][3][NV];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int base = ((2 * wave + m) * AW + lr) * CH * 16;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int v = 0; v < NV; ++v) offA[m][dx][v] = base + w64_swz(lr + dx, v * 4 + lg) * 16;
    }
    int offB[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) offB[v] = lr * WCH * 16 + w64_swz(lr, v * 4 + lg) * 16;
    float* epi = epi_all + wave * EpiLds<NT>::FLOATS;
    __syncthreads();
    for (int r = 0; r < ntl; ++r) {
        const char* hsm = halo0 + (r & 1) * HALO_BYTES;
        f32x4 acc[2][NT];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[m][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        auto lda = [&](int ks, bf16x8(&x)[2]) {
            const int tap = (ks * 32) / CIN, cq = ((ks * 32) % CIN) / 32;
            const int imm = ((tap / 3) * AW + (tap % 3)) * CH * 16;
#pragma unroll
            for (int m = 0; m < 2; ++m) x[m] = *(const bf16x8*)(hsm + offA[m][tap % 3][cq] + imm);
        };
        auto ldb = [&](int ks, bf16x8(&b)[NT]) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = *(const bf16x8*)(wsm + offB[ks % NV] + nt * 16 * WCH * 16 + (ks / NV) * NV * 64);
        };
        // one-step-ahead software pipeline over the K steps (order of conv3x3_lds: bit-identical accumulation)
        bf16x8 aq[2][2], bq[2][NT];
        lda(0, aq[0]);
        ldb(0, bq[0]);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + 1 < KS) {
                lda(ks + 1, aq[(ks + 1) & 1]);
                ldb(ks + 1, bq[(ks + 1) & 1]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq[ks & 1][m], bq[ks & 1][nt], acc[m][nt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                  // the data-movement waves have finished tile r-1: the transpose buffers are free
        conv_epilogue_put<NT>(acc, epi);
        __syncthreads();                  // tile r handed over; the halo of tile r+1 is in place
    }
    if (a.stats != nullptr) {
        __syncthreads();                  // the partials of the data-movement waves are folded into red[]
        stats_add<NT, NCW>(a, 0, red, bid, event);
    }
}

template <bool AFF, bool RELU, int RS, bool BNB, bool MPF, bool FULL>
static int ws64_launch_f(const ConvArgs& a, hipStream_t st) {
    const int tiles_w = (a.W + W64_W - 1) / W64_W, tiles_h = (a.H + W64_H - 1) / W64_H;
    const int ntiles = a.N * tiles_w * tiles_h;
    const int n_events = (a.stats != nullptr && a.n_per_event > 0) ? a.N / a.n_per_event : 1;
    const int tpe = ntiles / n_events;
    int bpe = 256 / n_events;                             // one persistent block per CU; a block's tiles stay inside one event
    if (bpe < 1) bpe = 1;
    int tpb = (tpe + bpe - 1) / bpe;
    if (tpb < 4) tpb = 4;                                 // a block stages 73.7 KB of weights, as much as three halos: at least 4 tiles for them
    if (tpb > tpe) tpb = tpe;
    bpe = (tpe + tpb - 1) / tpb;
    const int nblk = bpe * n_events;
    CONV_PLAN_POINT(bpe, 1)
    auto kern = conv3x3_ws64_kernel<AFF, RELU, RS, BNB, MPF, FULL>;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, W64_LDS_BYTES) != hipSuccess) {
            ieagan_set_error("conv3x3_ws64: cannot reserve %d bytes of LDS", W64_LDS_BYTES);
            return IEAGAN_ELAUNCH;
        }
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3(nblk), dim3(512), (size_t)W64_LDS_BYTES, st, a, tiles_w, tiles_h, tpe, tpb, nblk, bpe);
    return 1;
}

template <bool AFF, bool RELU, int RS, bool BNB, bool MPF>
static int ws64_launch_c(const ConvArgs& a, hipStream_t st) {
    if (a.H % W64_H == 0 && a.W % W64_W == 0) return ws64_launch_f<AFF, RELU, RS, BNB, MPF, true>(a, st);
    return ws64_launch_f<AFF, RELU, RS, BNB, MPF, false>(a, st);
}

template <int RS>
static int ws64_launch_pro(const ConvArgs& a, hipStream_t st) {
    const bool aff = a.src.scale != nullptr, relu = a.src.relu != 0;
    if (a.mask != nullptr && (aff || relu || RS != 0)) return 0;            // a masked epilogue belongs to a dgrad launch (plain prologue)
    if (aff && relu) return ws64_launch_c<true, true, RS, false, false>(a, st);
    if (aff) return ws64_launch_c<true, false, RS, false, false>(a, st);
    if (relu) return ws64_launch_c<false, true, RS, false, false>(a, st);
    if (RS == 0 && a.bnb_scale != nullptr) return ws64_launch_c<false, false, 0, (RS == 0), (RS == 0)>(a, st);
    if (RS == 0 && a.mask != nullptr) return ws64_launch_c<false, false, 0, false, (RS == 0)>(a, st);
    return ws64_launch_c<false, false, RS, false, false>(a, st);
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
    return a.src.rs == 0 ? ws64_launch_pro<0>(a, st) : ws64_launch_pro<1>(a, st);
}
