// d_stem: the first discriminator block's input side as ONE forward and ONE backward kernel (one per kind of backward pass).
//
// Reference (model.py:902-909, 534-557 with the shipped config): h0 = input_conv(x) (3x3, 1 -> 32 channels at 256x768), then the first
// DBlock (no pre-activation) reads h0 three times -- conv1 (1x1, 32 -> 16), conv_sc on AvgPool2d(h0) (1x1, 32 -> 32) and the pooled
// identity shortcut -- 503 MB per read at N = 40, 25 % of the discriminator's forward traffic.  h0 is a K = 9 convolution of a
// 31 MB single-channel image: cheaper to recompute than to move.  So
//   d_stem_fwd:  img -> { h1 = conv1(h0), p0 = AvgPool2d(h0), sc = conv_sc(p0) }     h0 never reaches HBM (writes 504 MB instead of
//                2.4 GB of reads + writes); conv4 of the block then takes p0 as a same-resolution shortcut operand.
//   d_stem_bwd:  (img, dh1, dp0) -> dW_in, db_in, dW1, db1     with h0 recomputed and dh0 = dh1 W1 + 0.25 expand(dp0) formed in LDS only
//                (replaces conv1's dgrad + wgrad and input_conv's wgrad: 1.9 GB -> 0.41 GB per backward pass).  D-phase passes only.
//   d_stem_dimg: (dh1, dp0) -> d img     the G-phase pass (weights frozen, d img wanted): dh0 as above, formed in registers and fed
//                straight into the transposed input_conv (replaces conv1's dgrad + conv_Cto1: 1.4 GB -> 0.41 GB).
// Numerics follow the separate kernels: the image enters the matrix cores as bf16 high + low parts against bf16 weights
// (conv_c1.hip), h0 / p0 are rounded to bf16 where the separate path stored them, every accumulation is fp32.
// Tile = 8 x 32 pixels per block, wave w owns rows 2w, 2w+1 (= one pooled row); everything after the halo load is wave-private.
// Every pixel-by-channel product has the weights as the MFMA's A operand and the pixels as its B operand, so that an accumulator
// lane holds four consecutive channels of ONE pixel: bias, rounding and the store (8 bytes to LDS for h0 / dh0; 16 bytes to global
// memory for h1 / sc, after lane groups 16 apart exchanged halves of two tiles) happen in registers, with no transpose through LDS.
// The image halo is split into its bf16 high and low parts once per halo element, when it is staged.
#include "common.h"
#include "conv_args.h"

#define ST_TH 8
#define ST_TW 32
#define ST_C0 32          // input_conv output channels
#define ST_C1 16          // conv1 output channels (hidden)
#define ST_CS 32          // conv_sc output channels
#define ST_XS 48          // bf16 row stride of the 32-channel LDS tiles: 96 bytes = an odd multiple of 32 (conflict-free transposed reads)

struct DStemArgs {
    const float* img;     // fp32 [N, H, W]
    int N, H, W;
    const float* w_in;    // fp32 [9][32]   input_conv weight / sigma (tap-major)
    const float* b_in;    // [32]
    const void* w1;       // bf16 [16][32]  conv1 forward pack (k = cin)
    const float* b1;      // [16]
    const void* wsc;      // bf16 [32][32]  conv_sc forward pack
    const float* bsc;     // [32]
    void* h1;             // bf16 [N, H, W, 16]
    void* p0;             // bf16 [N, H/2, W/2, 32]
    void* sc;             // bf16 [N, H/2, W/2, 32]
    // backward
    const void* dh1;      // bf16 [N, H, W, 16]
    const void* dp0;      // bf16 [N, H/2, W/2, 32]
    const void* w1_bwd;   // bf16 [32][32]  conv1 transposed pack ([cin][k = cout], 16 used)
    float* dw_in;         // fp32 [9][32]        accumulated
    float* db_in;         // fp32 [32 repl][32]  accumulated (replica = block % 32)
    float* dw1;           // fp32 [16][32]       accumulated
    float* db1;           // fp32 [32 repl][16]  accumulated
    float* dimg;          // fp32 [N, H, W]      (d_stem_dimg)
};

#define ST_HW (ST_TW + 4)  // row stride of the halo image (words)
#define ST_HN ((((ST_TH + 2) * (ST_TW + 2)) + 255) / 256)                  // halo values per thread
// The image halo in LDS: one word per element, bf16(v) in the lower and bf16(v - bf16(v)) in the upper half.  Two words make one dword
// of a bf16 fragment with a single byte permute, whose selector picks the high or the low parts.
typedef unsigned StHalo[ST_HW];
typedef const volatile __attribute__((address_space(3))) unsigned* StHaloWords;    // volatile: plain aligned dword reads, never merged
#define ST_SEL_HI 0x05040100u
#define ST_SEL_LO 0x07060302u
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct StTile {
    int n, y0, x0;
};
__device__ __forceinline__ StTile st_tile(int tile, int tiles_w, int tiles_h) {
    StTile t;
    t.n = tile / (tiles_w * tiles_h);
    const int trem = tile - t.n * tiles_w * tiles_h;
    t.y0 = (trem / tiles_w) * ST_TH;
    t.x0 = (trem % tiles_w) * ST_TW;
    return t;
}

// The image halo of a tile (340 floats) into ST_HN registers per thread: unconditional loads from clamped coordinates, the padding
// ring recorded in a mask.
__device__ __forceinline__ void st_request_halo(const float* img, int H, int W, StTile t, float (&hn)[ST_HN], unsigned& hok) {
    constexpr int AWH = ST_TW + 2, AHH = ST_TH + 2;
    const float* im = img + (long)t.n * H * W;
    hok = 0;
#pragma unroll
    for (int j = 0; j < ST_HN; ++j) {
        const int i = min((int)threadIdx.x + j * 256, AHH * AWH - 1);
        const int qy = i / AWH, qx = i - qy * AWH;
        const int yy = t.y0 - 1 + qy, xx = t.x0 - 1 + qx;
        hn[j] = im[(long)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)];
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) hok |= 1u << j;
    }
}

// The requested halo into LDS: the high / low split of the image is done here, once per halo element.
__device__ __forceinline__ void st_stage_halo(StHalo* halo, const float (&hn)[ST_HN], unsigned hok) {
    constexpr int AWH = ST_TW + 2, AHH = ST_TH + 2;
#pragma unroll
    for (int j = 0; j < ST_HN; ++j) {
        const int i = threadIdx.x + j * 256;
        if (i < AHH * AWH) {
            const float v = (hok & (1u << j)) ? hn[j] : 0.f;
            const bf16 hi = f2bf(v), lo = f2bf(v - bf2f(hi));
            halo[i / AWH][i % AWH] = (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
        }
    }
}

// h0 of this wave's two tile rows (64 pixels x 32 channels, + bias, rounded to bf16) into h0s[(rr*32 + col)][ST_XS].
// The weights are the MFMA's A operand and the 3x3 patches its B operand: D[channel 4 lg + r][pixel lr], so a lane holds four
// consecutive channels of one pixel and writes them with one 8-byte store per n-tile.  k = 8 lg + j: lane groups 0 / 1 carry taps
// 0..7 / 8 of the high parts, groups 2 / 3 the same taps of the low parts (k 9..15 and 25..31 are zero).  The 4 x 3 halo words over
// a lane's column serve both tile rows.
__device__ __forceinline__ void st_h0_tile(const StHalo* halo, int wave, int lane, const bf16x8 (&wfrag)[2], const float (&bq)[2][4], bf16* h0s) {
    const int lr = lane & 15, lg = lane >> 4;
    const bool odd = lg & 1;
    const unsigned sel = (lg >> 1) ? ST_SEL_LO : ST_SEL_HI;
    const int o0 = odd ? 2 * ST_HW + 2 : 0;                      // the word of k = 8 lg: tap 0, in the odd groups tap 8
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        StHaloWords b = (StHaloWords)&halo[2 * wave][half * 16 + lr];
        unsigned w[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) w[r][dx] = b[r * ST_HW + dx];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            u32x4 pw;
            pw[0] = __builtin_amdgcn_perm(odd ? 0u : w[rr][1], b[rr * ST_HW + o0], sel);                     // taps 0, 1 | tap 8
            pw[1] = odd ? 0u : __builtin_amdgcn_perm(w[rr + 1][0], w[rr][2], sel);
            pw[2] = odd ? 0u : __builtin_amdgcn_perm(w[rr + 1][2], w[rr + 1][1], sel);
            pw[3] = odd ? 0u : __builtin_amdgcn_perm(w[rr + 2][1], w[rr + 2][0], sel);
            const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfrag[nt], pf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                bf16x4 ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[r] = f2bf(d[r] + bq[nt][r]);
                *(bf16x4*)(h0s + (rr * 32 + half * 16 + lr) * ST_XS + nt * 16 + 4 * lg) = ov;
            }
        }
    }
    wave_fence();
}

// Two accumulator tiles A, B with a lane's four bf16 values each (rows 4 lg .. 4 lg + 3 of column lr) -> 16 bytes per lane: lane group
// lg ends up with rows 8 (lg >> 1) .. + 7 of tile (lg & 1).  v_permlane16_swap exchanges the odd 16-lane rows of its first operand with
// the even rows of its second.
__device__ __forceinline__ u32x4 st_pair16(bf16x4 ta, bf16x4 tb) {
    u32x2 x = __builtin_bit_cast(u32x2, ta), y = __builtin_bit_cast(u32x2, tb);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const u32x2 r = __builtin_amdgcn_permlane16_swap(x[k], y[k], false, false);
        x[k] = r[0];
        y[k] = r[1];
    }
    return (u32x4){x[0], x[1], y[0], y[1]};
}

__device__ __forceinline__ void st_in_frags(const float* w_in, int lane, bf16x8 (&bfrag)[2]) {
    const int lr = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int tap = (lg & 1) * 8 + j;
            bfrag[nt][j] = f2bf(tap < 9 ? w_in[tap * ST_C0 + nt * 16 + lr] : 0.f);
        }
}

// the four bias values of a lane's channels nt*16 + 4 lg + r
__device__ __forceinline__ void st_bias4(const float* b, int lg, int nt, float (&q)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = b[nt * 16 + 4 * lg + r];
}

__global__ __launch_bounds__(256, 4) void d_stem_fwd_kernel(DStemArgs a, int tiles_w, int tiles_h) {
    __shared__ __attribute__((aligned(16))) StHalo halo[ST_TH + 2];
    __shared__ __attribute__((aligned(16))) bf16 h0t[4][64 * ST_XS];
    __shared__ __attribute__((aligned(16))) bf16 p0t[4][16 * ST_XS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int H = a.H, W = a.W, Hp = H >> 1, Wp = W >> 1;
    bf16x8 bin[2];
    st_in_frags(a.w_in, lane, bin);
    const int cc4 = lane & 3;
    float bq[2][4], bsq[2][4], b1q[4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        st_bias4(a.b_in, lg, nt, bq[nt]);
        st_bias4(a.bsc, lg, nt, bsq[nt]);
    }
    st_bias4(a.b1, lg, 0, b1q);
    // conv1: A[row = cout lr][k = cin] = w1[lr][lg*8 ..];  conv_sc: two n-tiles of the [32][32] pack
    const bf16x8 w1f = *(const bf16x8*)((const bf16*)a.w1 + lr * 32 + lg * 8);
    bf16x8 wsf[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) wsf[nt] = *(const bf16x8*)((const bf16*)a.wsc + (nt * 16 + lr) * 32 + lg * 8);
    bf16* h0s = h0t[wave];
    bf16* p0s = p0t[wave];
    const int ntiles = a.N * tiles_w * tiles_h;
    const int per = (ntiles + gridDim.x - 1) / gridDim.x;
    const int tile_end = min((int)(blockIdx.x + 1) * per, ntiles);
    // The image halo of tile t+1 is requested into two registers per thread right after tile t's halo went to LDS, and every global
    // access of the loop is unconditional (coordinates clamped, the padding ring zeroed through a mask; all 64 lanes store): this
    // kernel writes 0.5 GB per launch, and a halo load that follows the stores in program order -- or that the compiler cannot
    // count past -- waits for every one of them (stores count on vmcnt on gfx9).
    float hn[ST_HN];
    unsigned hok = 0;
    const int tile_begin = blockIdx.x * per;
    if (tile_begin < tile_end) st_request_halo(a.img, H, W, st_tile(tile_begin, tiles_w, tiles_h), hn, hok);
    for (int tile = tile_begin; tile < tile_end; ++tile) {
        const StTile t = st_tile(tile, tiles_w, tiles_h);
        __syncthreads();                                           // the previous tile is done with halo / h0s / p0s
        st_stage_halo(halo, hn, hok);
        __syncthreads();
        st_request_halo(a.img, H, W, st_tile(min(tile + 1, tile_end - 1), tiles_w, tiles_h), hn, hok);   // (last tile: itself, unused)
        st_h0_tile(halo, wave, lane, bin, bq, h0s);
        // ---- conv1: h1[px][16] = h0[px][32] W1^T + b1, one K step; D[cout 4 lg + r][pixel lr] goes from registers to global memory:
        // the two 16-pixel tiles of a row pair up, one 16-byte store per lane covers the row's 1024 contiguous bytes
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            bf16x4 ov[2];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const bf16x8 hf = *(const bf16x8*)(h0s + (rr * 32 + half * 16 + lr) * ST_XS + lg * 8);
                const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1f, hf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[half][r] = f2bf(d[r] + b1q[r]);
            }
            bf16* row = (bf16*)a.h1 + (((long)t.n * H + t.y0 + 2 * wave + rr) * W + t.x0) * ST_C1;
            *(u32x4*)(row + ((lg & 1) * 16 + lr) * ST_C1 + (lg >> 1) * 8) = st_pair16(ov[0], ov[1]);
        }
        // ---- p0 = 2x2 average of the bf16 h0 (as the pooled prologue of the separate kernels: fp32 sum, one rounding)
        const int yp = (t.y0 >> 1) + wave;
        {
            const int ppx = lane >> 2;                             // 16 pooled pixels x 4 chunks
            const bf16* b0 = h0s + (2 * ppx) * ST_XS + cc4 * 8;
            const bf16x8 t0 = *(const bf16x8*)b0, t1 = *(const bf16x8*)(b0 + ST_XS), t2 = *(const bf16x8*)(b0 + 32 * ST_XS),
                         t3 = *(const bf16x8*)(b0 + 33 * ST_XS);
            bf16x8 pv;
#pragma unroll
            for (int i = 0; i < 8; ++i) pv[i] = f2bf(0.25f * (bf2f(t0[i]) + bf2f(t1[i]) + bf2f(t2[i]) + bf2f(t3[i])));
            *(bf16x8*)(p0s + ppx * ST_XS + cc4 * 8) = pv;
            *(bf16x8*)((bf16*)a.p0 + (((long)t.n * Hp + yp) * Wp + (t.x0 >> 1) + ppx) * ST_C0 + cc4 * 8) = pv;
        }
        wave_fence();
        // ---- conv_sc: sc[ppx][32] = p0[ppx][32] Wsc^T + bsc, D[cout nt*16 + 4 lg + r][pooled pixel lr]
        {
            const bf16x8 pf = *(const bf16x8*)(p0s + lr * ST_XS + lg * 8);
            bf16* dst = (bf16*)a.sc + (((long)t.n * Hp + yp) * Wp + (t.x0 >> 1) + lr) * ST_CS;
            bf16x4 ov[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wsf[nt], pf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[nt][r] = f2bf(d[r] + bsq[nt][r]);
            }
            *(u32x4*)(dst + (lg & 1) * 16 + (lg >> 1) * 8) = st_pair16(ov[0], ov[1]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backward (weight gradients only)
// ------------------------------------------------------------------------------------------------
// K(pixel)-major fragments of one halo row: the high and the low parts of the 8 consecutive values from column c0 on
__device__ __forceinline__ void st_row8(const unsigned* row, int c0, bf16x8& hi, bf16x8& lo) {
    StHaloWords w = (StHaloWords)(row + c0);
    u32x4 h, l;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned w0 = w[2 * k], w1 = w[2 * k + 1];
        h[k] = __builtin_amdgcn_perm(w1, w0, ST_SEL_HI);
        l[k] = __builtin_amdgcn_perm(w1, w0, ST_SEL_LO);
    }
    hi = __builtin_bit_cast(bf16x8, h);
    lo = __builtin_bit_cast(bf16x8, l);
}

__global__ __launch_bounds__(256, 2) void d_stem_bwd_kernel(DStemArgs a, int tiles_w, int tiles_h) {
    __shared__ __attribute__((aligned(16))) StHalo halo[ST_TH + 2];
    __shared__ __attribute__((aligned(16))) bf16 h0t[4][64 * ST_XS];
    __shared__ __attribute__((aligned(16))) bf16 d0t[4][64 * ST_XS];       // dh0
    __shared__ __attribute__((aligned(16))) bf16 g1t[4][64 * ST_C1];       // dh1 (32-byte rows)
    __shared__ __attribute__((aligned(16))) bf16 dpt[4][16 * ST_XS];       // dp0 of the wave's pooled row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int H = a.H, W = a.W, Hp = H >> 1, Wp = W >> 1;
    bf16x8 bin[2];
    st_in_frags(a.w_in, lane, bin);
    const int cc4 = lane & 3;
    float bq[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) st_bias4(a.b_in, lg, nt, bq[nt]);
    // dgrad of conv1: dh0[px][cin] = sum_cout dh1[px][cout] W1[cout][cin]: A[row = cin lr][k = cout] = w1_bwd[nt*16 + lr][lg*8 ..], 16 k used
    bf16x8 w1b[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) w1b[nt] = (lg < 2) ? *(const bf16x8*)((const bf16*)a.w1_bwd + (nt * 16 + lr) * 32 + lg * 8) : zero8();
    bf16* h0s = h0t[wave];
    bf16* d0s = d0t[wave];
    bf16* g1s = g1t[wave];
    bf16* dps = dpt[wave];
    f32x4 aw1[2], awin[2], ab1;                                  // dW1 [16 couts][32 cin], dW_in [16 "taps" (9 + the bias row)][32], db1 [16]
    ab1 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) aw1[nj] = awin[nj] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;
    const int ntiles = a.N * tiles_w * tiles_h;
    const int per = (ntiles + gridDim.x - 1) / gridDim.x;
    const int tile_end = min((int)(blockIdx.x + 1) * per, ntiles);
    // Every operand of tile t+1 -- dh1 (64 pixels x 2 chunks per wave), dp0 (16 pooled pixels x 4 chunks), the image halo -- is
    // requested into registers (unconditionally, halo coordinates clamped) once tile t's copies sit in LDS: the 60 tiles of a block
    // were a chain of exposed load latencies.
    bf16x8 rg[2], rp;
    float hn[ST_HN];
    unsigned hok = 0;
    auto request = [&](int tile) {
        const StTile t = st_tile(tile, tiles_w, tiles_h);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int item = j * 64 + lane, p = item >> 1, cc = item & 1;
            const int y = t.y0 + 2 * wave + (p >> 5), x = t.x0 + (p & 31);
            rg[j] = *(const bf16x8*)((const bf16*)a.dh1 + (((long)t.n * H + y) * W + x) * ST_C1 + cc * 8);
        }
        {
            const int ppx = lane >> 2;
            rp = *(const bf16x8*)((const bf16*)a.dp0 + (((long)t.n * Hp + (t.y0 >> 1) + wave) * Wp + (t.x0 >> 1) + ppx) * ST_C0 + cc4 * 8);
        }
        st_request_halo(a.img, H, W, t, hn, hok);
    };
    // the dW_in operand of this lane: row lr < 9 = tap lr of the patch (high and low parts), row 9 = ones (-> db_in), rows 10..15 zero
    const int wtap = min(lr, 8), wdy = wtap / 3, wdx = wtap - 3 * wdy;
    const int tile_begin = blockIdx.x * per;
    if (tile_begin < tile_end) request(tile_begin);
    for (int tile = tile_begin; tile < tile_end; ++tile) {
        __syncthreads();                                           // the previous tile is done with halo / g1s / dps
        st_stage_halo(halo, hn, hok);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int item = j * 64 + lane, p = item >> 1, cc = item & 1;
            *(bf16x8*)(g1s + p * ST_C1 + cc * 8) = rg[j];
        }
        *(bf16x8*)(dps + (lane >> 2) * ST_XS + cc4 * 8) = rp;
        __syncthreads();
        request(min(tile + 1, tile_end - 1));                      // (last tile: re-requests itself, unused)
        st_h0_tile(halo, wave, lane, bin, bq, h0s);
        // ---- dh0 = dh1 W1 + 0.25 expand(dp0), rounded to bf16 (what the separate path stored), LDS only: D[cin nt*16 + 4 lg + r][pixel lr]
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            bf16x4 dp[2];                                          // the pooled pixel under columns half*16 + lr of both rows
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) dp[nt] = *(const bf16x4*)(dps + ((half * 16 + lr) >> 1) * ST_XS + nt * 16 + 4 * lg);
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int prow = rr * 32 + half * 16;
                const bf16x8 gf = (lg < 2) ? *(const bf16x8*)(g1s + (prow + lr) * ST_C1 + lg * 8) : zero8();
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1b[nt], gf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    bf16x4 ov;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[r] = f2bf(d[r] + 0.25f * bf2f(dp[nt][r]));
                    *(bf16x4*)(d0s + (prow + lr) * ST_XS + nt * 16 + 4 * lg) = ov;
                }
            }
        }
        wave_fence();
        // ---- weight gradients: K = the 64 pixels of the wave's two rows, 8 consecutive pixels of a row per lane group
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int pix0 = rr * 32 + 8 * lg;
            // dW1[cout lr][cin] += dh1^T h0;  db1 via an all-ones B tile
            const bf16x8 ag = tr_frag(g1s, ST_C1, pix0, 4, 0, lr);
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) aw1[nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ag, tr_frag(h0s, ST_XS, pix0, 4, nj * 16, lr), aw1[nj], 0, 0, 0);
            ab1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ag, ones, ab1, 0, 0, 0);
            // dW_in[tap lr][c] += patch^T dh0 (image values as bf16 high + low parts, the split done at staging); row 9 = ones -> db_in
            const int row = 2 * wave + rr + wdy;
            bf16x8 ahi, alo;
            st_row8(halo[row], 8 * lg + wdx, ahi, alo);
            if (lr >= 9) {
                ahi = (lr == 9) ? ones : zero8();
                alo = zero8();
            }
#pragma unroll
            for (int nj = 0; nj < 2; ++nj) {
                const bf16x8 b = tr_frag(d0s, ST_XS, pix0, 4, nj * 16, lr);
                awin[nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, b, awin[nj], 0, 0, 0);
                awin[nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, b, awin[nj], 0, 0, 0);
            }
        }
    }
    // ---- fold the four waves through LDS, one round of atomics per block.  D[row 4lg + r][col nj*16 + lr]
    __syncthreads();
    float* T = (float*)h0t;                                      // [16][32] dW1 | [16][32] dW_in (+ bias row) | [16] db1
    for (int i = threadIdx.x; i < 16 * 32 * 2 + 16; i += 256) T[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            atomicAdd(&T[(4 * lg + r) * 32 + nj * 16 + lr], aw1[nj][r]);
            atomicAdd(&T[512 + (4 * lg + r) * 32 + nj * 16 + lr], awin[nj][r]);
        }
    if (lr == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(&T[1024 + 4 * lg + r], ab1[r]);
    }
    __syncthreads();
    const int rep = blockIdx.x % STAT_REPL;
    for (int i = threadIdx.x; i < 512; i += 256) atomicAdd(a.dw1 + i, T[i]);                       // [16][32] (Kpad = 32)
    for (int i = threadIdx.x; i < 9 * 32; i += 256) atomicAdd(a.dw_in + i, T[512 + i]);            // taps 0..8
    if (threadIdx.x < 32) atomicAdd(a.db_in + rep * 32 + threadIdx.x, T[512 + 9 * 32 + threadIdx.x]);
    if (threadIdx.x < 16) atomicAdd(a.db1 + rep * 16 + threadIdx.x, T[1024 + threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------
// d img of the pass that trains G (weights frozen): d img = input_conv^T (dh1 W1 + 0.25 expand(dp0)) in one launch.
// For each of the 340 pixels q of the (8+2) x (32+2) halo of an output tile, 16 pixels per MFMA: dh0[q] as in d_stem_bwd
// (D[cin nt*16 + 4 lg + r][pixel lr], rounded to bf16, zero outside the image -- the padding of the separate launches).  The lane's
// eight values -- channels 4 lg .. 4 lg + 3 and 16 + 4 lg .. 16 + 4 lg + 3 of pixel lr -- are at once the A fragment (row = pixel lr,
// k = 8 lg + j) of the second MFMA, whose B fragment holds the flipped taps in the same channel permutation: dh0 never touches LDS.
// That MFMA gives the nine per-tap dot products s[tap][q] = sum_c dh0[q, c] bf16(w[8 - tap][c]) of conv_Cto1_kernel (conv_c1.hip),
// and an output pixel is sum_tap s[tap][p + d(tap)] in the same tap order.  Persistent blocks; the operands of m-tile i of tile t+1 are
// requested (unconditionally, coordinates clamped) as soon as m-tile i of tile t has left its registers; s is double-buffered: one
// barrier per tile.
#define SD_AW (ST_TW + 2)
#define SD_NPIX ((ST_TH + 2) * SD_AW)          // 340 halo pixels
#define SD_MT ((SD_NPIX + 15) / 16)            // 22 m-tiles
#define SD_MPW ((SD_MT + 3) / 4)               // up to 6 per wave
#define SD_LDQ (SD_MT * 16 + 16)               // row stride of s: 368 = 48 mod 64 dwords, the 9 tap rows spread over the banks
__global__ __launch_bounds__(256, 4) void d_stem_dimg_kernel(DStemArgs a, int tiles_w, int tiles_h) {
    __shared__ __attribute__((aligned(16))) float s[2][9][SD_LDQ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int H = a.H, W = a.W, Hp = H >> 1, Wp = W >> 1;
    bf16x8 w1b[2];                                               // as in d_stem_bwd
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) w1b[nt] = (lg < 2) ? *(const bf16x8*)((const bf16*)a.w1_bwd + (nt * 16 + lr) * 32 + lg * 8) : zero8();
    bf16x8 wt;                                                   // B[k = 8 lg + j -> channel (j < 4 ? 4 lg + j : 12 + 4 lg + j)][col = tap lr], flipped
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = j < 4 ? 4 * lg + j : 12 + 4 * lg + j;
        const float v = a.w_in[max(8 - lr, 0) * ST_C0 + c];
        wt[j] = f2bf(lr < 9 ? v : 0.f);
    }
    int qyx[SD_MPW];                                             // this lane's halo pixel of each of the wave's m-tiles (the same in every tile): qy << 8 | qx
#pragma unroll
    for (int i = 0; i < SD_MPW; ++i) {
        const int q = min((wave + 4 * i) * 16 + lr, SD_NPIX - 1);
        qyx[i] = ((q / SD_AW) << 8) | (q % SD_AW);
    }
    const int ntiles = a.N * tiles_w * tiles_h;
    const int per = (ntiles + gridDim.x - 1) / gridDim.x;
    const int tile_end = min((int)(blockIdx.x + 1) * per, ntiles);
    bf16x8 rg[SD_MPW];                                           // dh1[q][8 (lg & 1) ..]
    bf16x4 rp[SD_MPW][2];                                        // dp0[pooled q][nt*16 + 4 lg ..]
    unsigned okm = 0;                                            // bit i: q of m-tile i lies inside the image
    // the operands of m-tile i of a tile: element offsets inside one image fit 32 bits, the image base is wave-uniform
    auto request = [&](StTile t, int i) {
        const int yy = t.y0 - 1 + (qyx[i] >> 8), xx = t.x0 - 1 + (qyx[i] & 255);
        const int yc = min(max(yy, 0), H - 1), xc = min(max(xx, 0), W - 1);
        okm = (yy == yc && xx == xc) ? okm | (1u << i) : okm & ~(1u << i);
        const bf16* g = (const bf16*)a.dh1 + (long)t.n * H * W * ST_C1;
        const bf16* dp = (const bf16*)a.dp0 + (long)t.n * Hp * Wp * ST_C0;
        rg[i] = *(const bf16x8*)(g + ((yc * W + xc) * ST_C1 + (lg & 1) * 8));
        const int o = ((yc >> 1) * Wp + (xc >> 1)) * ST_C0 + 4 * lg;
        rp[i][0] = *(const bf16x4*)(dp + o);
        rp[i][1] = *(const bf16x4*)(dp + o + 16);
    };
    const int tile_begin = blockIdx.x * per;
    if (tile_begin < tile_end) {
        const StTile t = st_tile(tile_begin, tiles_w, tiles_h);
#pragma unroll
        for (int i = 0; i < SD_MPW; ++i) request(t, i);
    }
    int buf = 0;
    for (int tile = tile_begin; tile < tile_end; ++tile, buf ^= 1) {
        const StTile t = st_tile(tile, tiles_w, tiles_h);
        const StTile tn = st_tile(min(tile + 1, tile_end - 1), tiles_w, tiles_h);     // (last tile: re-requests itself, unused)
#pragma unroll
        for (int i = 0; i < SD_MPW; ++i) {
            const int mt = wave + 4 * i;
            const bf16x8 gf = (lg < 2) ? rg[i] : zero8();
            bf16x8 af;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1b[nt], gf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) af[nt * 4 + r] = f2bf(d[r] + 0.25f * bf2f(rp[i][nt][r]));
            }
            if (!(okm & (1u << i))) af = zero8();
            request(tn, i);                                        // this m-tile's registers are free: the next tile's operands
            if (mt < SD_MT) {                                      // D[row = pixel 4 lg + r][col = tap lr]
                const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wt, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                if (lr < 9) *(f32x4*)&s[buf][lr][mt * 16 + lg * 4] = acc;
            }
        }
        __syncthreads();                                           // (s[buf] is rewritten two tiles on, past the next barrier)
        {
            const int ty = threadIdx.x >> 5, tx = threadIdx.x & 31;
            float r = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) r += s[buf][tap][(ty + tap / 3) * SD_AW + tx + tap % 3];
            a.dimg[((long)t.n * H + t.y0 + ty) * W + t.x0 + tx] = r;
        }
    }
}

// ------------------------------------------------------------------------------------------------
static int stem_check(const ieagan_d_stem_desc* d) {
    CHECK_ARG(d != nullptr && d->img != nullptr && d->w_in != nullptr && d->b_in != nullptr, "d_stem: null pointer");
    CHECK_ARG(d->N >= 1 && d->H % ST_TH == 0 && d->W % ST_TW == 0, "d_stem: H %% 8 and W %% 32 required (%d x %d)", d->H, d->W);
    return 0;
}

static DStemArgs stem_args(const ieagan_d_stem_desc* d) {
    DStemArgs a{};
    a.img = d->img; a.N = d->N; a.H = d->H; a.W = d->W;
    a.w_in = d->w_in; a.b_in = d->b_in; a.w1 = d->w1; a.b1 = d->b1; a.wsc = d->wsc; a.bsc = d->bsc;
    a.h1 = d->h1; a.p0 = d->p0; a.sc = d->sc;
    a.dh1 = d->dh1; a.dp0 = d->dp0; a.w1_bwd = d->w1_bwd; a.dw_in = d->dw_in; a.db_in = d->db_in; a.dw1 = d->dw1; a.db1 = d->db1;
    return a;
}

extern "C" int ieagan_d_stem_fwd(const ieagan_d_stem_desc* d, void* stream) {
    if (int rc = stem_check(d)) return rc;
    CHECK_ARG(d->w1 != nullptr && d->b1 != nullptr && d->wsc != nullptr && d->bsc != nullptr && d->h1 != nullptr && d->p0 != nullptr && d->sc != nullptr,
              "d_stem_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const double P = (double)d->N * d->H * d->W;
    ProfScope prof("d_stem_fwd", 2.0 * P * (9 * 32 + 32 * 16 + 0.25 * 32 * 32), P * (4.0 + 2.0 * (16 + 0.25 * 64)), st);
    const int tiles_w = d->W / ST_TW, tiles_h = d->H / ST_TH;
    const long ntl = (long)d->N * tiles_w * tiles_h;
    const long blocks = ntl < 1024 ? ntl : 1024;                  // one round of persistent blocks (32 KB of LDS, 96 VGPRs: four per CU)
    hipLaunchKernelGGL(d_stem_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, stem_args(d), tiles_w, tiles_h);
    CHECK_LAUNCH("d_stem_fwd");
    return 0;
}

extern "C" int ieagan_d_stem_bwd(const ieagan_d_stem_desc* d, void* stream) {
    if (int rc = stem_check(d)) return rc;
    CHECK_ARG(d->dh1 != nullptr && d->dp0 != nullptr && d->w1_bwd != nullptr && d->dw_in != nullptr && d->db_in != nullptr && d->dw1 != nullptr && d->db1 != nullptr,
              "d_stem_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const double P = (double)d->N * d->H * d->W;
    ProfScope prof("d_stem_bwd", 2.0 * P * (9 * 32 + 3 * 32 * 16 + 2 * 9 * 32), P * (4.0 + 2.0 * (16 + 0.25 * 32)), st);
    const int tiles_w = d->W / ST_TW, tiles_h = d->H / ST_TH;
    const long ntl = (long)d->N * tiles_w * tiles_h;
    const long blocks = ntl < 512 ? ntl : 512;                    // one round of persistent blocks (two per CU)
    hipLaunchKernelGGL(d_stem_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, stem_args(d), tiles_w, tiles_h);
    CHECK_LAUNCH("d_stem_bwd");
    return 0;
}

extern "C" int ieagan_d_stem_dimg(const void* dh1, const void* dp0, const void* w1_bwd, const float* w_in, float* dimg, int N, int H, int W,
                                  void* stream) {
    CHECK_ARG(dh1 != nullptr && dp0 != nullptr && w1_bwd != nullptr && w_in != nullptr && dimg != nullptr, "d_stem_dimg: null pointer");
    CHECK_ARG(N >= 1 && H >= ST_TH && W >= ST_TW && H % ST_TH == 0 && W % ST_TW == 0, "d_stem_dimg: H %% 8 and W %% 32 required (%d x %d)", H, W);
    hipStream_t st = (hipStream_t)stream;
    const double P = (double)N * H * W;
    ProfScope prof("d_stem_dimg", 2.0 * P * (16 * 32 + 9 * 32), P * (2.0 * (16 + 0.25 * 32) + 4.0), st);
    DStemArgs a{};
    a.N = N; a.H = H; a.W = W;
    a.dh1 = dh1; a.dp0 = dp0; a.w1_bwd = w1_bwd; a.w_in = w_in; a.dimg = dimg;
    const int tiles_w = W / ST_TW, tiles_h = H / ST_TH;
    const long ntl = (long)N * tiles_w * tiles_h;
    CHECK_ARG(ntl < (1L << 31), "d_stem_dimg: bad geometry");
    const long blocks = ntl < 1024 ? ntl : 1024;                  // one round of persistent blocks (four per CU)
    hipLaunchKernelGGL(d_stem_dimg_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, tiles_w, tiles_h);
    CHECK_LAUNCH("d_stem_dimg");
    return 0;
}
