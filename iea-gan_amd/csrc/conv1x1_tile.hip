// conv1x1_tile: the 1x1 convolutions that conv1x1_stream does not take -- Cin >= 256, the 2x2-pooled source of a DBlock's conv4
// (model.py:541-557), mid-size feature maps -- as an LDS-tiled implicit GEMM.
//
// conv_gather fetches every operand fragment straight from global memory: per k-step and wave two A fragments (16 pixels x 64 bytes
// each, the pixels Cin*2 bytes apart) and NT weight fragments (16 rows x 64 bytes, Kpad*2 bytes apart) -- the weight fragments again
// in all four waves and in every block.  For 256 -> 128 at 32x96 that is 192 KB of fragment-shaped L2 -> CU traffic per 128-pixel
// block against 96 KB of operands, and the address path (one 128-byte line per 64 useful bytes), not HBM or the MFMA, bounds the
// launch (the non-local attention kernels had the same disease: attention.hip).  Here a block moves its 128 pixels x KC channels and
// its NT*16 x KC weight slice into LDS ONCE per K chunk, in full rows with the prologue applied (per-image BatchNorm scale / shift,
// ReLU, 2x2 average pool of the activated source), and all fragments are ds_read_b128 from XOR-swizzled tiles.
// Same operator contract and epilogue (conv_common.h: bias, residuals, ReLU mask, BatchNorm-backward, statistics) as conv_gather for
// taps == 1; the accumulation order over k is the same, so the two kernels agree bit for bit.
#include "common.h"
#include "conv_args.h"
#include "conv_common.h"

namespace {

// 16-byte chunk c of row r of a [rows][KC] bf16 tile lives at chunk position c ^ key(r): 16 consecutive rows read by the 16 lanes of
// an A / B fragment (one chunk each, rows KC*2 bytes apart) then cover all banks
template <int KC>
__device__ __forceinline__ int tkey(int r) { return KC == 128 ? (r & 15) : KC == 64 ? ((r >> 1) & 7) : ((r >> 2) & 3); }
template <int KC>
__device__ __forceinline__ int toff(int r, int c) { return r * KC + ((c ^ tkey<KC>(r)) << 3); }      // in bf16 elements

// pooled source: items (four 16-byte loads each) requested per batch and thread; the BatchNorm forms spend their registers on the fp32 prologue
constexpr int POOL_BATCH = 4, POOL_BATCH_AFF = 2;

template <bool AFF, bool RELU>
__device__ __forceinline__ void pro8(float (&v)[8], const bf16x8& raw, const SrcDesc& s, int n, int c, const float* aff) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bf2f(raw[i]);
    xform8<AFF, RELU>(v, s, n, c, aff);
}

}  // namespace

template <bool AFF, bool RELU, int RS, int NT, int KC, bool BNB>
__global__ __launch_bounds__(256, 3) void conv1x1_tile_kernel(ConvArgs a) {
    constexpr int CPR = KC / 8;                               // 16-byte chunks per tile row
    constexpr int EROWS = 16;
    constexpr int ABYTES = 128 * KC * 2, BBYTES = NT * 16 * KC * 2;
    constexpr int EPIB = 4 * EROWS * EpiLds<NT>::LDW * 4;
    constexpr int ASZ = ABYTES > EPIB ? ABYTES : EPIB;        // the epilogue's transpose buffer reuses the A tile
    static_assert(EPIB >= 4 * STATS_SX_FLOATS * 4, "epilogue buffer doubles as the statistics scratch");
    __shared__ __attribute__((aligned(16))) char smem[ASZ + BBYTES];
    __shared__ float red[4 * NT * 16 * 2];
    __shared__ __attribute__((aligned(32))) float aff_s[AFF ? 2 * AFF_MAXC : 8];
    bf16* atile = (bf16*)smem;
    bf16* btile = (bf16*)(smem + ASZ);
    float* epi = (float*)smem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int H = a.H, W = a.W, HW = H * W;
    const long M = (long)a.N * HW;
    // XCD-aware order with the n-tile column as the fast index (see conv1x1_stream.hip): the gy blocks that read the same 128 pixels
    // run side by side on one XCD and share them through its L2
    const int gy = a.Cout / (NT * 16);
    const int vid = xcd_block_order(blockIdx.x, gridDim.x);
    const int bx = vid / gy;
    const long m_blk = (long)bx * 128;
    const long m_base = m_blk + wave * 32;                    // this wave's 32 output pixels
    const int n_base = (vid % gy) * NT * 16;
    const int n_img = (int)(m_blk / HW);                      // AFF: the launcher guarantees HW % 128 == 0 (one image per block)
    if (AFF) stage_aff(aff_s, a.src, n_img, a.Cin);           // (the first barrier of the K loop publishes it)
    const float* affp = AFF ? aff_s : nullptr;
    const bf16* xsrc = (const bf16*)a.src.x;

    f32x4 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    constexpr int IT = (128 * CPR) / 256;                     // A staging items (16-byte chunks) per thread and K chunk
    constexpr int ITB = (NT * 16 * CPR + 255) / 256;          // weight staging items per thread and K chunk
    constexpr bool WFULL = (NT * 16 * CPR) % 256 == 0;        // every thread has a weight item in every pass
    constexpr int EIT = NT / 2;                               // epilogue iterations per 16-row half: (16 * 2*NT) / 64
    const bf16* wsrc = (const bf16*)a.w;

    // ---- staging.  Every global load is UNCONDITIONAL on a clamped address (row <= Cout - 1, channel <= Kpad - 8 / Cin - 8, pixel
    // <= M - 1) and what lies outside is zeroed by a select when the chunk goes to LDS: behind a per-lane branch the compiler cannot
    // count the requests and drains the counter after each one -- ITB + 1 dependent memory round trips per chunk where one does.
    // request = global -> registers, store = prologue + registers -> LDS; between the two a chunk may stay in flight.
    // Addresses are a block-uniform base (scalar registers) plus a 32-bit lane offset: 64-bit lane pointers of a dozen requests,
    // hoisted out of the K loop, cost two registers each.
    const bf16* wblk = wsrc + (long)n_base * a.Kpad;          // Cout % (NT*16) == 0 (dispatch): n_base < Cout
    const int c8 = (threadIdx.x % CPR) * 8;                   // this thread's channel offset inside a chunk: 256 % CPR == 0, the same for every item
    auto w_request = [&](int kc0, bf16x8(&wr)[ITB]) {         // rows [n_base, n_base + NT*16) x k in [kc0, kc0 + KC)
        const unsigned k = (unsigned)min(kc0 + c8, a.Kpad - 8);
#pragma unroll
        for (int j = 0; j < ITB; ++j) {
            const int row = (threadIdx.x + j * 256) / CPR;
            wr[j] = *(const bf16x8*)(wblk + ((unsigned)(min(n_base + row, a.Cout - 1) - n_base) * (unsigned)a.Kpad + k));
        }
    };
    auto w_store = [&](int kc0, const bf16x8(&wr)[ITB]) {
#pragma unroll
        for (int j = 0; j < ITB; ++j) {
            const int idx = threadIdx.x + j * 256;
            const int row = idx / CPR, c = idx - row * CPR;
            const bool in = n_base + row < a.Cout && kc0 + c * 8 < a.Kpad;
            if (WFULL || idx < NT * 16 * CPR) *(bf16x8*)(btile + toff<KC>(row, c)) = in ? wr[j] : zero8();
        }
    };
    // activations, RS == 0: 128 pixels x KC channels; consecutive threads take consecutive 16-byte chunks of consecutive pixels (full
    // 128-byte lines)
    const bf16* ablk = xsrc + m_blk * a.src.Cx;
    const int p_last = (int)min((long)127, M - 1 - m_blk);    // last pixel of this block inside the tensor
    auto a_request = [&](int kc0, bf16x8(&ar)[IT]) {
        const unsigned k = (unsigned)min(kc0 + c8, a.Cin - 8);
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const int p = (threadIdx.x + j * 256) / CPR;
            ar[j] = *(const bf16x8*)(ablk + ((unsigned)min(p, p_last) * (unsigned)a.src.Cx + k));
        }
    };
    auto a_store = [&](int kc0, const bf16x8(&ar)[IT]) {
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const int idx = threadIdx.x + j * 256;
            const int p = idx / CPR, c = idx - p * CPR;
            const int ch = kc0 + c * 8;
            bf16x8 o = ar[j];
            if (AFF || RELU) {
                if (!AFF) {
                    o = relu8(o);
                } else {
                    float v[8];
                    pro8<AFF, RELU>(v, ar[j], a.src, n_img, min(ch, a.Cin - 8), affp);
#pragma unroll
                    for (int i = 0; i < 8; ++i) o[i] = f2bf(v[i]);
                }
            }
            if (m_blk + p >= M || ch >= a.Cin) o = zero8();   // (Cin = 16: half of a 32-deep k-step is padding)
            *(bf16x8*)(atile + toff<KC>(p, c)) = o;
        }
    };
    // RS == 2: conv pixel = mean of the 2x2 block of the ACTIVATED source (AvgPool2d(2), model.py:547-550).  4 loads per item: PB items
    // per batch, the weight slice rides with the first batch
    constexpr int PBW = AFF ? POOL_BATCH_AFF : POOL_BATCH;
    constexpr int PB = IT < PBW ? IT : PBW;
    auto pool_off = [&](long m) -> long {                     // source element offset of the 2x2 block of conv pixel m
        const int n = (int)(m / HW);
        const int rem = (int)(m - (long)n * HW);
        const int h = rem / W, w = rem - h * W;
        return (((long)n * a.src.Hs + 2 * h) * a.src.Ws + 2 * w) * a.src.Cx;
    };
    const long pool_o0 = RS == 2 ? pool_off(m_blk) : 0;       // images follow one another: a block's offsets relative to it are small
    const bf16* pblk = xsrc + pool_o0;
    auto pooled_stage = [&](int kc0) {
        bf16x8 wr[ITB];
        w_request(kc0, wr);
        const unsigned k = (unsigned)min(kc0 + c8, a.Cin - 8);
        const bf16 *b0 = pblk, *b1 = pblk + a.src.Cx, *b2 = pblk + (long)a.src.Ws * a.src.Cx, *b3 = b2 + a.src.Cx;
#pragma unroll
        for (int j0 = 0; j0 < IT; j0 += PB) {
            bf16x8 raw[PB][4];
#pragma unroll
            for (int jj = 0; jj < PB; ++jj) {
                const int p = (threadIdx.x + (j0 + jj) * 256) / CPR;
                const unsigned o = (unsigned)(pool_off(min(m_blk + p, M - 1)) - pool_o0) + k;
                raw[jj][0] = *(const bf16x8*)(b0 + o);
                raw[jj][1] = *(const bf16x8*)(b1 + o);
                raw[jj][2] = *(const bf16x8*)(b2 + o);
                raw[jj][3] = *(const bf16x8*)(b3 + o);
            }
            if (j0 == 0) w_store(kc0, wr);
#pragma unroll
            for (int jj = 0; jj < PB; ++jj) {
                const int idx = threadIdx.x + (j0 + jj) * 256;
                const int p = idx / CPR, c = idx - p * CPR;
                const int ch = kc0 + c * 8;
                const int n = AFF ? n_img : 0;
                float s8[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) s8[i] = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v[8];
                    pro8<AFF, RELU>(v, raw[jj][q], a.src, n, min(ch, a.Cin - 8), affp);
#pragma unroll
                    for (int i = 0; i < 8; ++i) s8[i] += v[i];
                }
                bf16x8 o;
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = f2bf(0.25f * s8[i]);
                if (m_blk + p >= M || ch >= a.Cin) o = zero8();
                *(bf16x8*)(atile + toff<KC>(p, c)) = o;
            }
        }
    };
    // ---- MFMA over the chunk in LDS, every fragment a ds_read_b128
    auto mfma_chunk = [&]() {
#pragma unroll
        for (int ks = 0; ks < KC / 32; ++ks) {
            bf16x8 af[2], bf[NT];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) af[mt] = *(const bf16x8*)(atile + toff<KC>(wave * 32 + mt * 16 + lr, ks * 4 + lg));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bf[nt] = *(const bf16x8*)(btile + toff<KC>(nt * 16 + lr, ks * 4 + lg));
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
            if (KC == 128) __builtin_amdgcn_sched_barrier(0); // the fragments of all four k-steps at once would push the in-flight chunk to scratch
        }
    };
    // ---- the epilogue's global operands of BOTH 16-row halves (ReLU mask / BatchNorm input, same- or half-resolution residual chunk),
    // requested before the last chunk's MFMAs: same lane -> (row, chunk) mapping as conv_epilogue_finish, pixel clamped to M - 1 (the
    // epilogue neither uses nor stores rows past M).  The double-resolution residual (four loads per chunk) stays in the epilogue.
    bf16x8 mk_pre[2][EIT], rs_pre[2][EIT];
    float bias_v[8];
    auto epi_request = [&]() {
        load_bias8<NT>(a, n_base, bias_v);                    // once per block, not a round trip inside each epilogue half
        const int co0 = n_base + (lane % (2 * NT)) * 8;
        long m[2][EIT];
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int it = 0; it < EIT; ++it) m[half][it] = min(m_base + 16 * half + (it * 64 + lane) / (2 * NT), M - 1);
        // No branch around the loads, not even a block-uniform one: a value loaded on one side of a branch and zero on the other is
        // merged by register copies right behind the branch, which wait for the load.  An absent operand reads the first 16 bytes of
        // the weights instead (one line for the whole wave; the epilogue does not look at the value).
        const bf16* mbase = a.mask != nullptr ? (const bf16*)a.mask + co0 : wsrc;
        const long mstride = a.mask != nullptr ? a.Cout : 0;
        // this lane's residual operand: A on channels [0, Ca), B on [Ca, Cout)
        const bool ra_here = a.ra != nullptr && co0 < a.Ca;
        const bool rb_here = !ra_here && a.rb != nullptr && co0 >= a.Ca;
        const bool ra_ok = ra_here && a.ra_rs != 2;
        const bf16* rbase = ra_ok ? (const bf16*)a.ra + co0 : rb_here ? (const bf16*)a.rb + (co0 - a.Ca) : wsrc;
        const long rstride = ra_ok ? a.Cra : rb_here ? a.Crb : 0;
        const bool up = ra_ok && a.ra_rs == 1;                // operand lives at half resolution: nearest x2 upsample
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int it = 0; it < EIT; ++it) {
                long pi = m[half][it];
                if (a.ra != nullptr && a.ra_rs == 1) {
                    const int n = (int)(pi / HW);
                    const int rem = (int)(pi - (long)n * HW);
                    const int h = rem / W, w = rem - h * W;
                    const long hi = ((long)n * (H >> 1) + (h >> 1)) * (W >> 1) + (w >> 1);
                    pi = up ? hi : pi;
                }
                mk_pre[half][it] = *(const bf16x8*)(mbase + m[half][it] * mstride);
                rs_pre[half][it] = *(const bf16x8*)(rbase + pi * rstride);
            }
    };

    // ---- K loop.  RS == 0 keeps the raw operands of chunk k + 1 in registers across the MFMAs of chunk k (requested before them,
    // written to LDS after them); the last chunk -- the only one of a launch with Cin <= KC -- runs straight, with the epilogue's
    // operands in flight instead.  The k order of every accumulation is unchanged.
    bf16x8 wr[RS == 0 ? ITB : 1], ar[RS == 0 ? IT : 1];
    if constexpr (RS == 0) {
        w_request(0, wr);
        a_request(0, ar);
    }
    int kc0 = 0;
    if constexpr (KC == 128)                                  // (the dispatch gives Cin <= 32 and Cin == 64 a chunk of their own depth: one trip)
    for (; kc0 + KC < a.Cin; kc0 += KC) {
        __syncthreads();                                      // the previous chunk's fragment reads are done (first trip: aff_s is complete)
        if constexpr (RS == 0) {
            w_store(kc0, wr);
            a_store(kc0, ar);
        } else {
            pooled_stage(kc0);
        }
        __syncthreads();
        if constexpr (RS == 0) {
            w_request(kc0 + KC, wr);
            a_request(kc0 + KC, ar);
        }
        mfma_chunk();
    }
    __syncthreads();
    if constexpr (RS == 0) {
        w_store(kc0, wr);
        a_store(kc0, ar);
    } else {
        pooled_stage(kc0);
    }
    __syncthreads();
    epi_request();
    mfma_chunk();
    __syncthreads();                                          // the A tile is dead: its memory becomes the epilogue's transpose buffer

    float s1[8], s2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s1[i] = s2[i] = 0.f;
    const bool need_hw = (a.ra != nullptr && a.ra_rs != 0) || (BNB && a.bnb_scale != nullptr);
    auto pix = [&](int row, long& m, int& n, int& h, int& w) -> bool {
        m = m_base + row;
        n = h = w = 0;
        if (m >= M) return false;
        if (need_hw) {
            n = (int)(m / HW);
            const int rem = (int)(m - (long)n * HW);
            h = rem / W;
            w = rem - h * W;
        }
        return true;
    };
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        auto pixh = [&](int row, long& m, int& n, int& h, int& w) -> bool { return pix(row + 16 * half, m, n, h, w); };
        const f32x4(&sub)[1][NT] = *reinterpret_cast<const f32x4(*)[1][NT]>(&acc[half]);
        conv_epilogue<BNB, NT, 1, (RS != 2)>(a, sub, epi + wave * EROWS * EpiLds<NT>::LDW, n_base, pixh, s1, s2, bias_v, mk_pre[half], rs_pre[half]);
    }
    if (a.stats != nullptr) {
        __syncthreads();          // every wave is done with its part of the epilogue buffer, which now serves as fold scratch
        const int event = (a.n_per_event > 0) ? (int)(m_blk / ((long)a.n_per_event * HW)) : 0;
        stats_flush<NT>(a, s1, s2, n_base, red, epi, bx, event);
    }
}

template <bool AFF, bool RELU, int RS, bool BNB>
static int tile_dispatch(const ConvArgs& a, hipStream_t st) {
    const long M = (long)a.N * a.H * a.W;
    const unsigned gx = (unsigned)((M + 127) / 128);
    const int n_events_t = (a.stats != nullptr && a.n_per_event > 0) ? a.N / a.n_per_event : 1;
#define TL(NTV, KCV)                                                                                                                    \
    {                                                                                                                                   \
        CONV_PLAN_POINT((int)(gx / n_events_t), 1)                                                                                      \
        hipLaunchKernelGGL((conv1x1_tile_kernel<AFF, RELU, RS, NTV, KCV, BNB>), dim3(gx * (a.Cout / (NTV * 16))), dim3(256), 0, st, a);     \
        return 1;                                                                                                                       \
    }
#define BY_KC(NTV)                      \
    if (a.Cin <= 32) TL(NTV, 32)        \
    else if (a.Cin == 64) TL(NTV, 64)   \
    else TL(NTV, 128)
    if (a.Cout % 64 == 0) { BY_KC(4) }
    else { BY_KC(2) }
#undef BY_KC
#undef TL
    return 0;
}

// 1 = launched, 0 = not applicable (the caller falls back to conv_gather)
int conv1x1_tile_launch(const ConvArgs& a, hipStream_t st) {
    if (a.taps != 1 || (a.src.rs != 0 && a.src.rs != 2) || a.Cout % 32 != 0 || a.Cin % 8 != 0) return 0;
    if (!(a.Cin <= 32 || a.Cin == 64 || a.Cin % 128 == 0) || a.Kpad != ((a.Cin + 31) / 32) * 32) return 0;
    const long HW = (long)a.H * a.W, M = (long)a.N * HW;
    // tiny maps stay with conv_gather's split-K form (4x12: 512 -> 128 7.3 us there, 14.0 here); from 8x24 up this kernel wins even with 60
    // pixel blocks (8x24: 256 -> 256 19.7 -> 8.7 us, pooled source 40.3 -> 13.3; 128 -> 512 13.2 -> 9.4), pooled sources already at 4x12 (13.0 -> 8.5)
    const bool forced = (a.flags & IEAGAN_CONV_FORCE_TILE) != 0;      // tools/tile1x1_ab.py scans the two floors below with it
    if (!forced && M < (a.src.rs == 2 ? 1024 : 4096)) return 0;
    if (!forced && M < 16384 && a.Cin > 256) return 0;                    // four serial K chunks on 120 blocks: in-step 17.7 -> 26.5 us for 512 -> 128 at 8x24
    const bool aff = a.src.scale != nullptr, relu = a.src.relu != 0;
    if (aff && (HW % 128 != 0 || a.Cin > AFF_MAXC)) return 0;  // one image (one BatchNorm table) per 128-pixel block
    if (a.bnb_scale != nullptr) {
        if (aff || relu || a.src.rs != 0) return 0;
        return tile_dispatch<false, false, 0, true>(a, st);
    }
    if (a.src.rs == 0) {
        if (aff && relu) return tile_dispatch<true, true, 0, false>(a, st);
        if (aff) return tile_dispatch<true, false, 0, false>(a, st);
        if (relu) return tile_dispatch<false, true, 0, false>(a, st);
        return tile_dispatch<false, false, 0, false>(a, st);
    }
    if (aff && relu) return tile_dispatch<true, true, 2, false>(a, st);
    if (aff) return tile_dispatch<true, false, 2, false>(a, st);
    if (relu) return tile_dispatch<false, true, 2, false>(a, st);
    return tile_dispatch<false, false, 2, false>(a, st);
}
