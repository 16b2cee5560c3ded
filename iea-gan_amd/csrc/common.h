// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of the IEA-GAN train step.
// Activations: bf16, NHWC.  Accumulation / statistics / parameters: fp32.  Wavefront = 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

#define IEAGAN_OK 0
#define IEAGAN_EINVAL (-1)
#define IEAGAN_ELAUNCH (-2)

// thread-local last-error text, set by the launchers in api.hip
void ieagan_set_error(const char* fmt, ...);
// optional per-kernel event profiling (api.hip); name must be a string literal
// (the scope OWNS its two events and hands the finished record to the collector in its destructor: a scope that is open on the autograd or
//  side-stream thread while another thread collects / resets never touches the collector's storage)
struct ProfScope {
    ProfScope(const char* name, double flops, double bytes, hipStream_t s, const char* tag = nullptr, double bytes_min = -1.0);
    ~ProfScope();
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;
    bool active;
    hipStream_t stream;
    hipEvent_t ev_a, ev_b;
    double flops, bytes, bytes_min;
    char name[96];
};

bool prof_tags_on();

#define CHECK_ARG(cond, ...)                                   \
    do {                                                       \
        if (!(cond)) {                                         \
            ieagan_set_error(__VA_ARGS__);                     \
            return IEAGAN_EINVAL;                              \
        }                                                      \
    } while (0)

#define CHECK_LAUNCH(name)                                                          \
    do {                                                                            \
        hipError_t e__ = hipGetLastError();                                         \
        if (e__ != hipSuccess) {                                                    \
            ieagan_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return IEAGAN_ELAUNCH;                                                  \
        }                                                                           \
    } while (0)

__device__ __forceinline__ float bf2f(bf16 v) { return (float)v; }
__device__ __forceinline__ bf16 f2bf(float v) { return (bf16)v; }

// ReLU of 8 packed bf16 values on their bit patterns: as signed 16-bit integers every negative float (sign bit set, incl. -0
// and negative NaNs) is a negative integer and every non-negative float keeps its order, so max(bits, 0) is exact --
// four v_pk_max_i16 instead of unpack / v_max_f32 / repack per element.
typedef short i16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 relu8(bf16x8 v) {
    i16x8 s = __builtin_bit_cast(i16x8, v);
    const i16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    s = __builtin_elementwise_max(s, z);
    return __builtin_bit_cast(bf16x8, s);
}

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = (bf16)0.0f;
    return z;
}

// sum over the 64 lanes of a wave
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Make this wave's LDS stores visible to its other lanes (and keep the compiler from moving LDS accesses across): the LDS operations
// of one wave execute in order, so wave-private buffers need no block barrier.
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Two ds_read_b64_tr_b16 as one MFMA fragment: lane 4q+p of a 16-lane group supplies row q, columns 4p .. 4p+3 of a [row][channel]
// 16-bit LDS image and receives column (lane & 15) of the 4 rows.  p0 / p1: this lane's addresses in the two row groups.  EXEC must be
// all ones.
__device__ __forceinline__ bf16x8 tr_pair(const bf16* p0, const bf16* p1) {
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)p0);
    const bf16x4 hh = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)p1);
    bf16x8 f;
    f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
    f[4] = hh[0]; f[5] = hh[1]; f[6] = hh[2]; f[7] = hh[3];
    return f;
}
// K(row)-major fragment: rows row0 .. row0+3 and row0+hi .. row0+hi+3 of column (col0 + lr) of an LDS image with `stride_elems` per row.
// Bank layout: one half-wave instruction reads 8 image rows x 32 bytes; with the rows of lane groups 0, 1 consecutive and a row stride
// that is an odd multiple of 32 bytes (lds_stride_odd32) they cover the 64 banks exactly once.
__device__ __forceinline__ bf16x8 tr_frag(const bf16* lds, int stride_elems, int row0, int hi, int col0, int lr) {
    const int q = lr >> 2, p = lr & 3;
    const bf16* p0 = lds + (row0 + q) * stride_elems + col0 + 4 * p;
    return tr_pair(p0, p0 + hi * stride_elems);
}
// row stride (elements) of a C-channel 16-bit LDS image: an odd multiple of 32 bytes
__host__ __device__ constexpr int lds_stride_odd32(int C) { return ((C / 16) % 2 == 0) ? C + 16 : C; }

// XCD-aware block order: hardware blocks b and b + 8 share an XCD (and its L2); the returned index makes every XCD walk one contiguous
// run of the nblk work items.
__device__ __forceinline__ int xcd_block_order(int bid, int nblk) {
    const int q = nblk / 8, r = nblk % 8, xcd = bid % 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// Replicated statistics buffers: float atomics on a single address serialise (MI355X: ~14x slower
// than spread adds), so per-channel sums are spread over STAT_REPL replicas keyed by the block
// index and folded by the consumer (bn_finalize / the python side).
#define STAT_REPL 32
#define BNB_REPL 8          // replicas of the per-image (d shift, d scale) accumulators of a BatchNorm-backward dgrad launch

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
