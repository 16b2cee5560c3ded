"""Plain restatement of the arithmetic of csrc/d_stem.hip (d_stem_fwd, d_stem_bwd): the checker of tests/test_d_stem_gpu.py, itself pinned
against fp64 ``torch.autograd`` of conv2d / avg_pool2d in tests/test_d_stem_reference.py.

Written from the header comment of csrc/d_stem.hip, with explicit shifted sums instead of library layers.  Every function computes in
the dtype ``dt`` it is given: with fp64 it is the reference, with fp32 it is the "ordered fp32 chain" yardstick that the GPU tests print
next to the kernel's error.  Values are rounded to bf16 exactly where the kernels round them: the image enters as bf16 high + low parts,
the weights of every product are bf16, h0 / p0 / dh0 are rounded once where they are formed.  Nothing here imports the product package.

Layouts: activations NHWC; ``w_in`` fp32 [9][32] (tap = 3 ky + kx, cross-correlation with padding 1); ``w1`` [16][32] and ``wsc`` [32][32]
as [cout][cin]; ``w1_bwd`` [32][32] = [cin][cout] with columns 16.. zero."""
import numpy as np
import torch
import torch.nn.functional as F

from sn_reference import bf16_neighbours
from small_ops_reference import rel_err      # noqa: F401  (the error measure of the backward checks)

BF16 = torch.bfloat16
C0, C1, CS = 32, 16, 32


def rb(x):
    """Round to bf16 once, keep the dtype: fp64 values through integer arithmetic on the bit patterns (no double rounding through fp32)."""
    if x.dtype == torch.float64:
        return bf16_neighbours(x)[0].double()
    return x.to(BF16).to(x.dtype)


def split(img32):
    """fp32 image -> (hi, lo) fp32 tensors holding bf16 values: hi = bf16(v), lo = bf16(v - hi)."""
    hi = img32.to(BF16).float()
    return hi, (img32 - hi).to(BF16).float()


def _shift(x, tap):
    """x [N, H, W] -> the values at (y + ky - 1, x + kx - 1), zero outside the image."""
    ky, kx = tap // 3, tap % 3
    H, W = x.shape[1:]
    return F.pad(x, (1, 1, 1, 1))[:, ky:ky + H, kx:kx + W]


def h0_of(img32, w_in, b_in, dt):
    """input_conv: sum over taps of (hi + lo) * bf16(w) + bias, rounded to bf16.  -> [N, H, W, 32]"""
    hi, lo = (t.to(dt) for t in split(img32))
    w = rb(w_in.to(dt))
    acc = torch.zeros(*img32.shape, C0, dtype=dt)
    for part in (hi, lo):                                            # the MFMA's k order: nine high taps, then nine low taps
        for tap in range(9):
            acc += _shift(part, tap)[..., None] * w[tap]
    return rb(acc + b_in.to(dt))


def forward(img32, w_in, b_in, w1, b1, wsc, bsc, dt):
    """-> h0, h1, p0, sc (all holding bf16 values in dtype ``dt``).  w1 / wsc: tensors holding bf16 values."""
    h0 = h0_of(img32, w_in, b_in, dt)
    h1 = rb(h0 @ w1.to(dt).t() + b1.to(dt))
    N, H, W, _ = h0.shape
    q = h0.view(N, H // 2, 2, W // 2, 2, C0)
    p0 = rb(0.25 * (q[:, :, 0, :, 0] + q[:, :, 0, :, 1] + q[:, :, 1, :, 0] + q[:, :, 1, :, 1]))
    sc = rb(p0 @ wsc.to(dt).t() + bsc.to(dt))
    return h0, h1, p0, sc


def dh0_of(dh1, dp0, w1_bwd, dt):
    """dh0 = dh1 W1 + 0.25 expand(dp0), rounded to bf16.  -> [N, H, W, 32]"""
    e = dp0.to(dt).repeat_interleave(2, 1).repeat_interleave(2, 2)
    return rb(dh1.to(dt) @ w1_bwd.to(dt)[:, :C1].t() + 0.25 * e)


def backward(img32, w_in, b_in, dh1, dp0, w1_bwd, dt):
    """-> dW_in [9][32], db_in [32], dW1 [16][32], db1 [16]."""
    h0 = h0_of(img32, w_in, b_in, dt)
    dh0 = dh0_of(dh1, dp0, w1_bwd, dt)
    g = dh1.to(dt)
    dw1 = torch.einsum("nhwo,nhwc->oc", g, h0)
    db1 = g.sum((0, 1, 2))
    hi, lo = (t.to(dt) for t in split(img32))
    dw_in = torch.stack([torch.einsum("nhw,nhwc->c", _shift(hi, tap), dh0) + torch.einsum("nhw,nhwc->c", _shift(lo, tap), dh0) for tap in range(9)])
    return dw_in, dh0.sum((0, 1, 2)), dw1, db1


def dimg_of(dh1, dp0, w1_bwd, w_in, dt):
    """d img = input_conv^T dh0: the nine per-tap dot products s[tap][q] = sum_c dh0[q, c] bf16(w[8 - tap][c]) (flipped taps), summed over
    the taps at q = p + d(tap), dh0 zero outside the image.  -> [N, H, W]"""
    dh0 = dh0_of(dh1, dp0, w1_bwd, dt)
    w = rb(w_in.to(dt))
    out = torch.zeros(dh0.shape[:3], dtype=dt)
    for tap in range(9):
        out += _shift((dh0 * w[8 - tap]).sum(-1), tap)
    return out


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def synth_image(n, h, w, seed):
    """PXD-like image as bench.synth_event makes it: background -1, ~1 % log-normalised hits, 4e-3 dequantisation noise.  -> fp32 [N, H, W]"""
    rng = np.random.Generator(np.random.PCG64([seed, 77]))
    hit = rng.random((n, 1, h, w)) < 0.01
    u = rng.uniform(0.03, 1.0, (n, 1, h, w))
    img = np.where(hit, np.log(255.0 * u + 1.0) / np.log(256.0), 0.0) + 4e-3 * rng.random((n, 1, h, w))
    return torch.from_numpy((2.0 * img - 1.0).astype(np.float32))[:, 0].contiguous()


def inputs(n, h, w, seed=0):
    """Seeded operands of one case.  Weights and gradients that the kernels read as bf16 are fp32 tensors holding bf16 values."""
    g = torch.Generator().manual_seed(1000 + seed)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    w1 = rn(C1, C0, scale=0.25).to(BF16).float()
    w1_bwd = torch.zeros(C0, 32)
    w1_bwd[:, :C1] = w1.t()
    return dict(img=synth_image(n, h, w, 505 + seed), w_in=rn(9, C0, scale=0.3), b_in=rn(C0, scale=0.1), w1=w1, b1=rn(C1, scale=0.1),
                wsc=rn(CS, C0, scale=0.2).to(BF16).float(), bsc=rn(CS, scale=0.1), w1_bwd=w1_bwd,
                dh1=rn(n, h, w, C1).to(BF16).float(), dp0=rn(n, h // 2, w // 2, C0).to(BF16).float())
