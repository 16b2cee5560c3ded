"""Per-operator parity of the HIP kernels (through the C ABI / ops.py) on a real MI355X.

Checker: plain fp32 PyTorch of the same operator on the same bf16-rounded inputs (and, for the
module-level cases, the reference-generated golden vectors in tests/golden/).  bf16 tolerance: outputs
are rounded to bf16 (8 mantissa bits) and the A operand is re-rounded after the fused prologue, so the
bound is 1.5e-2 * max|ref| per element (tighter for fp32-in/fp32-out kernels).
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    import _hip
    _hip.require_gpu()
    _hip.lib()
    return torch.device("cuda:0")


def close(a, b, tol, what=""):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    scale = max(b.abs().max().item(), 1e-3)
    assert err <= tol * scale, f"{what}: max|diff|={err:.4e} vs scale {scale:.4e} (tol {tol})"


def r16(t):
    return t.to(BF).float()


def nhwc(t):   # NCHW fp32 -> NHWC bf16 contiguous
    return t.permute(0, 2, 3, 1).contiguous().to(BF)


def nchw(t):   # NHWC -> NCHW fp32
    return t.float().permute(0, 3, 1, 2).contiguous()


def sn_ref(W, u, eps=1e-6):
    Wm = W.reshape(W.shape[0], -1)
    with torch.no_grad():
        v = F.normalize(u @ Wm, eps=eps)
        u2 = F.normalize(v @ Wm.t(), eps=eps)
    sigma = ((v @ Wm.t()) @ u2.t()).squeeze()
    return W / sigma, u2, sigma


def make_rec(W, u, sv, kind=None):
    """Run the batched SN kernel on a tiny private arena holding (W, u, sv)."""
    import ops
    flat = torch.cat([W.reshape(-1), u.reshape(-1), sv.reshape(-1)]).contiguous()
    Wv = flat[:W.numel()].view(W.shape)
    uv = flat[W.numel():W.numel() + u.numel()].view(u.shape)
    svv = flat[W.numel() + u.numel():].view(sv.shape)
    if kind is None:
        kind = ops.KIND_CONV if W.dim() == 4 else ops.KIND_PLAIN
    bank = ops.SNBank(flat, [("l", kind, Wv, uv, svv)])
    rec = bank.run(True, 1e-6)["l"]
    return rec, Wv, uv, svv


def test_tr_read_selftest(dev):
    """ds_read_b64_tr_b16 delivers the MFMA B fragment the wgrad kernel assumes."""
    import _hip
    src = torch.arange(64 * 16, device=dev, dtype=torch.float32).view(64, 16).to(BF)
    out = torch.zeros(64, 8, device=dev, dtype=BF)
    _hip.call("ieagan_selftest_tr_read", src.data_ptr(), out.data_ptr(), _hip.stream())
    torch.cuda.synchronize()
    lanes = torch.arange(64, device=dev)
    exp = torch.stack([src[8 * (lanes >> 4) + j, lanes & 15] for j in range(8)], 1)
    assert torch.equal(out, exp), (out[:20], exp[:20])


@pytest.mark.parametrize("out_f,in_shape", [(48, (32, 3, 3)), (16, (64, 1, 1)), (128, (132,)), (40, (1024,)), (24576, (256,))])
def test_sn_forward_backward(dev, out_f, in_shape):
    import ops
    torch.manual_seed(0)
    W = (torch.randn(out_f, *in_shape, device=dev) / math.sqrt(np.prod(in_shape))).requires_grad_(True)
    u = torch.randn(1, out_f, device=dev)
    rec, Wv, uv, svv = make_rec(W.detach(), u, torch.ones(1, device=dev))
    Wsn, u2, sigma = sn_ref(W, u)
    close(rec.ctx[0:1], sigma.view(1), 1e-5, "sigma")
    close(uv, u2, 1e-4, "u update")
    close(svv, sigma.view(1), 1e-5, "sv")
    inn = int(np.prod(in_shape))
    if rec.kind == ops.KIND_CONV:
        taps, cin = rec.taps, rec.cin
        exp = Wsn.detach().view(out_f, cin, taps).permute(0, 2, 1).reshape(out_f, taps * cin)
        close(rec.w_fwd[:, :taps * cin], exp, 1e-2, "fwd pack")
        assert float(rec.w_fwd[:, taps * cin:].float().abs().sum()) == 0.0
        expb = Wsn.detach().view(out_f, cin, taps).flip(2).permute(1, 2, 0).reshape(cin, taps * out_f)
        close(rec.w_bwd[:, :taps * out_f], expb, 1e-2, "dgrad pack")
        g = torch.randn(out_f, rec.kpad, device=dev)
        g[:, taps * cin:] = 0
        g_param = g[:, :taps * cin].view(out_f, taps, cin).permute(0, 2, 1).reshape(W.shape)
    else:
        close(rec.w_plain, Wsn.detach().view(out_f, inn), 1e-5, "plain pack")
        g = torch.randn(out_f, inn, device=dev)
        g_param = g.view(W.shape)
    (ref,) = torch.autograd.grad(Wsn, [W], g_param)
    got = ops.sn_backward(g.contiguous(), Wv, rec)[0]
    close(got, ref, 1e-4, "sn backward")


CONV_CASES = [
    # taps Cin Cout H  W  aff   relu  rs residual            stats
    (9, 32, 48, 10, 14, False, False, 0, None, False),
    (9, 16, 16, 12, 20, True, True, 0, None, True),
    (9, 64, 64, 6, 10, True, True, 1, None, True),          # upsampled source (GBlock.conv2)
    (9, 128, 128, 4, 12, False, True, 0, None, False),
    (1, 64, 16, 9, 7, True, True, 0, None, True),
    (1, 16, 64, 8, 12, True, True, 0, ("same", 64, 64), True),   # GBlock.conv4, same resolution
    (1, 16, 32, 8, 12, True, True, 0, ("up", 64, 32), True),     # GBlock.conv4 + upsampled, channel-dropped shortcut
    (1, 16, 64, 4, 6, False, True, 2, ("pool+sc", 32, 32), False),  # DBlock.conv4 + pooled concat shortcut
    (1, 32, 32, 4, 6, False, False, 2, None, False),             # DBlock.conv_sc on the pooled input
    (1, 512, 128, 4, 12, True, True, 0, None, True),
    (1, 128, 512, 4, 12, False, True, 0, None, False),
    (9, 32, 32, 17, 48, True, True, 0, None, True),          # halo kernel, ragged rows (17 % 8 != 0)
    (9, 16, 16, 24, 96, False, True, 0, None, False),        # halo kernel, Cin = 16 (two taps per MFMA K step)
    (9, 128, 128, 8, 24, True, True, 0, None, True),         # halo kernel, ragged columns (24 % 32 != 0), 2 cout chunks
    (9, 64, 64, 8, 24, True, True, 1, None, True),           # halo kernel with upsampled source
]


def test_halo_and_gather_kernels_agree(dev):
    """The LDS-halo 3x3 kernel and the direct-gather kernel compute the same convolution."""
    import _hip, ops
    torch.manual_seed(7)
    N, Hh, Ww, Cin, Cout = 2, 19, 40, 32, 64
    x = torch.randn(N, Hh, Ww, Cin, device=dev).to(BF)
    w = (torch.randn(Cout, 9 * Cin, device=dev) / 17).to(BF)
    sc, sh = 1 + 0.3 * torch.randn(N, Cin, device=dev), 0.2 * torch.randn(N, Cin, device=dev)
    outs = []
    for force in (0, _hip.CONV_FORCE_GATHER):      # per-call flag of the conv descriptor (no process-wide switch)
        out = torch.empty(N, Hh, Ww, Cout, device=dev, dtype=BF)
        st = ops.new_stats(Cout, dev)
        ops._conv_launch(x, Cin, Hh, Ww, 0, sc, sh, Cin, True, N, Hh, Ww, Cin, Cout, 9, 9 * Cin, w, None, None, 0, 0, 0, None, 0,
                         None, out, st, flags=force)
        outs.append((out, st.sum((0, 1))))
    close(outs[0][0], outs[1][0], 4e-3, "halo vs gather out")
    close(outs[0][1], outs[1][1], 1e-3, "halo vs gather stats")


@pytest.mark.parametrize("N,Hh,Ww,C", [(40, 64, 192, 64),      # C = 64: conv3x3_ws64 (8x16 tiles) / halo kernel, weights from L1
                                       (6, 32, 96, 64),        # C = 64 on a small map
                                       (5, 20, 40, 64),        # C = 64, ragged tiles (20 % 16, 40 % 32)
                                       (4, 16, 48, 128),       # C = 128: conv3x3_lds (4 waves, 8x16 tiles)
                                       (3, 8, 24, 128),        # C = 128 on the 8x24 map (ragged columns)
                                       (8, 128, 96, 32),       # C = 32: prefetching variant, unrolled K loop
                                       (4, 100, 70, 16),       # C = 16: prefetching variant, ragged tiles
                                       (12, 100, 200, 16),     # C = 16, >= 1024 tiles: conv3x3_ws (producer / consumer waves), ragged tiles
                                       (2, 256, 768, 16),      # C = 16 at the production map: conv3x3_ws, 3 tiles per persistent block
                                       (6, 128, 384, 32),      # C = 32 at its production map (conv3x3_halo, persistent-prefetch variant)
                                       (11, 100, 232, 32)])    # C = 32, >= 1024 ragged tiles
def test_specialised_halo_variants_agree_with_gather(dev, N, Hh, Ww, C):
    """Every channel-specialised 3x3 kernel (compile-time K loop, software pipeline, LDS weights, register prefetch of the
    next tile, producer / consumer waves) against the plain gather kernel on the same operands: ReLU prologue + ReLU-mask
    epilogue + statistics together, and the two combinations the train step issues (forward: ReLU prologue, statistics;
    dgrad: plain prologue, ReLU mask) -- conv3x3_ws only takes those."""
    import _hip, ops
    torch.manual_seed(9)
    x = torch.randn(N, Hh, Ww, C, device=dev).to(BF)
    kpad = ops._kpad(9 * C)
    w = torch.zeros(C, kpad, device=dev)
    w[:, :9 * C] = torch.randn(C, 9 * C, device=dev) / math.sqrt(9 * C)
    w = w.to(BF)
    bias = 0.1 * torch.randn(C, device=dev)
    mask = torch.randn(N, Hh, Ww, C, device=dev).to(BF)
    for relu, mk in ((True, mask), (True, None), (False, mask)):
        outs = []
        for force in (0, _hip.CONV_FORCE_GATHER, _hip.CONV_NO_LDS_WEIGHTS):      # conv3x3_lds / conv3x3_ws | conv_gather | conv3x3_halo
            out = torch.empty(N, Hh, Ww, C, device=dev, dtype=BF)
            st = ops.new_stats(C, dev)
            ops._conv_launch(x, C, Hh, Ww, 0, None, None, 0, relu, N, Hh, Ww, C, C, 9, kpad, w, bias, None, 0, 0, 0, None, 0, mk, out, st,
                             flags=force)
            outs.append((out, st.sum((0, 1))))
        tag = f"relu={relu} mask={mk is not None}: "
        close(outs[0][0], outs[1][0], 4e-3, tag + "lds / ws / halo vs gather out")
        close(outs[0][1], outs[1][1], 2e-3, tag + "lds / ws / halo vs gather stats")
        close(outs[2][0], outs[1][0], 4e-3, tag + "halo vs gather out")
        close(outs[2][1], outs[1][1], 2e-3, tag + "halo vs gather stats")


# name: (C, N, H, W, flags that select the first family, events, (H, W) of the BatchNorm-backward variant).  The second family is always
# conv3x3_halo (CONV_NO_LDS_WEIGHTS).  The launcher accepts per-group statistics only for groups of a whole number of 128-pixel blocks
# (n_per_event * H * W % 128 == 0, whatever kernel takes the launch): the two events of the ws pair need H * W % 32 == 0, hence 124x248,
# and the per-image accumulators of a BatchNorm-backward dgrad need H * W % 128 == 0, hence a shape of its own per pair (same tile counts
# per image, still ragged in one direction).
TILE_PAIRS = {
    "lds_8wave_c64": (64, 25, 20, 40, "CONV_NO_WS64", 1, (24, 48)),     # 100 tile pairs: the least that selects the 8-wave form; ragged both ways
    "lds_4wave_c64": (64, 2, 12, 40, "CONV_NO_WS64", 1, (24, 48)),
    "lds_c128": (128, 2, 12, 24, None, 1, (12, 32)),
    "ws_c16": (16, 8, 124, 248, None, 2, (124, 256)),                   # 1024 ragged tiles: the least conv3x3_ws accepts; two events
}
TILE_VARIANTS = ("ccbn", "ccbn_up", "mask", "bnb")


def tile_variant_launch(dev, C, N, Hh, Ww, variant, flags, events):
    """One launch of a TILE_PAIRS shape on seeded operands: BatchNorm prologue + ReLU + statistics (`ccbn`), the same on an up-sampled
    source (`ccbn_up`), ReLU-mask dgrad (`mask`), BatchNorm-backward dgrad (`bnb`).  Returns (out, raw statistics or None); the
    statistics buffer has one slot per block of a group, so every slot has a single adder."""
    import ops
    g = torch.Generator(device="cpu").manual_seed(1000 + C + Hh + len(variant))
    up = variant == "ccbn_up"
    Hs, Ws = (Hh // 2, Ww // 2) if up else (Hh, Ww)
    x = torch.randn(N, Hs, Ws, C, generator=g).to(dev).to(BF)
    kpad = ops._kpad(9 * C)
    w = torch.zeros(C, kpad)
    w[:, :9 * C] = torch.randn(C, 9 * C, generator=g) / math.sqrt(9 * C)
    w = w.to(dev).to(BF)
    bias = (0.1 * torch.randn(C, generator=g)).to(dev)
    sc = (1 + 0.3 * torch.randn(N, C, generator=g)).to(dev)
    sh = (0.2 * torch.randn(N, C, generator=g)).to(dev)
    xin = (torch.randn(N, Hh, Ww, C, generator=g) * 1.3 + 0.2).to(dev).to(BF)      # ReLU mask / BatchNorm input
    out = torch.full((N, Hh, Ww, C), float("nan"), device=dev, dtype=BF)
    if variant in ("ccbn", "ccbn_up"):
        st = ops._conv_launch(x, C, Hs, Ws, int(up), sc, sh, C, True, N, Hh, Ww, C, C, 9, kpad, w, bias, None, 0, 0, 0, None, 0, None, out,
                              True, npe=N // events, flags=flags)
    elif variant == "mask":
        st = ops._conv_launch(x, C, Hs, Ws, 0, None, None, 0, False, N, Hh, Ww, C, C, 9, kpad, w, None, None, 0, 0, 0, None, 0, xin, out,
                              None, flags=flags)
    else:
        st = ops._conv_launch(x, C, Hs, Ws, 0, None, None, 0, False, N, Hh, Ww, C, C, 9, kpad, w, None, None, 0, 0, 0, None, 0, xin, out,
                              True, npe=1, flags=flags, bnb=(sc, sh, C, True))
    return out, st


@pytest.mark.parametrize("pair", list(TILE_PAIRS))
def test_3x3_tile_kernels_agree_bit_for_bit(dev, pair):
    """The same launch through two 3x3 tile-kernel families (conv3x3_lds in its three forms / conv3x3_ws against conv3x3_halo).  Every
    family accumulates each output element over the same k-steps in the same order, so the outputs must agree bit for bit; the folded
    statistics (per group: events, or images for the BatchNorm-backward accumulators) to 1e-5 relative, norm of the difference over the
    norm of the reference vector -- the block partials are added in a different order.  This pins the request, prologue, swizzle,
    K-loop and pixel-mapping code the families share (conv3x3_tile.h) against conv3x3_halo's own copy of it."""
    import _hip
    C, N, Hh, Ww, first, events, bnb_hw = TILE_PAIRS[pair]
    for variant in TILE_VARIANTS:
        hw = bnb_hw if variant == "bnb" else (Hh, Ww)
        res = [tile_variant_launch(dev, C, N, hw[0], hw[1], variant, fl, events)
               for fl in (getattr(_hip, first) if first else 0, _hip.CONV_NO_LDS_WEIGHTS)]
        (o1, s1), (o0, s0) = res
        assert torch.isfinite(o0.float()).all() and torch.isfinite(o1.float()).all(), (pair, variant)
        nd = int((o1 != o0).sum())
        print(f"{pair} {variant}: differing outputs {nd} of {o0.numel()}")
        assert torch.equal(o1, o0), (pair, variant, nd, float((o1.float() - o0.float()).abs().max()))
        if s1 is not None:
            f1, f0 = s1.sum(1).double(), s0.sum(1).double()             # [groups, 2, C]
            for k in range(2):
                r = float((f1[:, k] - f0[:, k]).norm() / max(float(f0[:, k].norm()), 1e-30))
                print(f"{pair} {variant}: statistics row {k} rel {r:.2e}")
                assert float(f0[:, k].abs().max()) > 0 and r <= 1e-5, (pair, variant, k, r)


def test_ws_kernel_affine_prologue_and_event_statistics(dev):
    """conv3x3_ws with the ccbn prologue (per-image scale / shift staged per producer wave), an upsampled source and per-event
    statistics, against conv3x3_halo on the same operands (the halo kernel itself is checked against fp32 PyTorch below)."""
    import _hip, ops
    torch.manual_seed(10)
    N, E = 8, 2
    for C, rs, (Hs, Ws) in ((16, 0, (128, 384)), (16, 1, (64, 192)), (32, 0, (128, 384)), (32, 1, (64, 192))):
        Hh, Ww = (Hs, Ws) if rs == 0 else (2 * Hs, 2 * Ws)
        x = torch.randn(N, Hs, Ws, C, device=dev).to(BF)
        kpad = ops._kpad(9 * C)
        w = torch.zeros(C, kpad, device=dev)
        w[:, :9 * C] = torch.randn(C, 9 * C, device=dev) / math.sqrt(9 * C)
        w = w.to(BF)
        bias = 0.1 * torch.randn(C, device=dev)
        sc = 1 + 0.2 * torch.randn(N, C, device=dev)
        sh = 0.2 * torch.randn(N, C, device=dev)
        res = []
        for force in (0, _hip.CONV_NO_LDS_WEIGHTS):
            out = torch.empty(N, Hh, Ww, C, device=dev, dtype=BF)
            st = ops.new_stats(C, dev, E)
            ops._conv_launch(x, C, Hs, Ws, rs, sc, sh, C, True, N, Hh, Ww, C, C, 9, kpad, w, bias, None, 0, 0, 0, None, 0, None, out, st,
                             npe=N // E, flags=force)
            res.append((out, st.sum(1)))
        close(res[0][0], res[1][0], 4e-3, f"C={C} rs={rs}: ws vs halo out")
        close(res[0][1], res[1][1], 2e-3, f"C={C} rs={rs}: ws vs halo per-event stats")
        assert (res[0][1][0] - res[0][1][1]).abs().max() > 0       # the two events really have different statistics


@pytest.mark.parametrize("Cin,Cout,Hh,Ww,N,aff,relu,res,mask,events", [
    (16, 32, 256, 768, 2, True, True, "up", False, 2),       # G b11 conv4: 4 m-tiles per wave, half-resolution shortcut, per-event statistics
    (16, 64, 128, 384, 4, False, True, "same", True, 1),     # D s0.1 conv4 dgrad-like: mask + same-resolution residual
    (32, 16, 256, 768, 2, False, False, None, True, 1),      # one n-tile (Cout = 16), mask
    (64, 16, 128, 384, 4, True, True, None, False, 2),       # two k-steps, one n-tile, statistics of two events
    (32, 64, 128, 384, 4, True, False, "cat", False, 1),     # residual A on channels [0, 32) + residual B on [32, 64)
    (128, 32, 64, 192, 12, False, True, None, False, 1),     # four k-steps
    (64, 128, 64, 192, 12, True, True, "pool", False, 1),    # grid.y = 2, double-resolution shortcut (2x2 average)
    (256, 256, 8, 24, 40, False, False, None, False, 1),     # conv1x1_tile on an 8x24 map (60 pixel blocks x 4 n-tile columns, round 4)
    (128, 256, 32, 96, 8, False, True, "same", True, 1),     # wide expansion: conv1x1_tile instead of conv1x1_stream, 4 columns share the pixels
    (64, 256, 32, 96, 8, True, True, None, False, 2),        # Cin = 64 / Cout = 256 with the BatchNorm prologue, two events
])
def test_streaming_1x1_agrees_with_gather(dev, Cin, Cout, Hh, Ww, N, aff, relu, res, mask, events):
    """conv1x1_stream (prefetched operands, weights in registers, per-block statistics) and conv1x1_tile (LDS-tiled; the last three cases)
    against conv_gather (one tile per block) on identical operands: same outputs bit for bit (same MFMA order per output) and the same
    per-event statistics."""
    import _hip, ops
    torch.manual_seed(21)
    x = torch.randn(N, Hh, Ww, Cin, device=dev).to(BF)
    kpad = ops._kpad(Cin)
    w = torch.zeros(Cout, kpad, device=dev)
    w[:, :Cin] = torch.randn(Cout, Cin, device=dev) / math.sqrt(Cin)
    w = w.to(BF)
    bias = 0.1 * torch.randn(Cout, device=dev)
    sc = (1 + 0.3 * torch.randn(N, Cin, device=dev)) if aff else None
    sh = (0.2 * torch.randn(N, Cin, device=dev)) if aff else None
    mk = torch.randn(N, Hh, Ww, Cout, device=dev).to(BF) if mask else None
    ra = rb = None
    Cra = Ca = ra_rs = Crb = 0
    if res == "same":
        ra, Cra, Ca = torch.randn(N, Hh, Ww, Cout, device=dev).to(BF), Cout, Cout
    elif res == "up":
        ra, Cra, Ca, ra_rs = torch.randn(N, Hh // 2, Ww // 2, 2 * Cout, device=dev).to(BF), 2 * Cout, Cout, 1
    elif res == "pool":
        ra, Cra, Ca, ra_rs = torch.randn(N, 2 * Hh, 2 * Ww, Cout, device=dev).to(BF), Cout, Cout, 2
    elif res == "cat":
        ra, Cra, Ca = torch.randn(N, Hh, Ww, Cout // 2, device=dev).to(BF), Cout // 2, Cout // 2
        rb, Crb = torch.randn(N, Hh, Ww, Cout // 2, device=dev).to(BF), Cout // 2
    outs = []
    for force in (0, _hip.CONV_FORCE_GATHER):
        out = torch.empty(N, Hh, Ww, Cout, device=dev, dtype=BF)
        st = ops.new_stats(Cout, dev, events)
        ops._conv_launch(x, Cin, Hh, Ww, 0, sc, sh, Cin if aff else 0, relu, N, Hh, Ww, Cin, Cout, 1, kpad, w, bias, ra, Cra, Ca, ra_rs,
                         rb, Crb, mk, out, st, npe=N // events, flags=force)
        outs.append((out, st.sum(1)))
    assert torch.equal(outs[0][0], outs[1][0]), float((outs[0][0].float() - outs[1][0].float()).abs().max())
    close(outs[0][1], outs[1][1], 1e-4, "stream vs gather statistics")
    if events > 1:
        assert not torch.allclose(outs[0][1][0], outs[0][1][1])          # the events really are separate accumulators


@pytest.mark.parametrize("N,Hh,Ww,C,aff", [(24, 64, 192, 64, False), (84, 32, 96, 64, True), (170, 20, 40, 64, False), (8, 64, 192, 64, False),
                                            (4, 16, 48, 128, True), (3, 8, 24, 128, False)])
def test_fp8_forward_conv_vs_bf16_and_fp32(dev, N, Hh, Ww, C, aff):
    """BASELINE configs[4]: the C = 64 / 128 3x3 forward launches with OCP e4m3 MFMA operands (per-slice weight scale, per-tile
    activation scale, fp32 accumulate).  Stated tolerance: relative L2 error of the output <= 4e-2 against fp32 (e4m3 carries 3
    mantissa bits: ~3 % per product; measured 3.5e-2), vs <= 6e-3 for the bf16 operands (measured 1.7e-3); statistics <= 5e-2."""
    import _hip, ops
    torch.manual_seed(31)
    x = torch.randn(N, Hh, Ww, C, device=dev).to(BF)
    kpad = ops._kpad(9 * C)
    wf = torch.randn(C, C, 3, 3, device=dev) / math.sqrt(9 * C)
    w = wf.permute(0, 2, 3, 1).reshape(C, 9 * C).to(BF).contiguous()
    bias = 0.1 * torch.randn(C, device=dev)
    sc = (1 + 0.3 * torch.randn(N, C, device=dev)) if aff else None
    sh = (0.2 * torch.randn(N, C, device=dev)) if aff else None
    a = x.float().permute(0, 3, 1, 2)
    if aff:
        a = a * sc[:, :, None, None] + sh[:, :, None, None]
    a = F.relu(a)
    ref = F.conv2d(a, w.float().view(C, 3, 3, C).permute(0, 3, 1, 2), bias, 1, 1)
    outs = {}
    for name, flags in (("bf16", 0), ("fp8", _hip.CONV_FP8), ("fp8_k32", _hip.CONV_FP8 | _hip.CONV_FP8_NOSCALE)):
        out = torch.empty(N, Hh, Ww, C, device=dev, dtype=BF)
        st = ops.new_stats(C, dev)
        ops._conv_launch(x, C, Hh, Ww, 0, sc, sh, C if aff else 0, True, N, Hh, Ww, C, C, 9, kpad, w, bias, None, 0, 0, 0, None, 0, None, out, st,
                         flags=flags)
        outs[name] = (nchw(out), st.sum((0, 1)))
    rel = lambda t: float((t - ref).norm() / ref.norm())
    e16, e8 = rel(outs["bf16"][0]), rel(outs["fp8"][0])
    print(f"rel-L2 vs fp32: bf16 {e16:.2e}, fp8 {e8:.2e}")
    assert e16 <= 6e-3 and e8 <= 4e-2, (e16, e8)
    if C == 64 and N * ((Hh + 7) // 8) * ((Ww + 31) // 32) < 1000:
        # C = 64 below 1000 tile-blocks keeps bf16 operands whatever the flag says (conv3x3_lds.hip, lds_fp8_launch: the 8-wave fp8
        # form is slower than the 4-wave bf16 form there): the flag must then change NOTHING
        assert torch.equal(outs["fp8"][0], outs["bf16"][0])
        return
    assert e8 > e16                                        # the fp8 path really ran with fp8 operands
    # the block-scaled K = 128 instruction (all block scales 1) sums the SAME e4m3 products as four K = 32 instructions: only the
    # fp32 accumulation order differs (a wrong k pairing of the two operands would be an O(1) error)
    d = float((outs["fp8"][0] - outs["fp8_k32"][0]).norm() / outs["fp8_k32"][0].norm())
    assert d <= 4e-3, d                                    # (outputs are bf16-rounded: a last-bit flip here and there)
    close(outs["fp8"][1][0], ref.sum((0, 2, 3)), 5e-2, "fp8 stat sum")
    close(outs["fp8"][1][1], (ref * ref).sum((0, 2, 3)), 5e-2, "fp8 stat sumsq")


def conv_reference(x, W, u, bias, scale, shift, relu, rs, taps, ra, ra_mode, Ca, rb):
    """fp32 NCHW composite with the kernel's rounding points (A operand and weights in bf16)."""
    a = x
    if scale is not None:
        a = a * scale[:, :, None, None] + shift[:, :, None, None]
    if relu:
        a = F.relu(a)
    if rs == 1:
        a = F.interpolate(a, scale_factor=2)
    elif rs == 2:
        a = F.avg_pool2d(a, 2)
    a = a + (r16(a) - a).detach()          # straight-through bf16 rounding of the MFMA operand
    Wsn, _, _ = sn_ref(W, u)
    Wq = Wsn + (r16(Wsn) - Wsn).detach()
    out = F.conv2d(a, Wq, bias, 1, 1 if taps == 9 else 0)
    if ra is not None:
        r = ra[:, :Ca]
        if ra_mode == 1:
            r = F.interpolate(r, scale_factor=2)
        elif ra_mode == 2:
            r = F.avg_pool2d(r, 2)
        if rb is not None:
            r = torch.cat([r, rb], 1)
        elif Ca < out.shape[1]:
            r = F.pad(r, (0, 0, 0, 0, 0, out.shape[1] - Ca))
        out = out + r
    return out


# The layers the benchmark spends its time in, at their production geometry (model.py:86-95, 573-582 with ch = 32), on a
# few images: forward + dgrad (incl. effgrad / prologue_bwd) + wgrad of every specialised kernel variant against fp32
# PyTorch -- not against another HIP kernel.   (N chosen so that the launcher takes the same variant as at N = 40.)
PROD_CASES = [
    # taps Cin Cout H    W    aff    relu  rs residual               stats  N
    (9, 16, 16, 256, 768, True, True, 0, None, True, 2),             # G b11 conv3: C=16 persistent-prefetch halo, ccbn prologue
    (9, 16, 16, 256, 768, False, True, 0, None, False, 2),           # D s0.0 conv2/3: bare-ReLU prologue, fused mask in dgrad
    (9, 16, 16, 128, 384, True, True, 1, None, True, 2),             # G b11 conv2: upsampled source 128x384 -> 256x768
    (9, 32, 32, 128, 384, True, True, 0, None, True, 3),             # G b9 conv3: C=32 prefetch variant
    (9, 32, 32, 128, 384, False, True, 0, None, False, 3),           # D s1.0 conv2/3
    (9, 64, 64, 64, 192, False, True, 0, None, False, 22),           # D s2.0: C=64 LDS-resident weights (>= 1024 tiles)
    (9, 64, 64, 32, 96, True, True, 0, None, True, 6),               # G b5/b6: C=64 pipelined K loop
    (9, 128, 128, 16, 48, True, True, 0, None, True, 8),             # G b3/b4, D s4.0: C=128
    (1, 16, 32, 256, 768, True, True, 0, ("up", 64, 32), True, 2),   # G b11 conv4 + upsampled, channel-dropped shortcut
    (1, 64, 16, 128, 384, True, True, 0, None, True, 3),             # G b10/b11 conv1 (streaming 1x1 kernel from 1024 pixel groups)
    (1, 32, 16, 256, 768, False, False, 0, None, False, 2),          # D s0.0 conv1 (first block: no pre-activation)
    (1, 16, 64, 128, 384, False, True, 2, ("pool+sc", 32, 32), False, 2),   # D s0.0 conv4: pooled source + concat shortcut
    (1, 32, 32, 128, 384, False, False, 2, None, False, 2),          # D s0.0 conv_sc on the pooled block input
    (1, 16, 64, 128, 384, False, True, 0, ("same", 64, 64), False, 3),      # D s0.1 conv4 + identity shortcut
]


@pytest.mark.parametrize("case", CONV_CASES + PROD_CASES,
                         ids=[f"c{i}" for i in range(len(CONV_CASES))] + [f"prod{i}" for i in range(len(PROD_CASES))])
def test_conv_forward_backward(dev, case):
    import ops
    taps, Cin, Cout, Hs, Ws, aff, relu, rs, res, stats = case[:10]
    torch.manual_seed(1)
    N = case[10] if len(case) > 10 else 3
    k = 3 if taps == 9 else 1
    x = r16(torch.randn(N, Cin, Hs, Ws, device=dev)).requires_grad_(True)
    W = (torch.randn(Cout, Cin, k, k, device=dev) / math.sqrt(Cin * taps)).requires_grad_(True)
    u = torch.randn(1, Cout, device=dev)
    bias = (0.1 * torch.randn(Cout, device=dev)).requires_grad_(True)
    scale = shift = None
    if aff:
        scale = (1 + 0.3 * torch.randn(N, Cin, device=dev)).requires_grad_(True)
        shift = (0.2 * torch.randn(N, Cin, device=dev)).requires_grad_(True)
    Hc, Wc = (2 * Hs, 2 * Ws) if rs == 1 else (Hs // 2, Ws // 2) if rs == 2 else (Hs, Ws)
    ra = rb = None
    ra_mode, Ca = 0, 0
    if res is not None:
        kind, Cra, Ca = res
        if kind == "same":
            ra = r16(torch.randn(N, Cra, Hc, Wc, device=dev)).requires_grad_(True)
        elif kind == "up":
            ra, ra_mode = r16(torch.randn(N, Cra, Hc // 2, Wc // 2, device=dev)).requires_grad_(True), 1
        else:
            ra, ra_mode = r16(torch.randn(N, Cra, 2 * Hc, 2 * Wc, device=dev)).requires_grad_(True), 2
            rb = r16(torch.randn(N, Cout - Ca, Hc, Wc, device=dev)).requires_grad_(True)
    ref = conv_reference(x, W, u, bias, scale, shift, relu, rs, taps, ra, ra_mode, Ca, rb)
    go = r16(torch.randn_like(ref))
    # reference statistics path: loss also depends on sum / sumsq of the output
    dsum = 0.05 * torch.randn(2, Cout, device=dev)
    loss_ref = (ref * go).sum()
    if stats:
        loss_ref = loss_ref + (ref.sum((0, 2, 3)) * dsum[0]).sum() + ((ref * ref).sum((0, 2, 3)) * dsum[1]).sum()
    leaves = [t for t in (x, W, bias, scale, shift, ra, rb) if t is not None]
    grads_ref = torch.autograd.grad(loss_ref, leaves)

    # ---- HIP path
    rec, Wv, uv, svv = make_rec(W.detach(), u, torch.ones(1, device=dev))
    Wp = Wv.detach().requires_grad_(True)
    xa = nhwc(x.detach()).requires_grad_(True)
    b2 = bias.detach().clone().requires_grad_(True)
    sc2 = scale.detach().clone().requires_grad_(True) if aff else None
    sh2 = shift.detach().clone().requires_grad_(True) if aff else None
    ra2 = nhwc(ra.detach()).requires_grad_(True) if ra is not None else None
    rb2 = nhwc(rb.detach()).requires_grad_(True) if rb is not None else None
    out, st = ops.conv(xa, Wp, b2, rec, taps, scale=sc2, shift=sh2, relu=relu, rs=rs, ra=ra2, Ca=Ca, ra_rs=ra_mode, rb=rb2,
                       want_stats=stats)
    close(nchw(out), ref, 1.5e-2, "conv out")
    loss = (out.float() * nhwc(go).float()).sum()
    if stats:
        ssum = st.sum((0, 1))
        close(ssum[0], ref.sum((0, 2, 3)), 2e-2, "stat sum")
        close(ssum[1], (ref * ref).sum((0, 2, 3)), 2e-2, "stat sumsq")
        loss = loss + (st.sum((0, 1)) * dsum).sum()
    leaves2 = [t for t in (xa, Wp, b2, sc2, sh2, ra2, rb2) if t is not None]
    grads = torch.autograd.grad(loss, leaves2)
    names = [n for n, t in zip(("x", "W", "bias", "scale", "shift", "ra", "rb"), (x, W, bias, scale, shift, ra, rb)) if t is not None]
    for n, g, gr in zip(names, grads, grads_ref):
        if n in ("x", "ra", "rb"):
            g = nchw(g)
        close(g, gr, 3e-2, f"grad {n}")


def test_wgrad_tr_vs_scalar_reads(dev):
    """The transposed-read operand path and the scalar-read reference path agree bit for bit in fp32 sums
    up to atomic ordering."""
    import _hip, ops
    torch.manual_seed(3)
    N, Hh, Ww, Cin, Cout = 2, 16, 32, 32, 48
    x = torch.randn(N, Hh, Ww, Cin, device=dev).to(BF)
    g = torch.randn(N, Hh, Ww, Cout, device=dev).to(BF)
    outs = []
    for tr in (1, 0):
        dw = torch.zeros(Cout, 9 * Cin, device=dev)
        d = _hip.WgradDesc(N, Hh, Ww, Cin, Cout, 9, 9 * Cin, _hip.src_desc(x, Cin, Hh, Ww), g.data_ptr(), Cout, dw.data_ptr(), 0, 0, None)
        _hip.call("ieagan_conv_wgrad", d, tr, _hip.stream())
        outs.append(dw)
    ref = torch.nn.grad.conv2d_weight(nchw(x), (Cout, Cin, 3, 3), nchw(g), padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    close(outs[1], ref, 2e-3, "scalar-read wgrad")
    close(outs[0], ref, 2e-3, "tr-read wgrad")


@pytest.mark.parametrize("C,Hh,Ww", [(32, 20, 28), (16, 9, 13)])
def test_single_channel_convs(dev, C, Hh, Ww):
    import ops
    torch.manual_seed(4)
    N = 3
    # ---- D.input_conv: image -> C channels
    img = torch.randn(N, 1, Hh, Ww, device=dev, requires_grad=True)
    W = (torch.randn(C, 1, 3, 3, device=dev) / 3).requires_grad_(True)
    u = torch.randn(1, C, device=dev)
    bias = (0.1 * torch.randn(C, device=dev)).requires_grad_(True)
    Wsn, _, _ = sn_ref(W, u)
    ref = F.conv2d(img, Wsn, bias, 1, 1)
    go = r16(torch.randn_like(ref))
    gref = torch.autograd.grad((ref * go).sum(), [img, W, bias])
    rec, Wv, _, _ = make_rec(W.detach(), u, torch.ones(1, device=dev), kind=ops.KIND_C1_IN)
    img2 = img.detach().clone().requires_grad_(True)
    Wp = Wv.detach().requires_grad_(True)
    b2 = bias.detach().clone().requires_grad_(True)
    out = ops.InputConvFn.apply(img2, Wp, b2, rec)
    close(nchw(out), ref, 1e-2, "input conv")
    g = torch.autograd.grad((out.float() * nhwc(go).float()).sum(), [img2, Wp, b2])
    for n, a, b in zip(("img", "W", "bias"), g, gref):
        close(a, b, 2e-2, f"input conv grad {n}")
    # ---- G.output_layer: bn apply + relu + conv (C -> 1) + tanh
    h = r16(torch.randn(N, C, Hh, Ww, device=dev)).requires_grad_(True)
    W = (torch.randn(1, C, 3, 3, device=dev) / math.sqrt(9 * C)).requires_grad_(True)
    u = torch.randn(1, 1, device=dev)
    bias = (0.1 * torch.randn(1, device=dev)).requires_grad_(True)
    scale = (1 + 0.3 * torch.randn(C, device=dev)).requires_grad_(True)
    shift = (0.2 * torch.randn(C, device=dev)).requires_grad_(True)
    Wsn, _, _ = sn_ref(W, u)
    ref = torch.tanh(F.conv2d(F.relu(h * scale[None, :, None, None] + shift[None, :, None, None]), Wsn, bias, 1, 1))
    go = torch.randn_like(ref)
    gref = torch.autograd.grad((ref * go).sum(), [h, scale, shift, W, bias])
    rec, Wv, _, _ = make_rec(W.detach(), u, torch.ones(1, device=dev), kind=ops.KIND_C1_OUT)
    ha = nhwc(h.detach()).requires_grad_(True)
    sc2, sh2 = scale.detach().clone().requires_grad_(True), shift.detach().clone().requires_grad_(True)
    Wp, b2 = Wv.detach().requires_grad_(True), bias.detach().clone().requires_grad_(True)
    y = ops.OutputConvFn.apply(ha, sc2, sh2, Wp, b2, rec)
    close(y, ref, 1e-2, "output conv")          # MFMA form: transformed activations and weights are bf16 operands, as in every other conv
    g = torch.autograd.grad((y * go).sum(), [ha, sc2, sh2, Wp, b2])
    for n, a, b in zip(("h", "scale", "shift", "W", "bias"), g, gref):
        close(nchw(a) if n == "h" else a, b, 2e-2, f"output conv grad {n}")


def test_bn_finalize_matches_batch_norm(dev):
    """stats -> scale/shift equals F.batch_norm * (1+gain) + bias, with the running-stat update and
    the complete backward (through mean / var) folded into (dsum, dsumsq)."""
    import ops
    torch.manual_seed(5)
    N, C, Hh, Ww = 4, 32, 6, 10
    x = r16(torch.randn(N, C, Hh, Ww, device=dev) * 1.5 + 0.3).requires_grad_(True)
    gb = (0.3 * torch.randn(N, 2 * C, device=dev)).requires_grad_(True)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    ref = F.batch_norm(x, rm.clone(), rv.clone(), None, None, True, 0.1, 1e-5) * (1 + gb[:, :C, None, None]) + gb[:, C:, None, None]
    ref = F.relu(ref)
    go = torch.randn_like(ref)
    gref = torch.autograd.grad((ref * go).sum(), [x, gb])
    rm_ref, rv_ref = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    F.batch_norm(x.detach(), rm_ref, rv_ref, None, None, True, 0.1, 1e-5)
    # HIP: stats from the layout kernel, finalize, apply through the conv prologue (identity weights)
    import layers
    x2 = x.detach().clone().requires_grad_(True)
    gb2 = gb.detach().clone().requires_grad_(True)
    xa, st = ops.ToNHWCFn.apply(x2, True)
    bank = ops.GainBank(gb2, 1)
    s, t = ops.BNFinalizeFn.apply(st, gb2, bank, 0, C, C, rm, rv, N * Hh * Ww, 1e-5, 0.1, True)
    out = layers._affine_act(xa, s, t, relu=True)
    close(nchw(out), ref, 1.5e-2, "bn+relu out")
    close(rm, rm_ref, 1e-3, "running mean")
    close(rv, rv_ref, 1e-3, "running var")
    g = torch.autograd.grad((out.float() * nhwc(go).float()).sum(), [x2, gb2])
    close(g[0], gref[0], 3e-2, "bn dx")
    close(g[1], gref[1], 3e-2, "bn dgain/dbias")


@pytest.mark.parametrize("taps,C,Cout,Hh,Ww,N,res", [(9, 16, 16, 64, 96, 3, None),        # halo dgrad kernel (C = 16 variant)
                                                     (9, 16, 16, 128, 384, 6, None),      # conv3x3_ws dgrad kernel (>= 1024 tiles)
                                                     (9, 32, 32, 128, 384, 6, None),      # C = 32 dgrad at its production map (conv3x3_halo)
                                                     (9, 64, 64, 16, 48, 3, None),        # halo dgrad kernel (C = 64)
                                                     (1, 64, 16, 32, 64, 3, None),        # gather dgrad kernel
                                                     (1, 32, 64, 128, 384, 3, "same"),    # streaming dgrad kernel + shortcut gradient
                                                     (1, 64, 32, 128, 384, 3, "up")])     # ... with the shortcut at double resolution
def test_bn_backward_fused_into_dgrad(dev, taps, C, Cout, Hh, Ww, N, res):
    """ccbn -> ReLU -> conv: the BatchNorm-apply backward folded into the dgrad epilogue (per-image accumulators, no da tensor)
    against (a) the stand-alone prologue_bwd pass and (b) fp32 PyTorch autograd of F.batch_norm * (1 + gain) + bias."""
    import layers, ops
    torch.manual_seed(23)
    k = 3 if taps == 9 else 1
    x = r16(torch.randn(N, C, Hh, Ww, device=dev) * 1.3 + 0.2)
    gb = 0.3 * torch.randn(N, 2 * C, device=dev)
    W = torch.randn(Cout, C, k, k, device=dev) / math.sqrt(C * taps)
    u = torch.randn(1, Cout, device=dev)
    go = r16(torch.randn(N, Cout, Hh, Ww, device=dev))
    # shortcut that also reads x (GBlock: conv4's residual operand): its gradient is handed to this conv's backward through a ResLink
    sg = None
    if res == "same":
        sg = r16(torch.randn(N, C, Hh, Ww, device=dev))
    elif res == "up":
        sg = r16(torch.randn(N, C, 2 * Hh, 2 * Ww, device=dev))

    def hip(fused):
        ops.DEFAULTS.fuse_bn_backward = fused          # (seeds the bank make_rec builds below)
        try:
            rec, Wv, _, _ = make_rec(W.clone(), u.clone(), torch.ones(1, device=dev))
            x2, gb2 = x.clone().requires_grad_(True), gb.clone().requires_grad_(True)
            xa, st = ops.ToNHWCFn.apply(x2, True)
            bank = ops.GainBank(gb2, 1)
            link = ops.BNLink()
            s, t = ops.BNFinalizeFn.apply(st, gb2, bank, 0, C, C, torch.zeros(C, device=dev), torch.ones(C, device=dev), N * Hh * Ww, 1e-5,
                                          0.1, True, 1, link)
            s._bn_link = link
            rl = None
            if sg is not None:
                rl = ops.ResLink()
                rl.deposit(nhwc(sg), C, C, 1 if res == "up" else 0)
            out, _ = ops.conv(xa, Wv.detach(), None, rec, taps, scale=s, shift=t, relu=True, res_in=rl)
            gx, ggb = torch.autograd.grad((out.float() * nhwc(go).float()).sum(), [x2, gb2])
            return nchw(out), gx, ggb
        finally:
            ops.DEFAULTS.fuse_bn_backward = True

    o1, gx1, gg1 = hip(True)
    o0, gx0, gg0 = hip(False)
    close(o1, o0, 8e-3, "forward")          # (the batch statistics are float-atomic sums: run-to-run differences of an ulp)
    close(gx1, gx0, 8e-3, "dx fused vs separate")              # same arithmetic, one bf16 rounding fewer (da is never stored)
    close(gg1, gg0, 8e-3, "d gain/bias fused vs separate")
    xr, gbr = x.clone().requires_grad_(True), gb.clone().requires_grad_(True)
    a = F.relu(F.batch_norm(xr, None, None, None, None, True, 0.1, 1e-5) * (1 + gbr[:, :C, None, None]) + gbr[:, C:, None, None])
    a = a + (r16(a) - a).detach()
    Wsn, _, _ = sn_ref(W, u)
    ref = F.conv2d(a, r16(Wsn), None, 1, 1 if taps == 9 else 0)
    loss = (ref * go).sum()
    if sg is not None:
        loss = loss + ((F.interpolate(xr, scale_factor=2) if res == "up" else xr) * sg).sum()
    gxr, ggr = torch.autograd.grad(loss, [xr, gbr])
    close(o1, ref, 1.5e-2, "out")
    close(gx1, gxr, 3e-2, "dx vs fp32")
    close(gg1, ggr, 3e-2, "d gain/bias vs fp32")


def test_diffaug_and_cr(dev, golden_dir):
    import cr_diff_aug
    import diff_aug
    g = np.load(os.path.join(golden_dir, "op_diffaug.npz"))
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    draws = {k[2:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("d_")}
    y = diff_aug.DiffAugment(x, "color,translation,cutout", draws=draws)
    close(y, torch.from_numpy(g["y"]), 1e-5, "diffaug fwd (golden)")
    (gx,) = torch.autograd.grad(y, [x], torch.from_numpy(g["go"]).to(dev))
    close(gx, torch.from_numpy(g["gx"]), 1e-5, "diffaug bwd (golden)")
    for seed in (7, 8):
        g = np.load(os.path.join(golden_dir, f"op_crdiffaug_{seed}.npz"))
        draws = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("d_")}
        y = cr_diff_aug.CR_DiffAug(torch.from_numpy(g["x"]).to(dev), draws=draws)
        assert torch.equal(y.cpu(), torch.from_numpy(g["y"])), "cr_diffaug (golden)"


def test_adam_and_ema(dev, golden_dir):
    import _hip
    a = np.load(os.path.join(golden_dir, "op_adam.npz"))
    w = torch.from_numpy(a["w0"]).to(dev)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    hp = torch.tensor([5e-5, 0.0, 0.999, 1e-6, 0.0, 1.0, 0.0, 0.0], device=dev)   # device-side hyper block, step 0
    for step in range(1, 4):
        gr = torch.from_numpy(a["grads"][step - 1]).to(dev)
        _hip.call("ieagan_adam_step", w.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel(), hp.data_ptr(),
                  _hip.stream())
    assert float(hp[4]) == 3.0
    close(w, torch.from_numpy(a["w3"]), 2e-6, "adam (golden)")
    t, s = torch.randn(1000, device=dev), torch.randn(1000, device=dev)
    exp = t * 0.9 + s * 0.1
    dec = torch.tensor([0.9], device=dev)
    _hip.call("ieagan_ema_update", t.data_ptr(), s.data_ptr(), 1000, dec.data_ptr(), _hip.stream())
    close(t, exp, 1e-6, "ema")


@pytest.mark.parametrize("N,Lq,Lk,dqk,dv", [(2, 256, 64, 8, 32), (3, 192, 96, 32, 128), (2, 150, 70, 16, 64), (2, 3072, 768, 32, 128), (1, 100, 33, 24, 128)])
def test_nl_attention_forward_backward(dev, N, Lq, Lk, dqk, dv):
    """Streaming-softmax attention core vs softmax(QK^T)V in fp32 (incl. ragged Lq / Lk tails)."""
    import ops
    torch.manual_seed(11)
    q = r16(torch.randn(N, Lq, dqk, device=dev) * 0.7).requires_grad_(True)
    k = r16(torch.randn(N, Lk, dqk, device=dev) * 0.7).requires_grad_(True)
    v = r16(torch.randn(N, Lk, dv, device=dev)).requires_grad_(True)
    go = r16(torch.randn(N, Lq, dv, device=dev))
    ref = torch.softmax(q @ k.transpose(1, 2), -1) @ v
    gref = torch.autograd.grad((ref * go).sum(), [q, k, v])
    q2, k2, v2 = (t.detach().to(BF).requires_grad_(True) for t in (q, k, v))
    out = ops.NLAttentionFn.apply(q2, k2, v2)
    close(out, ref, 1.5e-2, "attention out")
    g = torch.autograd.grad((out.float() * go).sum(), [q2, k2, v2])
    for nme, a, b in zip(("dq", "dk", "dv"), g, gref):
        close(a, b, 3e-2, f"attention {nme}")


def test_loss_block_vs_golden(dev, golden_dir):
    """Fused loss kernel against the reference-generated values and gradients (loss.py)."""
    import loss as L
    import ops
    g = np.load(os.path.join(golden_dir, "op_losses.npz"))
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    e, p = t("e").requires_grad_(True), t("p").requires_grad_(True)
    crit = L.Conditional_Contrastive_loss(dev, 40, False)
    vals = {"contra": crit(e, p, None, None, 1.0, 0), "unif": L.unif_loss(e), "iea": L.IEA_loss(e, t("e2")),
            "hinge_real": L.loss_hinge_dis(t("dfk"), t("drl"))[0], "hinge_fake": L.loss_hinge_dis(t("dfk"), t("drl"))[1],
            "hinge_gen": L.loss_hinge_gen(t("dfk"))}
    for k, v in vals.items():
        ref = float(g[k])
        assert abs(float(v) - ref) <= 2e-5 * max(1.0, abs(ref)) + 1e-6, (k, float(v), ref)
    # one fused call for contra + 0.1 unif + iea: value and both gradients
    total, terms = ops.loss_block(e=e, p=p, er=t("e2"), w_contra=1.0, w_unif=0.1, w_iea=1.0)
    ge, gp = torch.autograd.grad(total, [e, p])
    close(ge, t("g_e"), 1e-4, "d total / d e")
    close(gp, t("g_p"), 1e-4, "d total / d p")
    # hinge gradients
    dfk, drl = t("dfk").requires_grad_(True), t("drl").requires_grad_(True)
    tot, _ = ops.loss_block(dfake=dfk, dreal=drl, w_hinge_real=1.0, w_hinge_fake=1.0)
    gf, gr = torch.autograd.grad(tot, [dfk, drl])
    rf, rr = torch.autograd.grad(torch.relu(1 + dfk).mean() + torch.relu(1 - drl).mean(), [dfk, drl])
    close(gf, rf, 1e-6, "hinge d fake")
    close(gr, rr, 1e-6, "hinge d real")


@pytest.mark.parametrize("E,heads", [(128, 2), (512, 4)])
def test_rrm_attention_core(dev, E, heads):
    import ops
    torch.manual_seed(13)
    B, S = 1, 40
    hd = E // heads
    qkv = torch.randn(B, S, 3 * E, device=dev, requires_grad=True)
    go = torch.randn(B, S, E, device=dev)
    q, k, v = qkv.reshape(B, S, heads, 3 * hd).permute(0, 2, 1, 3).chunk(3, dim=-1)
    ref = (torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(hd), -1) @ v).permute(0, 2, 1, 3).reshape(B, S, E)
    (gref,) = torch.autograd.grad(ref, [qkv], go)
    qkv2 = qkv.detach().clone().requires_grad_(True)
    out, att = ops.RRMAttentionFn.apply(qkv2, heads)
    close(out, ref, 1e-5, "rrm attention out")
    (g2,) = torch.autograd.grad(out, [qkv2], go)
    close(g2, gref, 1e-4, "rrm attention grad")
    assert att.shape == (B, heads, S, S) and torch.allclose(att.sum(-1), torch.ones(B, heads, S, device=dev), atol=1e-5)


def test_batched_ortho_vs_oracle(dev, golden_dir):
    """utils.ortho = one batched HIP call over the arena: every >=2-D weight gets 2s((WW^T)(.)(1-I))W added to its .grad
    (row form R<=K, column form R>K incl. a split reduce, K=9, blacklist, 1-D parameters untouched)."""
    import ieagan_oracle as O
    import utils
    torch.manual_seed(5)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            mk = lambda *s: torch.nn.Parameter(torch.randn(*s) * 0.3)
            self.conv = mk(48, 24, 3, 3)         # row form, K=216
            self.c1 = mk(16, 1, 3, 3)            # K=9 (ragged reduce)
            self.tall = mk(4500, 40)             # column form with 3 reduce splits
            self.lin = mk(130, 70)               # column form, ragged tiles
            self.emb = mk(40, 1024)
            self.skip = mk(32, 32)               # blacklisted
            self.vec = mk(77)                    # 1-D: not regularised

    net = Net().to(dev)
    g0 = {}
    for n, p in net.named_parameters():
        p.grad = torch.randn_like(p)
        g0[n] = p.grad.clone()
    utils.ortho(net, 1e-3, blacklist=[net.skip])
    for n, p in net.named_parameters():
        exp = g0[n].cpu()
        if p.dim() >= 2 and n != "skip":
            exp = exp + O.ortho_grad(p.detach().cpu(), 1e-3)
        close(p.grad, exp, 2e-5, f"ortho {n}")
    g = np.load(os.path.join(golden_dir, "op_ortho.npz"))
    lone = torch.nn.Linear(1, 1).to(dev)
    lone.weight = torch.nn.Parameter(torch.from_numpy(g["w"]).to(dev))
    for p in lone.parameters():
        p.grad = torch.zeros_like(p)
    utils.ortho(lone, 1e-4)
    close(lone.weight.grad, torch.from_numpy(g["g"]), 2e-5, "ortho (golden)")


def test_nonlocal_glue_maxpool_and_gamma_residual(dev):
    """2x2 max-pool (bf16 NHWC, first-maximum argmax like F.max_pool2d) and out = gamma*o + x with their backwards."""
    import ops
    torch.manual_seed(11)
    x = (torch.randn(3, 8, 12, 16, device=dev) * 2).round().div(2).to(BF).requires_grad_(True)     # many exact ties
    y = ops.MaxPool2Fn.apply(x)
    xr = x.detach().float().permute(0, 3, 1, 2).requires_grad_(True)
    yr = F.max_pool2d(xr, [2, 2])
    assert torch.equal(y.float().permute(0, 3, 1, 2), yr), "maxpool2 forward"
    go = torch.randn_like(yr)
    y.backward(go.permute(0, 2, 3, 1).to(BF))
    yr.backward(go.to(BF).float())
    assert torch.equal(x.grad.float().permute(0, 3, 1, 2), xr.grad), "maxpool2 backward (tie-breaking)"

    o = torch.randn(2, 6, 10, 24, device=dev).to(BF).requires_grad_(True)
    xx = torch.randn(2, 6, 10, 24, device=dev).to(BF).requires_grad_(True)
    gamma = torch.tensor(0.37, device=dev, requires_grad=True)
    out = ops.GammaResidualFn.apply(o, xx, gamma)
    close(out, 0.37 * o.float() + xx.float(), 8e-3, "gamma residual fwd")
    d = torch.randn_like(out)
    out.backward(d)
    close(o.grad, 0.37 * d.float(), 8e-3, "gamma residual d_o")
    assert torch.equal(xx.grad, d), "gamma residual dx"
    close(gamma.grad, (d.float() * o.detach().float()).sum(), 1e-4, "gamma residual dgamma")


def test_event_ingest_and_frechet_distance(dev, golden_dir):
    """uint8 event -> network input (one kernel) and the device-side Frechet distance vs the reference-generated vectors."""
    import ieagan_oracle as O
    import utils
    g = np.load(os.path.join(golden_dir, "op_ingest.npz"))
    ev, u = torch.from_numpy(g["ev"]), torch.from_numpy(g["u"])
    out = utils.ingest_event(ev, noise=u.reshape(5, 16, 16))            # host uint8 in, device fp32 out
    assert out.is_cuda and out.shape == (5, 1, 16, 16)
    close(out, torch.from_numpy(g["out"]), 2e-6, "ingest (golden)")
    big = (torch.rand(40, 250, 768) < 0.01).to(torch.uint8) * torch.randint(1, 256, (40, 250, 768), dtype=torch.uint8)
    x = utils.ingest_event(big.to(dev))
    assert x.shape == (40, 1, 256, 768) and float(x.min()) >= -1.0 and float(x.max()) <= 1.0 + 8e-3
    close(utils.ingest_event(big.to(dev), noise=False), O.ingest_event(big), 2e-6, "ingest 40x250x768 (oracle)")
    assert float((x[:, :, :3] + 1).abs().max()) <= 8e-3 + 1e-6            # padded rows: -1 + dequantisation noise only

    f = np.load(os.path.join(golden_dir, "op_frechet.npz"))
    for name, (p, q) in {"ab": ("a", "b"), "aa": ("a", "a"), "ac": ("a", "c")}.items():
        m1, s1 = utils.feature_statistics(torch.from_numpy(f[p]).to(dev))
        m2, s2 = utils.feature_statistics(torch.from_numpy(f[q]).to(dev))
        fd = utils.frechet_distance(m1, s1, m2, s2)
        ref = float(f["fd_" + name])
        assert abs(fd - ref) <= 1e-5 * max(1.0, abs(ref)), (name, fd, ref)


@pytest.mark.parametrize("taps,Cin,Cout,Hh,Ww,N,events", [(1, 512, 128, 8, 24, 40, 1),     # G b2/b3 conv1 at 8x24
                                                          (1, 512, 128, 4, 12, 40, 2),     # ... at 4x12 (48 pixels per image), two events
                                                          (1, 256, 64, 16, 48, 40, 1),     # 16x48
                                                          (9, 128, 128, 4, 12, 40, 1),     # 3x3 on the 4x12 map: 36 K steps
                                                          (9, 32, 16, 6, 10, 7, 1)])       # ragged: 420 pixels, half-empty n-tile
def test_split_k_gather_matches_plain_gather(dev, taps, Cin, Cout, Hh, Ww, N, events):
    """conv_gather's split-K form (tiny maps: the four waves of a block share one 32-pixel tile and a quarter of the K steps each)
    against the plain form (FORCE_GATHER) on the same operands: ccbn prologue, mask, statistics per event."""
    import _hip, ops
    torch.manual_seed(17)
    x = torch.randn(N, Hh, Ww, Cin, device=dev).to(BF)
    kpad = ops._kpad(taps * Cin)
    w = torch.zeros(Cout, kpad, device=dev)
    w[:, :taps * Cin] = torch.randn(Cout, taps * Cin, device=dev) / math.sqrt(taps * Cin)
    w = w.to(BF)
    bias = 0.1 * torch.randn(Cout, device=dev)
    sc = 1 + 0.2 * torch.randn(N, Cin, device=dev)
    sh = 0.2 * torch.randn(N, Cin, device=dev)
    mask = torch.randn(N, Hh, Ww, Cout, device=dev).to(BF)
    res = []
    npe = N // events if (N % events == 0 and ((N // events) * Hh * Ww) % 128 == 0) else 0
    for force in (0, _hip.CONV_FORCE_GATHER):
        out = torch.empty(N, Hh, Ww, Cout, device=dev, dtype=BF)
        st = ops.new_stats(Cout, dev, events if npe else 1)
        ops._conv_launch(x, Cin, Hh, Ww, 0, sc, sh, Cin, True, N, Hh, Ww, Cin, Cout, taps, kpad, w, bias, None, 0, 0, 0, None, 0, mask, out, st,
                         npe=npe, flags=force)
        res.append((out, st.sum(1)))
    close(res[0][0], res[1][0], 4e-3, "split-K vs plain gather out")          # fp32 partial sums added in a different order
    close(res[0][1], res[1][1], 2e-3, "split-K vs plain gather statistics")


@pytest.mark.parametrize("kind,cin,cout,flag,Hh,Ww,N", [
    ("g", 64, 32, True, 32, 64, 3),       # G b11: conv1 64->16 (ccbn prologue, effgrad, 2x2-sum shortcut gradient), conv4 16->32 (g_eff stored for the link)
    ("g", 64, 64, False, 32, 64, 3),      # G b10: same-resolution shortcut gradient, conv4 16->64
    ("g", 128, 64, True, 16, 32, 2),      # G b9: conv4 32->64 fused, conv1 128->32 stays on the separate launches
    ("d", 32, 64, True, 64, 64, 3),       # D s0.0: conv1 32->16 (+ 0.25 x expand of the pooled shortcut gradient), conv4 16->64 on the pooled source, conv_sc 32->32
    ("d0", 32, 64, True, 64, 64, 3),      # ... as the very first block (no pre-activation)
    ("d", 64, 64, False, 32, 64, 3),      # D s0.1: conv1 64->16, conv4 16->64, identity shortcut
    ("d", 64, 128, True, 64, 64, 2),      # D s1.0: conv1 64->32 fused; conv4 32->128 / conv_sc 64->64 stay on the separate launches
    ("d", 64, 64, False, 12, 32, 3),      # W % 64 != 0: 32-pixel wave tiles, the last block of an image holds 4 of its 8 tiles; 6 blocks (< 8 XCDs)
    ("d", 32, 64, True, 24, 64, 3),       # conv1: 9 blocks (9 % 8 == 1); conv4 / conv_sc on the pooled 12x32 source, half-filled last block
    ("g", 64, 32, True, 8, 32, 4),        # one block per image; conv1 sits exactly at the 1024-pixel threshold set below
])
def test_fused_1x1_backward_matches_separate_launches(dev, ref_cfg, kind, cin, cout, flag, Hh, Ww, N):
    """ieagan_conv1x1_bwd (effgrad + dgrad + prologue backward + wgrad + bias sums in one launch, shortcut gradients added in the
    kernel) against the separate launches on whole G / D blocks: output gradient, conditioning gradient and every parameter gradient
    (incl. the spectral-norm sigma term).  The separate launches themselves are checked against fp32 PyTorch and the reference
    vectors (test_conv_forward_backward, test_gblock_vs_golden, test_dblock_vs_golden)."""
    import functools
    import layers, model, ops
    from parity_util import O
    torch.manual_seed(3)

    def build():
        if kind == "g":
            lin = functools.partial(layers.SNLinear, bias=False, eps=ref_cfg["SN_eps"])
            blk = model.GBlock(cin, cout, functools.partial(layers.SNConv2d, kernel_size=3, padding=1, eps=ref_cfg["SN_eps"]),
                               functools.partial(layers.ccbn, which_linear=lin, input_size=256, eps=ref_cfg["BN_eps"]),
                               torch.nn.ReLU(inplace=True), functools.partial(F.interpolate, scale_factor=2) if flag else None)
        else:
            blk = model.DBlock(cin, cout, functools.partial(layers.SNConv2d, kernel_size=3, padding=1, eps=ref_cfg["SN_eps"]), True,
                               kind == "d", torch.nn.ReLU(inplace=True), torch.nn.AvgPool2d(2) if flag else None)
        spec = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
        blk.load_state_dict(O.synth_state(spec, 15))
        return blk.to(dev).train()

    x0 = torch.randn(N, cin, Hh, Ww, device=dev)
    yv0 = torch.randn(N, 256, device=dev)
    go = None
    res = {}
    keep = ops.DEFAULTS.fuse_1x1_backward, ops.DEFAULTS.fuse_1x1_min_pixels
    launches = {}
    try:
        for fused in (False, True):
            ops.DEFAULTS.fuse_1x1_backward, ops.DEFAULTS.fuse_1x1_min_pixels = fused, 1024      # (seed the bank of the block built below)
            blk = build()
            x = x0.clone().requires_grad_(True)
            yv = yv0.clone().requires_grad_(True)
            import _hip
            _hip.call("ieagan_prof_reset")
            _hip.prof_enable(1)
            y = blk(x, yv) if kind == "g" else blk(x)
            if go is None:
                go = torch.randn_like(y)
            params = dict(blk.named_parameters())
            names = sorted(params)
            leaves = [x] + ([yv] if kind == "g" else []) + [params[k] for k in names]
            grads = torch.autograd.grad(y, leaves, go)
            torch.cuda.synchronize()
            _hip.prof_enable(0)
            launches[fused] = {r["name"]: r["launches"] for r in _hip.prof_collect()}
            res[fused] = (y.detach(), dict(zip(["x"] + (["yv"] if kind == "g" else []) + names, grads)))
    finally:
        ops.DEFAULTS.fuse_1x1_backward, ops.DEFAULTS.fuse_1x1_min_pixels = keep
    assert launches[True].get("conv1x1_bwd", 0) >= 1 and "conv1x1_bwd" not in launches[False], launches
    assert launches[True].get("conv1x1_wgrad", 0) < launches[False].get("conv1x1_wgrad", 0), launches
    # (the two forwards differ only through the float-atomic order of the BatchNorm statistics: last-bit bf16 flips)
    assert float((res[True][0] - res[False][0]).norm() / res[False][0].norm()) <= 2e-3
    wnorm = max(float(v.norm()) for k, v in res[False][1].items() if k not in ("x", "yv"))
    for k, ref in res[False][1].items():
        got = res[True][1][k]
        if float(ref.norm()) < 2e-3 * wnorm:          # (a bias in front of a BatchNorm: zero up to rounding)
            assert float(got.norm()) < 4e-3 * wnorm, k
            continue
        err = float((got - ref).norm() / ref.norm())
        assert err <= 1e-2, (k, err)


@pytest.mark.parametrize("C,Hs,Ws,aff,rs,stats,N,events", [
    (16, 256, 768, False, 0, False, 2, 1),      # D s0.0 conv2 / conv3 (PROD_CASES row 1)
    (16, 256, 768, True, 0, True, 2, 1),        # G b11 conv3 (row 0)
    (16, 128, 384, True, 1, True, 2, 1),        # G b11 conv2: up-sampled source, 2x2 sum in the store phase (row 2)
    (32, 64, 192, True, 1, True, 3, 1),         # G b9 conv2: up-sampled source, C = 32 (G b9 conv3 -- C = 32, BatchNorm prologue + effgrad at the
                                                # same resolution -- is not offered by the kernel: register spills, see conv3x3_bwd.hip)
    (32, 128, 384, False, 0, False, 3, 1),      # D s1.0 conv2 / conv3 (row 4)
    (32, 64, 192, True, 1, True, 4, 2),         # G b9 conv2 with two events of two images (per-event effgrad rows, per-image BatchNorm rows)
    (16, 64, 64, False, 0, False, 40, 1),       # the 64x64 plumbing geometry: one tile row of two tiles per block
    (32, 72, 96, False, 0, False, 5, 1),        # tile counts that do not divide the persistent grid evenly
    (16, 16, 64, False, 0, False, 3, 1),        # 6 blocks of 2 tiles (fewer blocks than XCDs)
    (16, 8, 32, True, 1, True, 3, 1),           # up-sampled source, BatchNorm prologue + effgrad, 6 blocks
    (32, 8, 32, False, 0, False, 5, 1),         # one tile per image: a block never requests a next tile
    (32, 8, 32, True, 1, True, 4, 2),           # two events, 8 blocks
])
def test_fused_3x3_backward_matches_separate_launches(dev, C, Hs, Ws, aff, rs, stats, N, events):
    """ieagan_conv3x3_bwd (effgrad on load + dgrad with the prologue backward in its store phase + wgrad + bias sums in one launch) against
    the separate launches it replaces, which test_conv_forward_backward pins against fp32 autograd (with the fused path ON those cases
    run through this kernel too): dx, dW (incl. the spectral-norm sigma term), dbias, d scale / d shift."""
    import _hip
    import ops
    torch.manual_seed(5)
    x0 = nhwc(torch.randn(N, C, Hs, Ws, device=dev))
    W0 = torch.randn(C, C, 3, 3, device=dev) / math.sqrt(9 * C)
    u = torch.randn(1, C, device=dev)
    b0 = 0.1 * torch.randn(C, device=dev)
    sc0 = (1 + 0.3 * torch.randn(N, C, device=dev)) if aff else None
    sh0 = 0.2 * torch.randn(N, C, device=dev) if aff else None
    Hc, Wc = (2 * Hs, 2 * Ws) if rs == 1 else (Hs, Ws)
    go = nhwc(torch.randn(N, C, Hc, Wc, device=dev))
    dsum = 0.05 * torch.randn(events, 1, 2, C, device=dev)
    res, launches = {}, {}
    keep = ops.DEFAULTS.fuse_3x3_backward, ops.DEFAULTS.fuse_3x3_min_pixels
    try:
        for fused in (False, True):
            ops.DEFAULTS.fuse_3x3_backward, ops.DEFAULTS.fuse_3x3_min_pixels = fused, 1024      # (seed the bank make_rec builds below)
            rec, Wv, uv, svv = make_rec(W0.clone(), u.clone(), torch.ones(1, device=dev))
            Wp = Wv.detach().requires_grad_(True)
            xa = x0.clone().requires_grad_(True)
            b2 = b0.clone().requires_grad_(True)
            sc2 = sc0.clone().requires_grad_(True) if aff else None
            sh2 = sh0.clone().requires_grad_(True) if aff else None
            _hip.call("ieagan_prof_reset")
            _hip.prof_enable(1)
            out, st = ops.conv(xa, Wp, b2, rec, 9, scale=sc2, shift=sh2, relu=True, rs=rs, want_stats=stats, events=events)
            loss = (out.float() * go.float()).sum()
            if stats:
                loss = loss + (st * dsum).sum()
            leaves = [t for t in (xa, Wp, b2, sc2, sh2) if t is not None]
            grads = torch.autograd.grad(loss, leaves)
            torch.cuda.synchronize()
            _hip.prof_enable(0)
            launches[fused] = {r["name"]: r["launches"] for r in _hip.prof_collect()}
            res[fused] = dict(zip([n for n, t in zip(("x", "W", "bias", "scale", "shift"), (xa, Wp, b2, sc2, sh2)) if t is not None], grads))
    finally:
        ops.DEFAULTS.fuse_3x3_backward, ops.DEFAULTS.fuse_3x3_min_pixels = keep
    assert launches[True].get("conv3x3_bwd", 0) == 1 and "conv3x3_bwd" not in launches[False], launches
    assert "conv3x3_wgrad" not in launches[True] and "effgrad" not in launches[True] and "prologue_bwd" not in launches[True], launches
    for k, ref in res[False].items():
        got = res[True][k]
        err = float((got.float() - ref.float()).norm() / ref.float().norm())
        # dx: same MFMA K order as the dgrad launch -> bit-equal for the bare-ReLU prologue at the same resolution; with the BatchNorm
        # prologue (no BNLink here) or an up-sampled source the separate path goes through prologue_bwd, which reads the conv-input gradient
        # back ROUNDED TO bf16 before masking / scaling / the 2x2 sum, while the fused kernel applies them to the fp32 accumulators (one
        # rounding less: 13-20 % of the elements differ by one bf16 ulp, 2.6e-3 .. 2.8e-3 in L2); weight-side sums: fp32 in another order
        tol = (1e-5 if (not aff and rs == 0) else 4e-3) if k == "x" else 4e-3 if k in ("scale", "shift") else 2e-3
        assert err <= tol, (k, err)


@pytest.mark.parametrize("N,Hh,Ww,C,aff", [(24, 64, 192, 64, True), (84, 32, 96, 64, False), (6, 32, 96, 64, False), (4, 16, 48, 128, True),
                                            (3, 8, 24, 128, False)])
def test_fp8_conv_dgrad_vs_fp32(dev, N, Hh, Ww, C, aff):
    """conv_dtype='fp8' dgrad of the C = 64 / 128 3x3 layers (plain prologue; ReLU-mask epilogue for the D layers, BatchNorm-backward
    epilogue for the G layers) through ops.conv's autograd: gradient w.r.t. the conv input against fp32 autograd of the same
    composite -- rel-L2 <= 5e-2 (e4m3 operands: ~3 % per product), the bf16 path <= 1.5e-2 on the same operands."""
    import _hip, ops
    torch.manual_seed(41)
    x = r16(torch.randn(N, C, Hh, Ww, device=dev)).requires_grad_(True)
    W = (torch.randn(C, C, 3, 3, device=dev) / math.sqrt(9 * C)).requires_grad_(True)
    u = torch.randn(1, C, device=dev)
    bias = (0.1 * torch.randn(C, device=dev)).requires_grad_(True)
    scale = (1 + 0.3 * torch.randn(N, C, device=dev)) if aff else None
    shift = (0.2 * torch.randn(N, C, device=dev)) if aff else None
    ref = conv_reference(x, W, u, bias, scale, shift, True, 0, 9, None, 0, 0, None)
    go = r16(torch.randn_like(ref))
    (gx_ref,) = torch.autograd.grad((ref * go).sum(), [x])
    errs = {}
    for name, flags in (("bf16", 0), ("fp8", _hip.CONV_FP8)):
        rec, Wv, uv, svv = make_rec(W.detach(), u, torch.ones(1, device=dev))
        xa = nhwc(x.detach()).requires_grad_(True)
        sc2 = scale.clone().requires_grad_(True) if aff else None
        sh2 = shift.clone().requires_grad_(True) if aff else None
        if aff:
            sc2._bn_link = ops.BNLink()              # dgrad with the BatchNorm-backward epilogue (per-image accumulators)
        out, _ = ops.conv(xa, Wv.detach().requires_grad_(True), bias.detach().clone().requires_grad_(True), rec, 9, scale=sc2, shift=sh2,
                          relu=True, flags=flags)
        (gx,) = torch.autograd.grad((out.float() * nhwc(go).float()).sum(), [xa])
        errs[name] = float((nchw(gx) - gx_ref).norm() / gx_ref.norm())
    print(errs)
    assert errs["bf16"] <= 1.5e-2 and errs["fp8"] <= 5e-2, errs
    if C == 64 and N * ((Hh + 7) // 8) * ((Ww + 31) // 32) < 1000:
        assert errs["fp8"] == errs["bf16"], errs        # below 1000 tile-blocks C = 64 keeps bf16 operands (lds_fp8_launch): the flag is inert
    else:
        assert errs["fp8"] > errs["bf16"], errs
