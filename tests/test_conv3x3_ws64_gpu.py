"""conv3x3_ws64 (wave-specialised 3x3 kernel, Cin = Cout = 64) against conv3x3_lds on identical operands, through the C entry point.

Every case launches the layer twice: with CONV_FORCE_WS64 (the new kernel, also below its tile-count threshold) and with CONV_NO_WS64
(conv3x3_lds, the path before this kernel existed).  Both kernels accumulate every output element over the same k-steps in the same
order, so

  * outputs must agree bit for bit;
  * folded statistics (sum and sum of squares per channel and event) must agree to 1e-5 relative (norm of the difference over the norm
    of the reference vector, the form and the bound of the reproducibility test for stream-form differences): the tile geometry
    changes the order in which the block partials are added;
  * BatchNorm-backward accumulators are compared in the same way after ieagan_bn_finalize_bwd (d gain, d bias, d statistics).

The shapes are the smallest that reach each hazard.  A persistent block walks at least four 8x16-pixel tiles when its event has them, so
e.g. 27 tiles make blocks of 4, 4, ..., 3 tiles, 9 tiles make 4 + 4 + 1.  The launcher sizes the grid to the tiles (no block is ever
empty, the kernel's early exit is a guard); every case here has fewer tiles than the 256 CUs.
One more case checks forward and dgrad of the new kernel against fp64 conv2d autograd with the tolerances test_conv_forward_backward
applies to its C = 64 rows.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
C = 64


@pytest.fixture(scope="module")
def dev():
    import _hip
    _hip.require_gpu()
    _hip.lib()
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def operands(dev, N, Hs, Ws, seed):
    import ops
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, Hs, Ws, C, generator=g).to(dev).to(BF)
    kpad = ops._kpad(9 * C)
    w = (torch.randn(C, kpad, generator=g) / math.sqrt(9 * C)).to(dev).to(BF)
    bias = (0.1 * torch.randn(C, generator=g)).to(dev)
    sc = (1 + 0.3 * torch.randn(N, C, generator=g)).to(dev)
    sh = (0.2 * torch.randn(N, C, generator=g)).to(dev)
    return x, w, kpad, bias, sc, sh


def both(dev, N, Hc, Wc, x, Hs, Ws, rs, sc, sh, relu, w, kpad, bias, mask, stats, npe, bnb=None):
    """The same launch through conv3x3_ws64 and through conv3x3_lds: [(out, folded statistics or None, raw statistics)] * 2."""
    import _hip, ops
    res = []
    for flags in (_hip.CONV_FORCE_WS64, _hip.CONV_NO_WS64):
        out = torch.full((N, Hc, Wc, C), float("nan"), device=dev, dtype=BF)
        st = ops._conv_launch(x, C, Hs, Ws, rs, sc, sh, C if sc is not None else 0, relu, N, Hc, Wc, C, C, 9, kpad, w, bias,
                              None, 0, 0, 0, None, 0, mask, out, True if stats else None, npe=npe, flags=flags, bnb=bnb)
        res.append((out, st.sum(1) if stats else None, st))
    return res


def check(res, what, events=1):
    (o1, s1, _), (o0, s0, _) = res
    assert torch.isfinite(o0.float()).all() and torch.isfinite(o1.float()).all(), what
    nd = int((o1 != o0).sum())
    print(f"{what}: differing outputs {nd}")
    assert torch.equal(o1, o0), (what, nd, float((o1.float() - o0.float()).abs().max()))
    if s1 is not None:
        for e in range(s1.shape[0]):
            for k in range(2):
                r = rel(s1[e, k], s0[e, k])
                print(f"{what}: event {e} {'sumsq' if k else 'sum'} rel {r:.2e}")
                assert r <= 1e-5, (what, e, k, r)
        if events > 1:
            assert not torch.allclose(s1[0], s1[1])            # the events really are separate accumulators


CASES = {
    # name: (N, H, W, aff, relu, rs, mask, stats, events)
    "c1_full_relu_16x32": (2, 16, 32, False, True, 0, False, False, 1),        # 8 tiles: blocks of 4 + 4, both buffer parities
    "c2_ccbn_stats_24x48": (3, 24, 48, True, True, 0, False, True, 1),         # 27 tiles, 9 per image: image changes inside a block's run
    "c3_two_events_16x32": (4, 16, 32, False, True, 0, False, True, 2),        # tile ranges stop at the event boundary
    "c4_partial_masked_12x40": (2, 12, 40, False, False, 0, True, False, 1),   # partial tiles in both directions, ReLU-mask dgrad
    "c5_upsampled_ccbn_16x32": (2, 16, 32, True, True, 1, False, True, 1),     # 8x16 source, clamped up-sampled halo
    "c7_one_tile_blocks_24x48": (1, 24, 48, False, True, 0, False, True, 1),   # 9 tiles: 4 + 4 + 1, fewer tiles than CUs
    "c8_affine_no_relu_20x24": (2, 20, 24, True, False, 0, False, True, 1),    # (AFF, !RELU) variant, partial tiles
    "c9_plain_upsampled_16x32": (2, 16, 32, False, False, 1, False, False, 1), # (!AFF, !RELU) at RS = 1
}


@pytest.mark.parametrize("name", list(CASES))
def test_ws64_agrees_with_lds_bit_for_bit(dev, name):
    N, Hc, Wc, aff, relu, rs, mask, stats, events = CASES[name]
    Hs, Ws = (Hc // 2, Wc // 2) if rs == 1 else (Hc, Wc)
    x, w, kpad, bias, sc, sh = operands(dev, N, Hs, Ws, 40 + len(name))
    mk = torch.randn(N, Hc, Wc, C, device=dev).to(BF) if mask else None
    res = both(dev, N, Hc, Wc, x, Hs, Ws, rs, sc if aff else None, sh if aff else None, relu, w, kpad, bias, mk, stats, N // events)
    check(res, name, events)


def test_ws64_bnb_dgrad_agrees_with_lds(dev):
    """Case 6: N = 2, 16x48, the BatchNorm-backward dgrad form (per-image accumulators, n_per_event = 1): outputs bit for bit, the
    accumulators after ieagan_bn_finalize_bwd to 1e-5 relative."""
    import _hip as H
    N, Hc, Wc = 2, 16, 48
    g, w, kpad, _, sc, sh = operands(dev, N, Hc, Wc, 77)
    xin = (torch.randn(N, Hc, Wc, C, device=dev) * 1.3 + 0.2).to(BF)          # the BatchNorm input (passed as `mask`)
    res = both(dev, N, Hc, Wc, g, Hc, Wc, 0, None, None, False, w, kpad, None, xin, True, 1, bnb=(sc, sh, C, True))
    (o1, _, a1), (o0, _, a0) = res
    assert torch.equal(o1, o0), float((o1.float() - o0.float()).abs().max())
    gb = 0.3 * torch.randn(N, 2 * C, device=dev)
    mr = torch.stack([0.1 * torch.randn(C, device=dev), 1 + 0.1 * torch.rand(C, device=dev)]).unsqueeze(0).contiguous()
    fin = []
    for acc in (a1, a0):
        dgb = torch.zeros(N, 2 * C, device=dev)
        dstat = torch.zeros(1, 2, C, device=dev)
        H.call("ieagan_bn_finalize_bwd", acc.data_ptr(), acc.data_ptr(), gb.data_ptr(), 2 * C, 1, mr.data_ptr(), float(N * Hc * Wc), 1,
               dgb.data_ptr(), dgb.data_ptr() + 4 * C, 2 * C, dstat.data_ptr(), N, C, 1, int(acc.shape[1]), None, H.stream())
        fin.append((dgb, dstat))
    for k, what in enumerate(("d gain / d bias", "d statistics")):
        r = rel(fin[0][k], fin[1][k])
        print(f"bnb {what}: rel {r:.2e}")
        assert float(fin[1][k].abs().max()) > 0
        assert r <= 1e-5, (what, r)


def test_ws64_forward_and_dgrad_vs_fp64_autograd(dev):
    """ReLU -> conv3x3 forward and its masked dgrad (flipped, transposed pack) through the new kernel against fp64 conv2d autograd on the
    same bf16-rounded operands: 1.5e-2 * max|ref| for the output, 3e-2 * max|ref| for the input gradient (test_conv_forward_backward)."""
    import _hip, ops
    N, Hc, Wc = 2, 24, 40
    torch.manual_seed(5)
    x = torch.randn(N, C, Hc, Wc, device=dev).to(BF)
    W = (torch.randn(C, C, 3, 3, device=dev) / math.sqrt(9 * C)).to(BF)
    bias = 0.1 * torch.randn(C, device=dev)
    go = torch.randn(N, C, Hc, Wc, device=dev).to(BF)
    xr = x.double().requires_grad_(True)
    ref = F.conv2d(F.relu(xr), W.double(), bias.double(), 1, 1)
    gref, = torch.autograd.grad((ref * go.double()).sum(), xr)
    kpad = ops._kpad(9 * C)
    wf = W.permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous()                          # [cout][tap][cin]
    wb = W.flip(2, 3).permute(1, 2, 3, 0).reshape(C, 9 * C).contiguous()               # [cin][flipped tap][cout]
    xa, ga = x.permute(0, 2, 3, 1).contiguous(), go.permute(0, 2, 3, 1).contiguous()
    out = torch.empty(N, Hc, Wc, C, device=dev, dtype=BF)
    dx = torch.empty(N, Hc, Wc, C, device=dev, dtype=BF)
    fl = _hip.CONV_FORCE_WS64
    ops._conv_launch(xa, C, Hc, Wc, 0, None, None, 0, True, N, Hc, Wc, C, C, 9, kpad, wf, bias, None, 0, 0, 0, None, 0, None, out, None, flags=fl)
    ops._conv_launch(ga, C, Hc, Wc, 0, None, None, 0, False, N, Hc, Wc, C, C, 9, kpad, wb, None, None, 0, 0, 0, None, 0, xa, dx, None, flags=fl)
    for what, got, want, tol in (("out", out, ref.detach(), 1.5e-2), ("dx", dx, gref, 3e-2)):
        got = got.double().permute(0, 3, 1, 2)
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"{what}: max|diff| {err:.3e}, max|ref| {scale:.3e}")
        assert math.isfinite(err) and err <= tol * scale, (what, err, scale)
