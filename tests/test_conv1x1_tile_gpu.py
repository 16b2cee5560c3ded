"""conv1x1_tile (operands staged by unconditional loads on clamped addresses, the next K chunk in flight during the MFMAs, the
epilogue's operands requested before the last chunk's MFMAs) against conv_gather on identical operands: outputs bit for bit (the k order
of every accumulation is the same), per-event statistics to the 1e-4 of test_streaming_1x1_agrees_with_gather, whose harness
(ops._conv_launch, flags=CONV_FORCE_GATHER for the reference) the cases reuse.  The shapes are the smallest that reach each path of the
kernel AND are dispatched to it (``takes_tile`` mirrors the launcher's conditions and is asserted per case)."""
import math

import pytest
import torch

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


def takes_tile(Cin, Cout, Hh, Ww, N, rs, aff):
    """conv1x1_tile_launch's conditions (and, for a same-resolution source, conv1x1_stream_launch declining first)."""
    HW, M = Hh * Ww, N * Hh * Ww
    if rs == 0 and Cin <= 128 and not ((Cin == 128 and Cout >= 128) or (Cin == 64 and Cout >= 256)) and HW % 128 == 0 and M // 128 >= 480:
        return False                                            # conv1x1_stream takes it
    if Cout % 32 or Cin % 8 or not (Cin <= 32 or Cin == 64 or Cin % 128 == 0):
        return False
    if M < (1024 if rs == 2 else 4096) or (M < 16384 and Cin > 256):
        return False
    return not (aff and (HW % 128 or Cin > 512))


def run_pair(dev, Cin, Cout, Hh, Ww, N, rs=0, aff=False, relu=False, bias=True, res=None, mask=False, events=1, bnb=False, seed=5):
    """The same launch through conv1x1_tile and through conv_gather: [(out, folded statistics)] * 2."""
    import _hip, ops
    assert takes_tile(Cin, Cout, Hh, Ww, N, rs, aff), "this case would not reach conv1x1_tile"
    torch.manual_seed(seed)
    Hs, Ws = (2 * Hh, 2 * Ww) if rs == 2 else (Hh, Ww)
    x = torch.randn(N, Hs, Ws, Cin, device=dev).to(BF)
    kpad = ops._kpad(Cin)
    w = torch.zeros(Cout, kpad, device=dev)
    w[:, :Cin] = torch.randn(Cout, Cin, device=dev) / math.sqrt(Cin)
    w = w.to(BF)
    b = 0.1 * torch.randn(Cout, device=dev) if (bias and not bnb) else None
    sc = (1 + 0.3 * torch.randn(N, Cin, device=dev)) if aff else None
    sh = (0.2 * torch.randn(N, Cin, device=dev)) if aff else None
    mk = (torch.randn(N, Hh, Ww, Cout, device=dev) * 1.3 + 0.2).to(BF) if (mask or bnb) else None      # ReLU mask / BatchNorm input
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
    bsc = (1 + 0.3 * torch.randn(N, Cout, device=dev)) if bnb else None
    bsh = (0.2 * torch.randn(N, Cout, device=dev)) if bnb else None
    outs = []
    for force in (0, _hip.CONV_FORCE_GATHER):
        out = torch.full((N, Hh, Ww, Cout), float("nan"), device=dev, dtype=BF)
        if bnb:           # per-image accumulators (n_per_event = 1), sized by the library for the launch it plans
            st = ops._conv_launch(x, Cin, Hs, Ws, rs, None, None, 0, False, N, Hh, Ww, Cin, Cout, 1, kpad, w, None, None, 0, 0, 0,
                                  None, 0, mk, out, True, npe=1, flags=force, bnb=(bsc, bsh, Cout, True))
        else:
            st = ops.new_stats(Cout, dev, events)
            ops._conv_launch(x, Cin, Hs, Ws, rs, sc, sh, Cin if aff else 0, relu, N, Hh, Ww, Cin, Cout, 1, kpad, w, b, ra, Cra, Ca, ra_rs,
                             rb, Crb, mk, out, st, npe=N // events, flags=force)
        outs.append((out, st.sum(1)))
    return outs


def check(outs, events=1):
    (o1, s1), (o0, s0) = outs
    assert torch.isfinite(o0.float()).all() and torch.isfinite(o1.float()).all()        # every pixel below M was stored (the buffers start as NaN)
    assert torch.equal(o1, o0), float((o1.float() - o0.float()).abs().max())
    close(s1, s0, 1e-4, "tile vs gather statistics")          # rows past M counted -> the sums would differ
    if events > 1:
        assert not torch.allclose(s1[0], s1[1])                # the events really are separate accumulators


# 8x24 with N = 23: M = 4416 = 34.5 blocks -- the last block's rows past M are clamped on load, neither stored nor counted.
# Cin > 256 reaches this kernel from M = 16384 up: N = 87 gives M = 16704 = 130.5 blocks.
@pytest.mark.parametrize("Cin,N", [(16, 23), (32, 23), (64, 23), (128, 23), (256, 23), (384, 87), (512, 87)])
def test_chunk_counts_with_a_tail_block(dev, Cin, N):
    """One chunk of 32 (Cin = 16: half of the only k-step is padding; 32), of 64, of 128; two, three (the odd count for a chunk held in
    flight) and four chunks of 128."""
    check(run_pair(dev, Cin, 64, 8, 24, N))


@pytest.mark.parametrize("Cout", [32, 96, 256])
def test_output_columns(dev, Cout):
    """Cout = 32 (two n-tiles per block), 96 (three such columns, Cout % 64 != 0), 256 (four columns of four n-tiles); 64 is in every other
    case.  Two K chunks, mask and same-resolution residual so that every column's epilogue operands are addressed."""
    check(run_pair(dev, 256, Cout, 8, 24, 23, mask=True, res="same"))


@pytest.mark.parametrize("Cin,relu", [(128, True), (256, False), (64, True)])
def test_batchnorm_prologue_two_events(dev, Cin, relu):
    """N = 6 at 16x48: six blocks per image, three images per event; the per-image table is applied when the held chunk goes to LDS."""
    check(run_pair(dev, Cin, 64, 16, 48, 6, aff=True, relu=relu, events=2), events=2)


@pytest.mark.parametrize("Cin,res", [(32, None), (64, "same"), (128, None), (256, "same")])
def test_pooled_source_with_relu(dev, Cin, res):
    """N = 7, output 8x24 from a 16x48 source: M = 1344 = 10.5 blocks.  One batch of loads per chunk (Cin <= 64), two batches (128), two
    chunks (256); the residual of the DBlock's shortcut."""
    check(run_pair(dev, Cin, 64, 8, 24, 7, rs=2, relu=True, res=res))


@pytest.mark.parametrize("Cin,relu", [(64, True), (128, True), (128, False)])
def test_pooled_source_with_batchnorm_table(dev, Cin, relu):
    """Output 16x48 (six blocks per image: one table per block) from a 32x96 source, two events of one image."""
    check(run_pair(dev, Cin, 64, 16, 48, 2, rs=2, aff=True, relu=relu, events=2), events=2)


@pytest.mark.parametrize("bias,res,mask,Cout", [
    (False, None, False, 64), (True, None, True, 64), (True, "same", False, 64), (True, "up", False, 64), (True, "pool", False, 64),
    (True, "cat", False, 64), (True, "up", True, 32), (False, "cat", True, 256),
])
def test_epilogue_operands(dev, bias, res, mask, Cout):
    """No bias / bias, ReLU mask, residual at the same, half (x2 upsample) and double (2x2 average) resolution, the `cat` pair (A on the
    lower half of the channels, B on the upper), on two K chunks with a tail block."""
    check(run_pair(dev, 256, Cout, 8, 24, 23, bias=bias, res=res, mask=mask))


@pytest.mark.parametrize("Cin", [64, 256])
def test_batchnorm_backward_epilogue(dev, Cin):
    """The BatchNorm-backward form (bnb = (scale, shift, nstride, relu); `mask` is the BatchNorm input, per-image accumulators)."""
    check(run_pair(dev, Cin, 64, 16, 48, 6, bnb=True))
