"""Operator-level tests of the small fp32 kernels around the Relational Reasoning Module and the two network heads (csrc/rrm_fused.hip,
the attention core and the D-head pooling of csrc/small_ops.hip, the layout / statistics / residual glue of csrc/bn_elem.hip) against
the plain fp64 restatements of tests/small_ops_reference.py (pinned against fp64 autograd in tests/test_small_ops_reference.py), at
the smallest shapes that reach every path of the kernels: clamped loads and their selects, remainder batches, ragged tiles, the
split reduction with float atomics, the staging tail, the K limit, null-pointer options.

The C ABI is called directly (``_hip.call``), so that the options are driven independently of ops.py; a few calls through ops.py pin
that its split decision and zeroing agree with the C side.

Output hygiene of EVERY call: each output is a slice of a larger buffer with 256 sentinel floats (1 KiB) on either side; the slice is
pre-filled with NaN -- or, where the contract says the kernel ADDS into it, with known non-zero values (zeros for the split-mode dX,
which the contract wants zeroed) -- and after the call the sentinels must be bit-identical and no NaN may be left inside: an unwritten
element or an out-of-bounds store fails the test.

Tolerances.  fp32 kernels: max|kernel - fp64| / max|fp64| per output over ALL elements, <= 2e-5 for forward outputs and <= 1e-4 for
gradients (the suite's fp32 figures, tests/test_golden_gpu.py).  Next to each figure the test prints the same measure for the
reference evaluated in fp32 on the CPU (an ordered fp32 chain: ~1e-7 ... 5e-7), so the bounds leave the kernels' summation orders
and atomics 40x / 200x while one dropped k-element (~1e-3) fails.  Glue kernels: inputs are multiples of 1/8 in [-8, 8], every sum
has one right answer, ``torch.equal``."""
import functools

import pytest
import torch

import small_ops_reference as R
from gpu_outputs import BF16, BWD_TOL, DEV, FWD_TOL, Out, _H, _call, _check, _d, _dev

pytestmark = pytest.mark.gpu


# =====================================================================================================
# slin_fwd
# =====================================================================================================
@pytest.mark.parametrize("case", R.SLIN_FWD_CASES, ids=str)
def test_slin_fwd(case):
    M, K, N, ln = case[:4]
    i = R.slin_fwd_inputs(*case)
    ref64 = R.linear(_d(i["x"]), _d(i["w"]), _d(i["b"]), _d(i["res"]), _d(i["ln_g"]), _d(i["ln_b"]), i["relu"], i["eps"])
    ref32 = R.linear(i["x"], i["w"], i["b"], i["res"], i["ln_g"], i["ln_b"], i["relu"], i["eps"])
    x, w, b, res, lg, lb = (_dev(i[k]) for k in ("x", "w", "b", "res", "ln_g", "ln_b"))
    y, xhat, rstd = Out((M, N)), Out((M, K)) if ln else None, Out((M,)) if ln else None
    outs = [y] + ([xhat, rstd] if ln else [])
    got = _call("ieagan_slin_fwd", outs, x, w, b, res, y, lg, lb, xhat, rstd, M, K, N, int(i["relu"]), float(i["eps"]))
    for name, g, r64, r32 in zip(("y", "xhat", "rstd"), got, ref64, ref32):
        _check("slin_fwd", name, case, g, r64, r32, FWD_TOL)
    if ln and M >= 2:
        assert torch.equal(got[1][1], torch.zeros(K))              # the constant row: variance 0, xhat exactly 0


def test_slin_fwd_limits():
    """K is a multiple of 4 in [4, 2048] (the largest K runs in test_slin_fwd, with and without the prologue); the LayerNorm prologue needs
    all four of its pointers."""
    H = _H()
    t = torch.zeros(8 * 2052, device=DEV)
    for K in (2052, 6, 0):
        with pytest.raises(RuntimeError, match="slin_fwd: M=2 K="):
            H.call("ieagan_slin_fwd", t.data_ptr(), t.data_ptr(), None, None, t.data_ptr(), None, None, None, None, 2, K, 2, 0, 1e-5, H.stream())
    with pytest.raises(RuntimeError, match="LayerNorm prologue needs"):
        H.call("ieagan_slin_fwd", t.data_ptr(), t.data_ptr(), None, None, t.data_ptr(), t.data_ptr(), t.data_ptr(), None, None, 2, 8, 2, 0, 1e-5,
               H.stream())
    with pytest.raises(RuntimeError, match="null pointer"):
        H.call("ieagan_slin_fwd", t.data_ptr(), None, None, None, t.data_ptr(), None, None, None, None, 2, 8, 2, 0, 1e-5, H.stream())


# =====================================================================================================
# slin_bwd
# =====================================================================================================
def _slin_bwd_refs(i):
    a = ("dy", "w", "xn", "xhat", "ln_g", "ln_b", "ymask")
    return R.linear_bwd(*[_d(i[k]) for k in a]), R.linear_bwd(*[i[k] for k in a])


@pytest.mark.parametrize("case", R.SLIN_BWD_CASES, ids=str)
def test_slin_bwd(case):
    M, K, N, ln, mask, which, dx_zeroed = case
    i = R.slin_bwd_inputs(M, K, N, ln, mask)
    ref64, ref32 = _slin_bwd_refs(i)
    dy, w, xn, xhat, lg, lb, ym = (_dev(i[k]) for k in ("dy", "w", "xn", "xhat", "ln_g", "ln_b", "ymask"))
    if which == "b" and ln:
        xhat = lg = lb = None                      # the bias gradient alone needs no GEMM input at all
    dx = Out((M, K), fill=0.0 if dx_zeroed else None) if "x" in which else None
    dw = Out((N, K)) if "w" in which else None
    db = Out((N,)) if "b" in which else None
    outs = [o for o in (dx, dw, db) if o is not None]
    got = _call("ieagan_slin_bwd", outs, dy, ym, xn, xhat, lg, lb, w, dx, dw, db, M, K, N, dx_zeroed)
    names = [n for n, o in zip(("dx", "dw", "db"), (dx, dw, db)) if o is not None]
    for name, g in zip(names, got):
        k = ("dx", "dw", "db").index(name)
        _check("slin_bwd", name, case, g, ref64[k], ref32[k], BWD_TOL)


def test_slin_bwd_limits():
    H = _H()
    t = torch.zeros(64, device=DEV)
    with pytest.raises(RuntimeError, match="nothing to compute"):
        H.call("ieagan_slin_bwd", t.data_ptr(), None, t.data_ptr(), None, None, None, t.data_ptr(), None, None, None, 2, 4, 2, 0, H.stream())
    with pytest.raises(RuntimeError, match="needs the GEMM input"):
        H.call("ieagan_slin_bwd", t.data_ptr(), None, None, None, None, None, t.data_ptr(), None, t.data_ptr(), None, 2, 4, 2, 0, H.stream())


@pytest.mark.parametrize("N", [2032, 2048, 2560])
def test_slin_bwd_through_ops(N):
    """ops._slin_bwd on either side of the split threshold (N >= 2048, N % 16 == 0): its decision to split and the zeroing of dx agree with
    the C side -- a split launch into an unzeroed dx, or an unsplit one the C side split, would show here."""
    import ops
    M, K = 19, 132
    i = R.slin_bwd_inputs(M, K, N, False, False)
    ref64, ref32 = _slin_bwd_refs(i)
    got = ops._slin_bwd(_dev(i["dy"]), _dev(i["w"]), xn=_dev(i["xn"]))
    torch.cuda.synchronize()
    for k, name in enumerate(("dx", "dw", "db")):
        _check("ops._slin_bwd", name, (M, K, N), got[k].cpu(), ref64[k], ref32[k], BWD_TOL)


def test_linear_fn_through_ops():
    """ops.LinearFn (the G entry / D head layers) forward and backward through autograd at a split shape."""
    import ops
    M, K, N = 19, 132, 2560
    i = R.slin_bwd_inputs(M, K, N, False, False)
    b = R._randn(R._gen(7), N)
    y64 = R.linear(_d(i["xn"]), _d(i["w"]), _d(b))[0]
    y32 = R.linear(i["xn"], i["w"], b)[0]
    ref64, ref32 = _slin_bwd_refs(i)
    x, w, bias = (_dev(t).requires_grad_(True) for t in (i["xn"], i["w"], b))
    y = ops.LinearFn.apply(x, w, bias, None)
    y.backward(_dev(i["dy"]))
    torch.cuda.synchronize()
    _check("LinearFn", "y", (M, K, N), y.detach().cpu(), y64, y32, FWD_TOL)
    for k, (name, p) in enumerate((("dx", x), ("dw", w), ("db", bias))):
        _check("LinearFn", name, (M, K, N), p.grad.cpu(), ref64[k], ref32[k], BWD_TOL)


# =====================================================================================================
# ln_fwd / ln_bwd
# =====================================================================================================
@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_layer_norm(case):
    M, K, l2 = case
    i = R.ln_inputs(M, K, l2)
    x64, g64, b64, dy64, dres64 = (_d(i[k]) for k in ("x", "g", "b", "dy", "dres"))
    ref64 = R.layer_norm(x64, g64, b64, i["eps"], bool(l2))
    ref32 = R.layer_norm(i["x"], i["g"], i["b"], i["eps"], bool(l2))
    x, g, b, dy, dres = (_dev(i[k]) for k in ("x", "g", "b", "dy", "dres"))
    y, xhat, rstd = Out((M, K)), Out((M, K)), Out((M,))
    got = _call("ieagan_ln_fwd", [y, xhat, rstd], x, g, b, y, xhat, rstd, M, K, float(i["eps"]), int(bool(l2)))
    for name, t, r64, r32 in zip(("y", "xhat", "rstd"), got, ref64, ref32):
        _check("ln_fwd", name, case, t, r64, r32, FWD_TOL)
    if M >= 2:
        assert torch.equal(got[1][1], torch.zeros(K))              # the constant row
    if l2 == "zero":
        assert torch.equal(got[0], torch.zeros(M, K))              # u = 0: the clamp gives finite zeros
    # backward on the fp32 CPU forward's xhat / rstd (inputs of both sides), every combination of the two optional parts.
    # K = 1: xhat, the LayerNorm's dx and the gradient of y = sign(beta) are identically 0 -- compared on the scale of their terms
    xh32, rs32 = ref32[1], ref32[2]
    floor = (i["dy"].abs().max() / (i["b"].abs().min() if l2 is True else 1.0)).item() if K == 1 else 0.0
    floor_x = floor * (rs32.max() * i["g"].abs().max()).item()
    for with_res in (False, True):
        for with_param in (False, True):
            tag = f"{case} dres={int(with_res)} dparam={int(with_param)}"
            a64 = (dy64, _d(xh32), _d(rs32), g64, b64 if l2 else None, dres64 if with_res else None)
            a32 = (i["dy"], xh32, rs32, i["g"], i["b"] if l2 else None, i["dres"] if with_res else None)
            r64, r32 = R.layer_norm_bwd(*a64), R.layer_norm_bwd(*a32)
            dx = Out((M, K))
            dg = Out((K,), fill=i["dg0"]) if with_param else None
            dbeta = Out((K,), fill=i["dbeta0"]) if with_param else None
            outs = [dx] + ([dg, dbeta] if with_param else [])
            got = _call("ieagan_ln_bwd", outs, dy, _dev(xh32), _dev(rs32), g, b if l2 else None, dres if with_res else None, dx, dg, dbeta, M, K)
            _check("ln_bwd", "dx", tag, got[0], r64[0], r32[0], BWD_TOL, floor_x)
            if with_param:                          # ADDED to the previous contents
                _check("ln_bwd", "dg", tag, got[1].double() - _d(i["dg0"]), r64[1], r32[1], BWD_TOL, floor)
                _check("ln_bwd", "dbeta", tag, got[2].double() - _d(i["dbeta0"]), r64[2], r32[2], BWD_TOL, floor)


# =====================================================================================================
# embed_norm_fwd / _bwd
# =====================================================================================================
@pytest.mark.parametrize("case", R.EMBED_CASES, ids=str)
def test_embed_norm(case):
    D, kind = case
    M, classes = R.EMBED_M, R.EMBED_CLASSES
    i = R.embed_inputs(D, kind)
    ref64, ref32 = R.embed_norm(i["y"], _d(i["w"])), R.embed_norm(i["y"], i["w"])
    yidx, w, dp = _dev(i["y"]), _dev(i["w"]), _dev(i["dp"])
    p, inv = Out((M, D)), Out((M,))
    got = _call("ieagan_embed_norm_fwd", [p, inv], yidx, w, p, inv, M, D)
    _check("embed_norm_fwd", "p", case, got[0], ref64[0], ref32[0], FWD_TOL)
    _check("embed_norm_fwd", "inv", case, got[1], ref64[1], ref32[1], FWD_TOL)
    if kind == "zero_row":
        assert torch.equal(got[0][0], torch.zeros(D))              # a zero weight row: finite zeros
    # backward on the fp32 CPU forward's p / inv; dW is ADDED to (scatter-add: 40 colliding atomics per element for "same").
    # D = 1: p = +-1 and its gradient is identically 0 -- compared on the scale of its terms dp * inv
    p32, inv32 = ref32
    r64 = R.embed_norm_bwd(i["y"], _d(p32), _d(inv32), _d(i["dp"]), classes)
    r32 = R.embed_norm_bwd(i["y"], p32, inv32, i["dp"], classes)
    floor = (i["dp"].abs().max() * inv32[inv32 < 1e11].max()).item() if (D == 1 and kind != "zero_row") else 0.0
    dw = Out((classes, D), fill=i["dw0"])
    got = _call("ieagan_embed_norm_bwd", [dw], yidx, _dev(p32), _dev(inv32), dp, dw, M, D)
    _check("embed_norm_bwd", "dw", case, got[0].double() - _d(i["dw0"]), r64, r32, BWD_TOL, floor)
    untouched = [c for c in range(classes) if c not in set(i["y"].tolist())]
    assert torch.equal(got[0][untouched], i["dw0"][untouched])     # rows of classes that do not occur keep their contents


# =====================================================================================================
# rrm_attention
# =====================================================================================================
@pytest.mark.parametrize("case", R.ATTENTION_CASES, ids=str)
def test_rrm_attention(case):
    B, S, heads, hd, scale = case
    i = R.attention_inputs(*case)
    ref64, ref32 = R.attention(_d(i["qkv"]), heads), R.attention(i["qkv"], heads)
    qkv, dout = _dev(i["qkv"]), _dev(i["dout"])
    out, att = Out((B, S, heads * hd)), Out((B, heads, S, S))
    got = _call("ieagan_rrm_attention_fwd", [out, att], qkv, out, att, B, S, heads, hd)
    _check("rrm_attention_fwd", "out", case, got[0], ref64[0], ref32[0], FWD_TOL)
    _check("rrm_attention_fwd", "att", case, got[1], ref64[1], ref32[1], FWD_TOL)
    att32 = ref32[1].contiguous()                  # the backward reads the saved affinity: an input of both sides
    r64 = R.attention_bwd(_d(i["qkv"]), _d(att32), _d(i["dout"]), heads)
    r32 = R.attention_bwd(i["qkv"], att32, i["dout"], heads)
    dqkv = Out((B, S, heads * 3 * hd))
    got = _call("ieagan_rrm_attention_bwd", [dqkv], qkv, _dev(att32), dout, dqkv, B, S, heads, hd)
    _check("rrm_attention_bwd", "dqkv", case, got[0], r64, r32, BWD_TOL)


def test_rrm_attention_limits():
    """Both entries take exactly the same shapes (the backward's LDS decides) and refuse any other with the same message; ops.py's predicate
    (the routing of RRM.py) agrees.  The largest accepted footprints run in test_rrm_attention: (1, 64, 2, 64) and (1, 59, 1, 128)."""
    import ops
    H = _H()
    t = torch.zeros(64 * 64 * 8, device=DEV)
    for S, hd, ok in ((64, 128, False), (60, 128, False), (59, 128, True), (64, 64, True), (65, 4, False), (0, 4, False)):
        assert ops.rrm_attention_fits(S, hd) == ok, (S, hd)
        if ok:
            continue
        msgs = []
        for name, nptr in (("ieagan_rrm_attention_fwd", 3), ("ieagan_rrm_attention_bwd", 4)):
            with pytest.raises(RuntimeError, match="rrm_attention: ") as e:
                H.call(name, *[t.data_ptr()] * nptr, 1, S, 1, hd, H.stream())
            msgs.append(str(e.value).split("): ", 1)[1])
        assert msgs[0] == msgs[1], msgs
        assert ("does not fit LDS" in msgs[0]) == (1 <= S <= 64), msgs
    with pytest.raises(RuntimeError, match="null pointer"):
        H.call("ieagan_rrm_attention_fwd", t.data_ptr(), None, t.data_ptr(), 1, 8, 1, 4, H.stream())


# =====================================================================================================
# glue kernels: exact
# =====================================================================================================
@pytest.mark.parametrize("shape", [(3, 35, 40), (2, 4, 300), (2, 1024, 264)], ids=str)
def test_relu_sum_pool(shape):
    """(2, 1024, 264): 2112 blocks of work on the backward's 2048-block grid, the grid-stride loop wraps."""
    N, HW, C = shape
    gen = R._gen(8, *shape)
    x = R.grid(gen, N, HW, C)
    x.view(-1)[::5] = 0.0
    x.view(-1)[1::7] = -0.0
    dh = R._randn(gen, N, C)                       # not bf16 values: the backward rounds them
    xb = x.to(BF16)
    assert torch.equal(xb.float(), x)
    out = Out((N, C))
    got = _call("ieagan_relu_sum_pool", [out], _dev(xb), out, N, HW, C)
    assert torch.equal(got[0], R.relu_sum_pool(x.double()).float())
    dx = Out((N, HW, C), BF16)
    got = _call("ieagan_relu_sum_pool_bwd", [dx], _dev(xb), _dev(dh), dx, N, HW, C)
    assert torch.equal(got[0], R.relu_sum_pool_bwd(x.double(), dh.double()).float().to(BF16))


@functools.lru_cache(maxsize=None)
def _layout_input():
    """fp32 [4, 40, 70] whose bf16 ROUNDING is a multiple of 1/8: grid values plus a quarter of a bf16 ulp (or less) on the non-zero ones."""
    x = R.grid(R._gen(9), 4, 40, 70)
    return torch.where(x != 0, x + 2.0 ** -12, x)


@pytest.mark.parametrize("npe", [2, 0, None], ids=lambda v: f"npe={v}")
def test_nchw_to_nhwc(npe):
    N, C, HW = 4, 40, 70
    x = _layout_input()
    xr = x.to(BF16)                                                 # the rounded values
    assert not torch.equal(xr.float(), x) and torch.equal(xr.float() * 8, (xr.float() * 8).round())
    out = Out((N, HW, C), BF16)
    stats = None
    if npe is not None:                            # sized like ops.ToNHWCFn: one slot per (image of the event, 32-pixel block); ADDED to
        events = N // npe if npe else 1
        slots = (N // events) * ((HW + 31) // 32)
        stats = Out((events, slots, 2, C), fill=0.5)
    got = _call("ieagan_nchw_to_nhwc", [out] + ([stats] if stats is not None else []), _dev(x), out, stats, N, C, HW, npe or 0)
    assert torch.equal(got[0], xr.transpose(1, 2).contiguous())
    if stats is not None:
        ref = torch.stack([R.channel_stats(xr[e * (N // events):(e + 1) * (N // events)].double().transpose(1, 2)) for e in range(events)])
        assert torch.equal(got[1].double().sum(1), ref + 0.5 * slots)
    back = Out((N, C, HW))
    got_b = _call("ieagan_nhwc_to_nchw", [back], out.t, back, N, C, HW)
    assert torch.equal(got_b[0], xr.float())


@pytest.mark.parametrize("C", [8, 40, 2048])
def test_channel_stats(C):
    H = _H()
    P = 37
    x = R.grid(R._gen(10, C), P, C)
    st = Out((H.STAT_REPL, 2, C), fill=0.25)       # replicas, ADDED to
    got = _call("ieagan_channel_stats", [st], _dev(x.to(BF16)), st, P, C)
    assert torch.equal(got[0].double().sum(0), R.channel_stats(x.double()) + 0.25 * H.STAT_REPL)


@pytest.mark.parametrize("mode", [1, 2])
def test_res_bwd(mode):
    """Ca < Cr (channels [Ca, Cr) are zero-filled) and Cg > Ca (the gradient's row stride is its own)."""
    N, Hr, Wr, Cr, Ca, Cg = 2, 6, 10, 24, 16, 32
    Hg, Wg = (2 * Hr, 2 * Wr) if mode == 1 else (Hr // 2, Wr // 2)
    g = R.grid(R._gen(11, mode), N, Hg, Wg, Cg)
    dr = Out((N, Hr, Wr, Cr), BF16)
    got = _call("ieagan_res_bwd", [dr], _dev(g.to(BF16)), Cg, dr, Cr, Ca, mode, N, Hr, Wr)
    ref = R.res_bwd(g.double(), Cr, Ca, mode, Hr, Wr).float().to(BF16)      # (a 2x2 sum may need bf16 rounding: nearest-even on both sides)
    assert torch.equal(got[0], ref)
    assert torch.equal(got[0][..., Ca:], torch.zeros(N, Hr, Wr, Cr - Ca, dtype=BF16))


def test_glue_bad_calls():
    """Null pointers and non-positive sizes are refused with a message, not launched."""
    H = _H()
    t = torch.zeros(4096, device=DEV)
    p, s = t.data_ptr(), H.stream()
    for name, args, msg in (("ieagan_relu_sum_pool", (None, p, 2, 4, 8, s), "relu_sum_pool: null pointer"),
                            ("ieagan_relu_sum_pool", (p, p, 2, 0, 8, s), "relu_sum_pool: N=2 HW=0 C=8"),
                            ("ieagan_relu_sum_pool_bwd", (p, p, p, 2, 4, 0, s), "relu_sum_pool_bwd: N=2 HW=4 C=0"),
                            ("ieagan_relu_sum_pool_bwd", (p, None, p, 2, 4, 8, s), "relu_sum_pool_bwd: null pointer"),
                            ("ieagan_nchw_to_nhwc", (p, p, None, 2, 8, 0, 0, s), "nchw_to_nhwc: N=2 C=8 HW=0"),
                            ("ieagan_nchw_to_nhwc", (p, None, None, 2, 8, 4, 0, s), "nchw_to_nhwc: null pointer"),
                            ("ieagan_nhwc_to_nchw", (p, None, 2, 8, 4, s), "nhwc_to_nchw: null pointer"),
                            ("ieagan_nhwc_to_nchw", (p, p, 0, 8, 4, s), "nhwc_to_nchw: N=0 C=8 HW=4")):
        with pytest.raises(RuntimeError, match=msg):
            H.call(name, *args)
