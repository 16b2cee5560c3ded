"""The checker of tests/test_small_ops_gpu.py pinned against fp64 ``torch.autograd`` of the library layers (F.linear, F.layer_norm,
F.normalize, F.embedding, torch.softmax, F.interpolate, F.avg_pool2d) on the GPU tests' own case lists and inputs, to 1e-12."""
import pytest
import torch
import torch.nn.functional as F

import small_ops_reference as R

TOL = 1e-12


def _d(t):
    return None if t is None else t.double()


def _leaf(t):
    return t.double().requires_grad_(True)


def _close(got, ref, tag, floor=0.0):
    e = R.rel_err(got, ref, floor)
    assert e <= TOL, f"{tag}: {e:.3e}"


@pytest.mark.parametrize("case", R.SLIN_FWD_CASES, ids=str)
def test_linear_forward(case):
    M, K, N = case[:3]
    i = R.slin_fwd_inputs(*case)
    x, w = _d(i["x"]), _d(i["w"])
    y, xhat, rstd, xn = R.linear(x, w, _d(i["b"]), _d(i["res"]), _d(i["ln_g"]), _d(i["ln_b"]), i["relu"], i["eps"])
    t = x
    if i["ln_g"] is not None:
        t = F.layer_norm(x, (K,), _d(i["ln_g"]), _d(i["ln_b"]), i["eps"])
        _close(xhat, F.layer_norm(x, (K,), None, None, i["eps"]), "xhat")
        _close(rstd, (x.var(1, unbiased=False) + i["eps"]).rsqrt(), "rstd")
        if M >= 2:
            assert torch.equal(xhat[1], torch.zeros(K, dtype=torch.float64))      # the constant row
    _close(xn, t, "xn")
    t = F.linear(t, w, _d(i["b"]))
    if i["relu"]:
        t = F.relu(t)
    if i["res"] is not None:
        t = t + _d(i["res"])
    _close(y, t, "y")


@pytest.mark.parametrize("case", R.SLIN_BWD_CASES, ids=str)
def test_linear_backward(case):
    M, K, N, ln, mask = case[:5]
    i = R.slin_bwd_inputs(M, K, N, ln, mask)
    dx, dw, db = R.linear_bwd(_d(i["dy"]), _d(i["w"]), _d(i["xn"]), _d(i["xhat"]), _d(i["ln_g"]), _d(i["ln_b"]), _d(i["ymask"]))
    xn = (_d(i["xhat"]) * _d(i["ln_g"]) + _d(i["ln_b"])).requires_grad_(True) if ln else _leaf(i["xn"])
    w, b = _leaf(i["w"]), torch.zeros(N, dtype=torch.float64, requires_grad=True)
    g = _d(i["dy"])
    if mask:
        assert (i["ymask"] == 0).any() and (i["ymask"] < 0).any() and (i["ymask"] > 0).any()
        g = g * (_d(i["ymask"]) > 0)
    (F.linear(xn, w, b) * g).sum().backward()
    _close(dx, xn.grad, "dx")
    _close(dw, w.grad, "dw")
    _close(db, b.grad, "db")


@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_layer_norm(case):
    M, K, l2 = case
    i = R.ln_inputs(M, K, l2)
    x, g, b = _leaf(i["x"]), _leaf(i["g"]), _leaf(i["b"])
    t = F.layer_norm(x, (K,), g, b, i["eps"])
    if l2:
        t = F.normalize(t, dim=1)
    y, xhat, rstd = R.layer_norm(_d(i["x"]), _d(i["g"]), _d(i["b"]), i["eps"], bool(l2))
    _close(y, t, "y")
    assert torch.isfinite(y).all()
    if l2 == "zero":
        assert torch.equal(y, torch.zeros_like(y))
    for dres in (None, _d(i["dres"])):
        for p in (x, g, b):
            p.grad = None
        loss = (t * _d(i["dy"])).sum() + (0 if dres is None else (x * dres).sum())
        loss.backward(retain_graph=True)
        dx, dg, dbeta = R.layer_norm_bwd(_d(i["dy"]), xhat, rstd, _d(i["g"]), _d(i["b"]) if l2 else None, dres)
        # K = 1: xhat and the LayerNorm's dx are identically 0 and, with F.normalize, y = sign(beta) has gradient 0 -- dx, d gamma and
        # d beta are then compared on the scale of their terms, rstd * dy * gamma and dy (/ |u|)
        floor = (i["dy"].abs().max() / (i["b"].abs().min() if l2 is True else 1.0)).item() if K == 1 else 0.0
        _close(dx, x.grad, "dx", floor * (rstd.max() * i["g"].abs().max()).item())
        _close(dg, g.grad, "dg", floor)
        _close(dbeta, b.grad, "dbeta", floor)
        assert torch.isfinite(dx).all() and torch.isfinite(dg).all() and torch.isfinite(dbeta).all()


@pytest.mark.parametrize("case", R.EMBED_CASES, ids=str)
def test_embed_norm(case):
    D, kind = case
    i = R.embed_inputs(D, kind)
    w = _leaf(i["w"])
    t = F.normalize(F.embedding(i["y"], w), dim=1)
    p, inv = R.embed_norm(i["y"], _d(i["w"]))
    _close(p, t, "p")
    (t * _d(i["dp"])).sum().backward()
    dw = R.embed_norm_bwd(i["y"], p, inv, _d(i["dp"]), R.EMBED_CLASSES)
    floor = (i["dp"].abs().max() * inv[inv < 1e11].max()).item() if D == 1 else 0.0
    _close(dw, w.grad, "dw", 0.0 if kind == "zero_row" else floor)
    assert torch.isfinite(p).all() and torch.isfinite(dw).all()
    if kind == "zero_row":
        assert torch.equal(p[0], torch.zeros(D, dtype=torch.float64))


@pytest.mark.parametrize("case", R.ATTENTION_CASES, ids=str)
def test_attention(case):
    B, S, H, hd, scale = case
    i = R.attention_inputs(*case)
    qkv = _leaf(i["qkv"])
    q, k, v = qkv.view(B, S, H, 3, hd).permute(3, 0, 2, 1, 4)
    a = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, -1)
    t = (a @ v).permute(0, 2, 1, 3).reshape(B, S, H * hd)
    out, att = R.attention(_d(i["qkv"]), H)
    _close(att, a, "att")
    _close(out, t, "out")
    (t * _d(i["dout"])).sum().backward()
    _close(R.attention_bwd(_d(i["qkv"]), att, _d(i["dout"]), H), qkv.grad, "dqkv")
    if scale > 1:
        assert (i["qkv"].view(B, S, H, 3, hd)[:, :, :, 0] * i["qkv"].view(B, S, H, 3, hd)[:, :, :, 1]).abs().sum(-1).max() < 2 ** 24 / 64


def test_glue():
    gen = R._gen(6)
    x = R.grid(gen, 3, 35, 40).double()
    x[0, :5] = -0.0
    xl = x.clone().requires_grad_(True)
    t = F.relu(xl).sum(1)
    dh = R.grid(gen, 3, 40).double()
    (t * dh).sum().backward()
    assert torch.equal(R.relu_sum_pool(x), t.detach())
    assert torch.equal(R.relu_sum_pool_bwd(x, dh), xl.grad)
    # res_bwd: mode 1 = the residual was upsampled (nearest) before it was added, mode 2 = it was 2x2 average-pooled
    N, Hr, Wr, Cr, Ca, Cg = 2, 6, 10, 24, 16, 32
    for mode in (1, 2):
        H, W = (2 * Hr, 2 * Wr) if mode == 1 else (Hr // 2, Wr // 2)
        g = R.grid(gen, N, H, W, Cg).double()
        r = torch.zeros(N, Hr, Wr, Cr, dtype=torch.float64, requires_grad=True)
        a = r[..., :Ca].permute(0, 3, 1, 2)
        a = F.interpolate(a, scale_factor=2, mode="nearest") if mode == 1 else F.avg_pool2d(a, 2)
        (a.permute(0, 2, 3, 1) * g[..., :Ca]).sum().backward()
        assert torch.equal(R.res_bwd(g, Cr, Ca, mode, Hr, Wr), r.grad)
    x = R.grid(gen, 37, 40).double()
    assert torch.equal(R.channel_stats(x), torch.stack([x.sum(0), x.pow(2).sum(0)]))
