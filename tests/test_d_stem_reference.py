"""tests/d_stem_reference.py (the checker of tests/test_d_stem_gpu.py) against fp64 ``torch.autograd`` of conv2d / avg_pool2d on UNROUNDED
operands.  The restatement rounds the weights, h0, p0 and dh0 to bf16 (2^-9 relative each) and the library layers round nothing, so the
bound is loose: a few bf16 steps of the largest element.  What it pins is the structure -- tap order, padding, the pooled expansion, the
layouts of the weight gradients -- where a mistake costs tens of percent, not the last bits."""
import pytest
import torch
import torch.nn.functional as F

import d_stem_reference as R

LOOSE = 2e-2       # <= 4 roundings of 2^-9 (two operands, h0, the result) on sums whose terms partly cancel
CASES = [(1, 8, 32), (2, 24, 96)]


def _autograd(i):
    """fp64 library layers on the unrounded operands -> forward outputs and the gradients for the out-gradients (dh1, dp0)."""
    x = i["img"].double()[:, None].requires_grad_(True)
    w_in = i["w_in"].double().t().reshape(R.C0, 1, 3, 3).clone().requires_grad_(True)
    b_in = i["b_in"].double().clone().requires_grad_(True)
    w1 = i["w1"].double().reshape(R.C1, R.C0, 1, 1).clone().requires_grad_(True)
    b1 = i["b1"].double().clone().requires_grad_(True)
    h0 = F.conv2d(x, w_in, b_in, padding=1)
    h1 = F.conv2d(h0, w1, b1)
    p0 = F.avg_pool2d(h0, 2)
    sc = F.conv2d(p0, i["wsc"].double().reshape(R.CS, R.C0, 1, 1), i["bsc"].double())
    loss = (h1 * i["dh1"].double().permute(0, 3, 1, 2)).sum() + (p0 * i["dp0"].double().permute(0, 3, 1, 2)).sum()
    gx, gw_in, gb_in, gw1, gb1 = torch.autograd.grad(loss, [x, w_in, b_in, w1, b1])
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
    return dict(h0=nhwc(h0), h1=nhwc(h1), p0=nhwc(p0), sc=nhwc(sc), dw_in=gw_in.reshape(R.C0, 9).t(), db_in=gb_in, dw1=gw1.reshape(R.C1, R.C0),
                db1=gb1, dimg=gx[:, 0])


@pytest.mark.parametrize("n,h,w", CASES)
def test_restatement_against_autograd(n, h, w):
    i = R.inputs(n, h, w)
    ref = _autograd(i)
    h0, h1, p0, sc = R.forward(i["img"], i["w_in"], i["b_in"], i["w1"], i["b1"], i["wsc"], i["bsc"], torch.float64)
    dw_in, db_in, dw1, db1 = R.backward(i["img"], i["w_in"], i["b_in"], i["dh1"], i["dp0"], i["w1_bwd"], torch.float64)
    got = dict(h0=h0, h1=h1, p0=p0, sc=sc, dw_in=dw_in, db_in=db_in, dw1=dw1, db1=db1,
               dimg=R.dimg_of(i["dh1"], i["dp0"], i["w1_bwd"], i["w_in"], torch.float64))
    for k, v in got.items():
        e = R.rel_err(v, ref[k])
        print(f"{k} {n}x{h}x{w}: {e:.3e}")
        assert e <= LOOSE, (k, e)


def test_values_are_bf16_where_the_kernels_round():
    i = R.inputs(1, 8, 32)
    for dt in (torch.float64, torch.float32):
        outs = R.forward(i["img"], i["w_in"], i["b_in"], i["w1"], i["b1"], i["wsc"], i["bsc"], dt)
        for t in outs + (R.dh0_of(i["dh1"], i["dp0"], i["w1_bwd"], dt),):
            assert t.dtype == dt and torch.equal(t.float().to(torch.bfloat16).to(dt), t)
    hi, lo = R.split(i["img"])
    assert ((hi.double() + lo.double()) - i["img"].double()).abs().max() <= 2.0 ** -16          # what two bf16 parts leave of |v| <= 1


def test_fp32_chain_stays_inside_the_gpu_bounds():
    """The fp32 restatement against the fp64 one: few elements round differently, and the sums agree to fp32 accumulation noise."""
    i = R.inputs(2, 24, 96)
    a = R.forward(i["img"], i["w_in"], i["b_in"], i["w1"], i["b1"], i["wsc"], i["bsc"], torch.float64)
    b = R.forward(i["img"], i["w_in"], i["b_in"], i["w1"], i["b1"], i["wsc"], i["bsc"], torch.float32)
    for u, v in zip(a, b):
        assert (u != v.double()).float().mean() <= 2e-3
    ga = R.backward(i["img"], i["w_in"], i["b_in"], i["dh1"], i["dp0"], i["w1_bwd"], torch.float64)
    gb = R.backward(i["img"], i["w_in"], i["b_in"], i["dh1"], i["dp0"], i["w1_bwd"], torch.float32)
    for u, v in zip(ga, gb):
        assert R.rel_err(v, u) <= 1e-4
    da = (i["dh1"], i["dp0"], i["w1_bwd"], i["w_in"])
    assert R.rel_err(R.dimg_of(*da, torch.float32), R.dimg_of(*da, torch.float64)) <= 1e-4
