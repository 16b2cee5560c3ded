"""The checker of tests/test_sn_gpu.py (tests/sn_reference.py) pinned on the CPU: its fp64 power iteration against ``F.normalize``, its
closed-form backward and its layout maps against fp64 ``torch.autograd`` through W / sigma, both to 1e-12, on the GPU tests' own case
lists and inputs; the conditioning of every case (the same reference in fp32 on the CPU stays within 2e-6 of fp64, so the GPU bounds
of 2e-5 / 1e-4 measure the kernels and not the problem); the one-rounding bf16 helper; and the pack layout of ``ops.SNBank`` for the
shipped networks."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

import sn_reference as S

TOL = 1e-12
COND = 2e-6                # fp32 on the CPU against fp64: an ill-conditioned case is replaced, never loosened
BF16_SHARE = 2e-3

ALL_BWD_CASES = (S.BWD_FUSED_CASES + S.BWD_LARGE_CASES + [(k, s) for k, s, _ in S.BATCHED_LAYERS if (k, s) not in S.BWD_FUSED_CASES]
                 + [(0, (o, i)) for i in S.STACK_BWD_INS for o in S.STACK_BWD_OUTS])
# (kind, shape, eps, scale of the weight): every forward call of the GPU file
ALL_FWD_CASES = ([(k, s, S.EPS_MODEL, 1.0) for k, s in S.FWD_CASES + S.STACK_LAYERS + [(0, (79, 256)), (0, (100, 200))]]
                 + [(k, s, S.EPS_BIG, sc) for k, s in S.MODE_CASES for sc in (1.0, S.TINY)])


def _close(got, ref, tag):
    e = S.rel_err(got, ref)
    assert e <= TOL, f"{tag}: {e:.3e}"


# ---------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_FWD_CASES, ids=str)
def test_power_iteration_is_the_normalize_form(case):
    kind, shape, eps, scale = case
    i = S.fwd_inputs(kind, shape, scale)
    W, u = i["W"].double(), i["u"].double()
    Wm = W.reshape(W.shape[0], -1)
    sigma, u_new, v_raw, v, t = S.power_iteration(Wm, u, eps)
    v_ref = F.normalize(u[None] @ Wm, eps=eps)
    u_ref = F.normalize(v_ref @ Wm.t(), eps=eps)
    _close(v_raw, (u[None] @ Wm)[0], "v_raw")
    _close(v, v_ref[0], "v")
    _close(t, (v_ref @ Wm.t())[0], "t")
    _close(u_new, u_ref[0], "u_new")
    _close(sigma, ((v_ref @ Wm.t()) @ u_ref.t()).squeeze(), "sigma")
    assert all(torch.isfinite(x).all() for x in (sigma, u_new, v, t)) and sigma > 0
    if scale != 1.0:            # both clamps decide: |v_raw| < eps and |t| < eps
        assert v_raw.norm() < eps and t.norm() < eps
        assert torch.isfinite(W / sigma).all()


def test_layouts_by_index():
    """The consumer layouts element by element, as the comments of sn.hip state them."""
    g = S._gen(23)
    out, cin, taps = 5, 3, 9
    P = S._randn(g, out, cin, 3, 3)
    fwd, dg = S.to_consumer(P, 1), S.dgrad_pack(P)
    assert fwd.shape == (out, 32) and dg.shape == (cin, 64)
    for o in range(out):
        for c in range(cin):
            for tap in range(taps):
                w = P[o, c, tap // 3, tap % 3]
                assert fwd[o, tap * cin + c] == w
                assert dg[c, (taps - 1 - tap) * out + o] == w
    assert torch.equal(fwd[:, taps * cin:], torch.zeros(out, 32 - 27)) and torch.equal(dg[:, taps * out:], torch.zeros(cin, 64 - 45))
    C = 7
    P2, P3 = S._randn(g, C, 1, 3, 3), S._randn(g, 1, C, 3, 3)
    c2, c3 = S.to_consumer(P2, 2), S.to_consumer(P3, 3)
    assert c2.shape == c3.shape == (9, C)
    for c in range(C):
        for tap in range(9):
            assert c2[tap, c] == P2[c, 0, tap // 3, tap % 3] and c3[tap, c] == P3[0, c, tap // 3, tap % 3]
    P0 = S._randn(g, 4, 6)
    assert torch.equal(S.to_consumer(P0, 0), P0)
    for kind, P in ((0, P0), (1, P), (2, P2), (3, P3)):
        assert torch.equal(S.from_consumer(S.to_consumer(P, kind), P.shape, kind), P)


# ---------------------------------------------------------------------------------------------------
# backward: the closed form (and the layout maps, in and out) against autograd
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_BWD_CASES, ids=str)
def test_closed_form_backward_is_autograd(case):
    kind, shape = case
    i = S.bwd_inputs(kind, shape)
    out, inn = i["out"], i["inn"]
    sigma, u_new, _, v, _ = S.ctx_unpack(i["ctx"].double(), out, inn)
    W = i["W"].double().requires_grad_(True)
    sig = u_new @ (W.reshape(out, inn) @ v)                      # sigma = u' W v^T with u', v constant
    loss = (S.to_consumer(W / sig, kind) * i["gsn"].double()).sum()          # the padding columns of gsn meet zeros
    (ref,) = torch.autograd.grad(loss, [W])
    # the closed form is stated at the ctx record's own sigma; the differentiable one is that value up to the record's fp32 rounding
    assert abs(sig.item() / sigma.item() - 1) < 1e-6
    _close(S.sn_backward(i["gsn"].double(), W.detach(), sig.detach(), u_new, v, kind), ref, "dW")
    b = i["colsum"].double().requires_grad_(True)
    (db,) = torch.autograd.grad((b.reshape(S.STAT_REPL, i["nb"]).sum(0) * i["db0"].double()).sum(), [b])
    assert torch.equal(S.bias_fold(i["colsum"].double(), i["nb"]), i["colsum"].double().reshape(S.STAT_REPL, -1).sum(0))
    assert torch.equal(db, i["db0"].double().repeat(S.STAT_REPL))


def test_ctx_record_layout():
    out, inn = 3, 5
    c = S.ctx_pack(out, inn, 2.0, torch.arange(3.) + 10, torch.arange(5.) + 20, torch.arange(5.) + 30, torch.arange(3.) + 40, fill=-1.0)
    assert c.tolist() == [2, -1, -1, -1, -1, -1, -1, -1, 10, 11, 12, 20, 21, 22, 23, 24, 30, 31, 32, 33, 34, 40, 41, 42]
    assert S.ctx_unwritten(out, inn).nonzero().flatten().tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert S.ctx_size(1, 2) == 16 and S.ctx_unwritten(1, 2).nonzero().flatten().tolist() == [1, 2, 3, 4, 5, 6, 7, 14, 15]


# ---------------------------------------------------------------------------------------------------
# conditioning
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_FWD_CASES, ids=str)
def test_forward_cases_are_well_conditioned(case):
    kind, shape, eps, scale = case
    i = S.fwd_inputs(kind, shape, scale)
    r64, r32 = S.forward_ref(i["W"].double(), i["u"].double(), eps, kind), S.forward_ref(i["W"], i["u"], eps, kind)
    for k in ("sigma", "u_new", "v_raw", "v", "t"):
        e = S.rel_err(r32[k], r64[k])
        assert e <= COND, f"{k}: {e:.3e}"
    for n, (a, b) in enumerate(zip(r32["packs"], r64["packs"])):
        e = S.rel_err(a, b)
        assert e <= COND, f"pack {n}: {e:.3e}"


@pytest.mark.parametrize("case", ALL_BWD_CASES, ids=str)
def test_backward_cases_are_well_conditioned(case):
    kind, shape = case
    i = S.bwd_inputs(kind, shape)
    (dw64, db64), (dw32, db32) = S.backward_ref(i, kind, torch.float64), S.backward_ref(i, kind, torch.float32)
    assert dw32.dtype == torch.float32
    for name, a, b in (("dW", dw32, dw64), ("dbias", db32, db64)):
        e = S.rel_err(a, b)
        assert e <= COND, f"{name}: {e:.3e}"


# ---------------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------------
def test_bf16_neighbours():
    x = S._randn(S._gen(24), 4096) * 3
    rne, lo, hi = S.bf16_neighbours(x.double())
    assert torch.equal(rne, x.to(torch.bfloat16).float())            # fp32 inputs: the library's rounding is a single one
    assert torch.equal(lo.abs().view(torch.int32) + 0x10000, rne.abs().view(torch.int32))
    assert torch.equal(hi.abs().view(torch.int32) - 0x10000, rne.abs().view(torch.int32))
    assert torch.equal(torch.signbit(lo), torch.signbit(rne)) and torch.equal(torch.signbit(hi), torch.signbit(rne))
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -8 - 2.0 ** -40],
                     dtype=torch.float64)
    # ties go to the even pattern; 2^-40 beyond a tie is no tie (it is one after a first rounding to fp32)
    assert S.bf16_neighbours(t)[0].tolist() == [1.0, 1 + 2.0 ** -6, -1.0, 1 + 2.0 ** -7, 1.0]
    assert t[3].float().to(torch.bfloat16).float().item() == 1.0


def test_bf16_packs_of_the_fp32_chain():
    """fp32 W * (1 / sigma) rounded to bf16 against the fp64 reference rounded once: the share of elements that differ bounds what a
    correct fp32 kernel can show (expected ~5e-5: fp32 error 2e-7 against a half step of 2^-9), and never more than one step."""
    total = diff = 0
    for kind, shape, eps, scale in ALL_FWD_CASES:
        if kind != 1:
            continue
        i = S.fwd_inputs(kind, shape, scale)
        out, inn, taps, cin = S.dims(i["W"], 1)
        s32 = S.power_iteration(i["W"].reshape(out, inn), i["u"], eps)[0]
        Wn32 = i["W"] * (1.0 / s32)
        r64 = S.forward_ref(i["W"].double(), i["u"].double(), eps, 1)["packs"]
        for a, b, kreal in ((S.to_consumer(Wn32, 1), r64[0], taps * cin), (S.dgrad_pack(Wn32), r64[1], taps * out)):
            got = a.to(torch.bfloat16).float()[:, :kreal]
            rne, lo, hi = (x[:, :kreal] for x in S.bf16_neighbours(b))
            assert ((got == rne) | (got == lo) | (got == hi)).all(), (kind, shape)
            n = int((got != rne).sum())
            assert n <= BF16_SHARE * got.numel(), (kind, shape, n, got.numel())
            total, diff = total + got.numel(), diff + n
    print(f"bf16 share of the fp32 chain: {diff} of {total}")
    assert total > 20000 and diff <= BF16_SHARE * total


# ---------------------------------------------------------------------------------------------------
# ops.SNBank: the pack layout
# ---------------------------------------------------------------------------------------------------
def _old_pack_offsets(bank, stack):
    """The layout rule before stack layers were packed back to back: every layer rounded up to 256 bytes, stack layers first."""
    off, p = 0, {}
    for n in list(stack) + [n for n in bank.names if n not in set(stack)]:
        kind, out, inn, taps, cin, kpad, kpad2 = bank.meta[bank.index[n]][:7]
        nbytes = out * kpad * 2 + cin * kpad2 * 2 if kind == 1 else out * inn * 4
        p[n] = (off, off + out * kpad * 2 if kind == 1 else 0)
        off += (nbytes + 255) // 256 * 256
    return p, off


def test_shipped_networks_keep_their_pack_offsets(ref_cfg):
    """Stack layers lie back to back, rounded to 256 bytes once after the last.  For the shipped generator (96 stacked ccbn linears) and
    discriminator (no stack) every layer's offsets and the pack size come out as under the former rule, which rounded after every layer:
    each stacked layer's out * in * 4 is a multiple of 256 there."""
    import model
    import ops
    from arena import Arena
    for tag, over in (("256x768", {}), ("64x64", {"resolution": 64, "H_base": 1})):
        cfg = dict(ref_cfg, device="cpu", **over)
        with contextlib.redirect_stdout(io.StringIO()):
            G, D = model.Generator(**cfg), model.Discriminator(**cfg)
        for net in (G, D):
            ar = Arena(net)
            entries = [(n, m._sn_kind, m.weight, m.u0, m.sv0) for n, m in model._sn_children(net, "")]
            stack = []
            if net is G:
                stack = [f"blocks.{bi}.0.{bn}.{gb}" for bi in range(len(G.blocks)) for bn in ("bn1", "bn2", "bn3", "bn4") for gb in ("gain", "bias")]
                assert len(stack) == 96 or over
            bank = ops.SNBank(ar.flat, entries, stack=stack)
            old, old_size = _old_pack_offsets(bank, stack)
            assert bank.pack_size == old_size
            for n, m in zip(bank.names, bank.meta):
                assert (m[8], m[9]) == old[n], (tag, n)
            if stack:
                sizes = [bank.meta[bank.index[n]][1] * bank.meta[bank.index[n]][2] * 4 for n in stack]
                assert all(s % 256 == 0 for s in sizes)
                assert bank.stack_total == sum(bank.meta[bank.index[n]][1] for n in stack)


def test_snbank_packs_a_stack_back_to_back_and_rejects_bad_ones():
    import ops
    shapes = [("a", 0, (24, 20)), ("c", 1, (16, 8, 1, 1)), ("b", 0, (40, 20)), ("d", 0, (8, 20)), ("e", 0, (8, 24)), ("f", 2, (16, 1, 3, 3))]
    n = sum((torch.Size(s).numel() + s[0] + 1 + 7) // 8 * 8 + 16 for _, _, s in shapes)
    flat, o, entries = torch.zeros(n), 0, []
    for name, kind, s in shapes:
        t = []
        for m in (torch.Size(s).numel(), s[0], 1):
            t.append(flat[o:o + m])
            o += (m + 7) // 8 * 8
        entries.append((name, kind, t[0].view(s), t[1], t[2]))
    bank = ops.SNBank(flat, entries, stack=("b", "d", "a"))
    p1 = {nm: m[8] for nm, m in zip(bank.names, bank.meta)}
    assert (p1["b"], p1["d"], p1["a"]) == (0, 3200, 3840) and bank.stack_total == 72
    rest = sorted(p1[k] for k in "cef")
    assert rest[0] == 5888 and all(r % 256 == 0 for r in rest)          # 72 * 80 = 5760 -> rounded once
    assert bank.stack_rows == {"b": (0, 40), "d": (40, 8), "a": (48, 24)}
    with pytest.raises(ValueError, match="only kind-0"):
        ops.SNBank(flat, entries, stack=("a", "c"))
    with pytest.raises(ValueError, match="share their length"):
        ops.SNBank(flat, entries, stack=("a", "e"))
    with pytest.raises(ValueError, match="distinct layers"):
        ops.SNBank(flat, entries, stack=("a", "zz"))
