"""Operator-level tests of the batched spectral normalisation (csrc/sn.hip: ieagan_sn_forward, ieagan_sn_backward, _batched, _stack)
against the plain fp64 restatement of tests/sn_reference.py (pinned against fp64 autograd and F.normalize, and shown to be well
conditioned at every case, in tests/test_sn_reference.py), at the smallest shapes that reach every path of the kernels: single rows,
row chunks of one row, the remainders of the 8-row / 6-column / 8-element load batches, 9 and 10 row chunks in the 8-way fold, padded
and unpadded conv packs, the single-channel forms, both clamps, a bank of many layers with a stack, the 20000-element switch of the
backward and its grid-stride rounds, the bias folds.

The C ABI is called directly (``_hip.call``).  The forward's tables come from ``ops.SNBank`` (so its offsets are under test with the
kernels); the tables of the batched and stacked backward are built by hand from the comments of sn.hip; the ctx records the backward
tests read are those of the fp64 reference, independent of the forward kernels.

Output hygiene as in tests/test_small_ops_gpu.py (tests/gpu_outputs.py): ctx, part, pack, the parameter arena (it holds u and sv) and
every dW / dbias / grad are slices between sentinel guards, NaN-filled where the kernel overwrites and filled with known non-zero
values where it adds.  By contract ctx slots [1, 8), the alignment tails of ctx and pack are not written (exactly those positions are
exempt from the NaN check) and ``part`` is scratch (only its guards are checked).

Tolerances (tests/test_small_ops_gpu.py): max|kernel - fp64| / max|fp64| <= 2e-5 for the forward's fp32 outputs, <= 1e-4 for
gradients, the fp32-CPU yardstick printed next to each figure.  bf16 packs: every element is the fp64 value rounded once to nearest-even
or a bf16 neighbour of it, at most 0.2 % of a pack's elements are not the exact rounding, padding columns are +0 bit for bit."""
import functools

import pytest
import torch

import sn_reference as S
from gpu_outputs import BF16, BWD_TOL, DEV, FWD_TOL, Out, _H, _call, _check, _dev

pytestmark = pytest.mark.gpu

BF16_SHARE = 2e-3
GAP = 3.0                   # what the alignment gaps of a hand-built arena hold


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _flat(tensors, gap=GAP):
    """[t0 | t1 | ...], each starting on a multiple of 8 floats, the gaps hold ``gap``.  -> (flat fp32 CPU tensor, offsets)."""
    offs, cur = [], 0
    for t in tensors:
        offs.append(cur)
        cur += (max(t.numel(), 1) + 7) // 8 * 8
    flat = torch.full((cur,), gap, dtype=torch.float32)
    for t, o in zip(tensors, offs):
        flat[o:o + t.numel()] = t.reshape(-1)
    return flat, offs


def _all(n):
    return torch.ones(n, dtype=torch.bool)


# =====================================================================================================
# ieagan_sn_forward
# =====================================================================================================
class Bank:
    """A bank over a guarded parameter arena; every ``forward`` call runs the C entry into fresh guarded buffers and checks them."""

    def __init__(self, layers, stack=(), scale=1.0):
        import ops
        self.layers = layers                                        # [(name, kind, shape)]
        ins = [S.fwd_inputs(kind, shape, scale) for _, kind, shape in layers]
        self.flat0, offs = _flat([t for i in ins for t in (i["W"], i["u"], i["sv"])])
        self.params = Out((self.flat0.numel(),), fill=self.flat0)
        self.where, entries = {}, []
        for k, ((name, kind, shape), i) in enumerate(zip(layers, ins)):
            ow, ou, osv = offs[3 * k:3 * k + 3]
            nW, out = i["W"].numel(), i["W"].shape[0]
            self.where[name] = (ow, nW, ou, out, osv)
            p = self.params.t
            entries.append((name, kind, p[ow:ow + nW].view(i["W"].shape), p[ou:ou + out], p[osv:osv + 1]))
        self.bank = ops.SNBank(self.params.t, entries, stack=stack)
        # the ctx records as documented: one per layer in table order, each rounded up to 8 floats
        self.ctx_off, self.ctx_exempt, o = {}, [], 0
        for (name, kind, shape), m in zip(layers, self.bank.meta):
            assert m[7] == o
            self.ctx_off[name] = o
            self.ctx_exempt.append(S.ctx_unwritten(m[1], m[2]))
            o += S.ctx_size(m[1], m[2])
        assert o == self.bank.ctx_size and self.bank.pack_size % 256 == 0
        self.ctx_exempt = torch.cat(self.ctx_exempt)

    def forward(self, eps, training):
        b = self.bank
        ctx, part, pack = Out((b.ctx_size,)), Out((b.part_size,)), Out((b.pack_size // 2,), BF16)
        _call("ieagan_sn_forward", [], b.table, b.blocks, b.nblocks, b.cblocks, b.ncblocks, self.params, ctx, part, pack, float(eps),
              int(training))
        res = dict(ctx=ctx.check("ctx", self.ctx_exempt), arena=self.params.check("params"), pack=pack.check("pack", _all(pack.n)))
        part.check("part", _all(part.n))
        return res

    def layer(self, res, name):
        """One layer's share of a forward's buffers: its ctx record, W / u / sv in the arena, its pack(s) as raw bf16 / fp32 rows."""
        kind, out, inn, taps, cin, kpad, kpad2, coff, p1, p2 = self.bank.meta[self.bank.index[name]]
        ow, nW, ou, _, osv = self.where[name]
        a = res["arena"]
        d = dict(ctx=res["ctx"][coff:coff + S.ctx_size(out, inn)], W=a[ow:ow + nW], u=a[ou:ou + out], sv=a[osv:osv + 1])
        if kind == 1:
            assert p1 % 2 == 0 and p2 == p1 + out * kpad * 2
            d["packs"] = (res["pack"][p1 // 2:p1 // 2 + out * kpad].view(out, kpad), res["pack"][p2 // 2:p2 // 2 + cin * kpad2].view(cin, kpad2))
        else:
            assert p1 % 4 == 0
            d["packs"] = (res["pack"].view(torch.float32)[p1 // 4:p1 // 4 + out * inn],)
        for p in d["packs"]:
            assert not torch.isnan(p.float()).any(), f"{name}: pack elements unwritten"
        return d


def _layer_equal(a, b, out, inn):
    keep = ~S.ctx_unwritten(out, inn)
    return (_same_bits(a["ctx"][keep], b["ctx"][keep]) and _same_bits(a["u"], b["u"]) and _same_bits(a["sv"], b["sv"])
            and all(_same_bits(x, y) for x, y in zip(a["packs"], b["packs"])))


def _verify_layer(tag, got, before, kind, shape, eps, training, scale=1.0):
    """One layer of a forward against the fp64 reference: ctx, the arena's W / u / sv, the pack(s)."""
    i = S.fwd_inputs(kind, shape, scale)
    out, inn, taps, cin = S.dims(i["W"], kind)
    r64, r32 = S.forward_ref(i["W"].double(), i["u"].double(), eps, kind), S.forward_ref(i["W"], i["u"], eps, kind)
    sigma, u_new, v_raw, v, t = S.ctx_unpack(got["ctx"], out, inn)
    assert torch.isfinite(got["ctx"][~S.ctx_unwritten(out, inn)]).all()
    for name, g in (("sigma", sigma), ("u_new", u_new), ("v_raw", v_raw), ("v", v), ("t", t)):
        _check("sn_forward", name, tag, g, r64[name], r32[name], FWD_TOL)
    assert _same_bits(got["W"], i["W"].reshape(-1)), "the weight moved"
    if training:
        assert _same_bits(got["u"], u_new) and _same_bits(got["sv"], sigma.reshape(1)), "u / sv are not the ctx record's u' / sigma"
    else:
        assert _same_bits(got["u"], before["u"]) and _same_bits(got["sv"], before["sv"]), "u / sv moved in evaluation mode"
    if kind != 1:
        name = {0: "w_plain [out][in]", 2: "w [9][C]", 3: "w [9][C]"}[kind]
        _check("sn_forward", name, tag, got["packs"][0].view(r64["packs"][0].shape), r64["packs"][0], r32["packs"][0], FWD_TOL)
        return
    for name, p, ref, kreal in (("fwd pack", got["packs"][0], r64["packs"][0], taps * cin), ("dgrad pack", got["packs"][1], r64["packs"][1], taps * out)):
        assert p.shape == ref.shape
        assert torch.equal(_bits(p[:, kreal:]), torch.zeros_like(_bits(p[:, kreal:]))), f"{name} {tag}: padding is not +0"
        g = p[:, :kreal].float()
        rne, lo, hi = (x[:, :kreal] for x in S.bf16_neighbours(ref))
        near = (g == rne) | (g == lo) | (g == hi)
        n = int((g != rne).sum())
        print(f"BF16 sn_forward {name} {tag}: {n} of {g.numel()} not the exact rounding, {int((~near).sum())} beyond a neighbour")
        assert near.all(), f"{name} {tag}: {int((~near).sum())} elements are no bf16 neighbour of the reference, first at {(~near).nonzero()[0].tolist()}"
        assert n <= BF16_SHARE * g.numel(), f"{name} {tag}: {n} of {g.numel()} elements are not the exact rounding"


@functools.lru_cache(maxsize=None)
def _single(kind, shape, eps=S.EPS_MODEL, training=1, scale=1.0):
    """A one-layer bank, run once.  -> (the layer's results, its state before)."""
    b = Bank([("l", kind, shape)], scale=scale)
    before = b.layer(dict(ctx=torch.zeros(b.bank.ctx_size), arena=b.flat0, pack=torch.zeros(b.bank.pack_size // 2, dtype=BF16)), "l")
    return b.layer(b.forward(eps, training), "l"), before


@pytest.mark.parametrize("case", S.FWD_CASES + S.STACK_LAYERS, ids=str)
def test_sn_forward(case):
    kind, shape = case
    got, before = _single(kind, shape)
    _verify_layer(case, got, before, kind, shape, S.EPS_MODEL, 1)


@pytest.mark.parametrize("mode", ["eps=1e-6", "training=0", "tiny weight"])
@pytest.mark.parametrize("case", S.MODE_CASES, ids=str)
def test_sn_forward_modes(case, mode):
    """The other clamp value; evaluation mode (u and sv stay bit for bit, ctx still holds sigma and u'); a weight of ~1e-9 at eps = 1e-6,
    where both clamps decide (|v_raw| < eps, |t| < eps) and everything stays finite."""
    kind, shape = case
    eps, training, scale = {"eps=1e-6": (S.EPS_BIG, 1, 1.0), "training=0": (S.EPS_MODEL, 0, 1.0), "tiny weight": (S.EPS_BIG, 1, S.TINY)}[mode]
    got, before = _single(kind, shape, eps, training, scale)
    _verify_layer((case, mode), got, before, kind, shape, eps, training, scale)
    assert all(torch.isfinite(p.float()).all() for p in got["packs"])


ALL_LAYERS = [(f"{k}{'x'.join(map(str, s))}", k, s) for k, s in S.FWD_CASES]
ALL_LAYERS = [ALL_LAYERS[j] for j in (0, 6, 10, 12, 1, 7, 2, 11, 8, 3, 13, 4, 9, 5)]           # kinds interleaved
for _pos, _l in ((2, S.STACK_LAYERS[0]), (8, S.STACK_LAYERS[1]), (13, S.STACK_LAYERS[2])):
    ALL_LAYERS.insert(_pos, (f"s{_l[1][0]}", *_l))
ALL_STACK = ("s40", "s8", "s24")                                     # not their order in the table


def test_sn_forward_all_layers_in_one_bank():
    """Every layer's ctx, u, sv and pack(s) are bit for bit those of its one-layer bank (a layer's result may not depend on its neighbours:
    the reductions are ordered), with more than one layer per table, pack order following the stack while table rows follow the entries.
    The stack is one contiguous [sum(out), in] matrix: the rows of its layers in stack order."""
    b = Bank(ALL_LAYERS, stack=ALL_STACK)
    res = b.forward(S.EPS_MODEL, 1)
    for name, kind, shape in ALL_LAYERS:
        got = b.layer(res, name)
        _verify_layer(name, got, None, kind, shape, S.EPS_MODEL, 1)
        out, inn = b.bank.meta[b.bank.index[name]][1:3]
        assert _layer_equal(got, _single(kind, shape)[0], out, inn), f"{name}: differs from its one-layer bank"
    gaps = torch.ones(b.flat0.numel(), dtype=torch.bool)
    for ow, nW, ou, out, osv in b.where.values():
        gaps[ow:ow + nW] = gaps[ou:ou + out] = gaps[osv:osv + 1] = False
    assert _same_bits(res["arena"][gaps], b.flat0[gaps]), "a store into the arena outside u / sv"
    # evaluation mode twice: bit-identical buffers (NaN fill included), the arena does not move
    e1, e2 = b.forward(S.EPS_MODEL, 0), b.forward(S.EPS_MODEL, 0)
    for k in ("ctx", "pack", "arena"):
        assert _same_bits(e1[k], e2[k]), f"two evaluation passes differ in {k}"
    assert _same_bits(e1["arena"], res["arena"])
    # through SNBank.run: the stack view
    recs = b.bank.run(False, S.EPS_MODEL)
    torch.cuda.synchronize()
    rows = torch.cat([recs[n].w_plain for n in ALL_STACK]).cpu()
    stack = recs["__stack__"].cpu()
    assert stack.shape == (72, 20)
    assert _same_bits(stack, rows), "recs['__stack__'] is not the rows of its layers in stack order"
    assert _same_bits(rows, torch.cat([b.layer(e1, n)["packs"][0] for n in ALL_STACK]).view(72, 20))
    for name, kind, shape in ALL_LAYERS:                             # ... and the other views of run() are the layer's pack bytes
        r, lay = recs[name], b.layer(e1, name)
        views = (r.w_fwd, r.w_bwd) if kind == 1 else (r.w_plain.reshape(-1),)
        assert all(_same_bits(v.cpu(), p) for v, p in zip(views, lay["packs"])), name
        assert _same_bits(r.ctx.cpu()[8:], lay["ctx"][8:8 + r.ctx.numel() - 8]) and _same_bits(r.ctx.cpu()[:1], lay["ctx"][:1])


def test_snbank_rejects_bad_stacks():
    import ops
    layers = [("a", 0, (24, 20)), ("b", 0, (8, 24)), ("c", 2, (16,))]
    ins = [S.fwd_inputs(k, s) for _, k, s in layers]
    flat, offs = _flat([t for i in ins for t in (i["W"], i["u"], i["sv"])])
    flat = _dev(flat)
    entries = [(n, k, flat[offs[3 * j]:offs[3 * j] + i["W"].numel()].view(i["W"].shape), flat[offs[3 * j + 1]:offs[3 * j + 1] + i["W"].shape[0]],
                flat[offs[3 * j + 2]:offs[3 * j + 2] + 1]) for j, ((n, k, s), i) in enumerate(zip(layers, ins))]
    with pytest.raises(ValueError, match="only kind-0"):
        ops.SNBank(flat, entries, stack=("a", "c"))
    with pytest.raises(ValueError, match="share their length"):
        ops.SNBank(flat, entries, stack=("a", "b"))


def test_sn_forward_bad_calls():
    """Null pointers and a missing column-block table are refused with a message; nothing is launched (the outputs keep their fill)."""
    H = _H()
    b = Bank([("l", 0, (33, 7))])
    k = b.bank
    ctx, part, pack = Out((k.ctx_size,), fill=1.0), Out((k.part_size,), fill=1.0), Out((k.pack_size // 2,), BF16, fill=1.0)
    good = [k.table.data_ptr(), k.blocks.data_ptr(), k.nblocks, k.cblocks.data_ptr(), k.ncblocks, b.params.ptr(), ctx.ptr(), part.ptr(),
            pack.ptr(), 1e-12, 1, H.stream()]
    for pos in (0, 1, 3, 5, 6, 7, 8):
        with pytest.raises(RuntimeError, match="sn_forward: null pointer"):
            H.call("ieagan_sn_forward", *[None if j == pos else a for j, a in enumerate(good)])
    for n in (0, -1):
        with pytest.raises(RuntimeError, match=f"sn_forward: nblocks=2 ncblocks={n}"):
            H.call("ieagan_sn_forward", *[n if j == 4 else a for j, a in enumerate(good)])
    torch.cuda.synchronize()
    for o, name in ((ctx, "ctx"), (part, "part"), (pack, "pack")):
        assert torch.equal(o.check(name).float(), torch.ones(o.n)), f"a refused call wrote {name}"
    assert _same_bits(b.params.check("params"), b.flat0)


# =====================================================================================================
# ieagan_sn_backward
# =====================================================================================================
@functools.lru_cache(maxsize=None)
def _bwd(kind, shape):
    """Inputs (on the device too) and the two references of one backward case, computed once."""
    i = S.bwd_inputs(kind, shape)
    i["ref64"], i["ref32"] = S.backward_ref(i, kind, torch.float64), S.backward_ref(i, kind, torch.float32)
    i["dev"] = {k: _dev(i[k]) for k in ("gsn", "W", "ctx", "colsum")}
    return i


def _sn_backward(i, kind, accumulate, bias_mode, scratch="zero"):
    """One call.  ``bias_mode``: None (no colsum), 0 (dbias overwritten), 1 (added to).  -> (dW, dbias) with previous contents removed."""
    d = i["dev"]
    dW = Out(i["W"].shape, fill=i["dw0"] if accumulate else None)
    db = None if bias_mode is None else Out((i["nb"],), fill=i["db0"] if bias_mode else None)
    inner = torch.zeros(1, device=DEV) if scratch == "zero" else None
    got = _call("ieagan_sn_backward", [dW] + ([db] if db is not None else []), d["gsn"], d["W"], kind, i["out"], i["inn"], i["taps"], i["cin"],
                i["kpad"], d["ctx"], inner, dW, int(accumulate), d["colsum"] if db is not None else None, db, int(bool(bias_mode)))
    raw = list(got)
    if accumulate:
        got[0] = got[0].double() - i["dw0"].double()
    if bias_mode:
        got[1] = got[1].double() - i["db0"].double()
    return got, raw


def _check_backward(entry, case, i, kind, variants, scratch="zero"):
    for accumulate, bias_mode in variants:
        tag = f"{case} accumulate={accumulate} bias={bias_mode}"
        got, _ = _sn_backward(i, kind, accumulate, bias_mode, scratch)
        _check(entry, "dW", tag, got[0], i["ref64"][0], i["ref32"][0], BWD_TOL)
        if bias_mode is not None:
            _check(entry, "dbias", tag, got[1], i["ref64"][1], i["ref32"][1], BWD_TOL)


@pytest.mark.parametrize("case", S.BWD_FUSED_CASES, ids=str)
def test_sn_backward_fused(case):
    """The one-block path (every forward shape of up to 20000 elements -- (20, 1001) has 20020 and runs in test_sn_backward_large -- and the
    boundary shape (100, 200); all without a scratch float): overwrite and accumulate, with and
    without the bias fold (kind 3: a bias of ONE element, the guards of dbias prove it), and twice for the same bits -- the reduction
    is ordered."""
    kind, shape = case
    i = _bwd(kind, shape)
    assert i["out"] * i["inn"] <= S.FUSED_MAX and (i["nb"] == 1) == (kind == 3 or i["out"] == 1)
    variants = [(0, None), (0, 0), (0, 1)] + ([(1, None), (1, 1)] if kind in (0, 1) else [])
    _check_backward("sn_backward fused", case, i, kind, variants, scratch=None)
    a, b = _sn_backward(i, kind, 0, 0, None)[1], _sn_backward(i, kind, 0, 0, None)[1]
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]), "two calls on the same inputs differ"


@pytest.mark.parametrize("case", S.BWD_LARGE_CASES, ids=str)
def test_sn_backward_large(case):
    """The multi-block path (a float atomic per block into a zeroed scratch float: held to the bound, not to the bit)."""
    kind, shape = case
    i = _bwd(kind, shape)
    assert i["out"] * i["inn"] > S.FUSED_MAX
    _check_backward("sn_backward large", case, i, kind, [(0, None), (1, None), (0, 0), (1, 1)])


def test_sn_backward_bad_calls():
    H = _H()
    i = _bwd(1, (37, 5, 9))
    d = i["dev"]
    dW, db = Out(i["W"].shape, fill=1.0), Out((i["nb"],), fill=1.0)
    good = [d["gsn"].data_ptr(), d["W"].data_ptr(), 1, i["out"], i["inn"], i["taps"], i["cin"], i["kpad"], d["ctx"].data_ptr(), None, dW.ptr(),
            0, d["colsum"].data_ptr(), db.ptr(), 0, H.stream()]

    def bad(msg, **at):
        pos = dict(gsn=0, W=1, kind=2, out=3, inn=4, taps=5, cin=6, kpad=7, ctx=8, dW=10, dbias=13)
        args = list(good)
        for k, v in at.items():
            args[pos[k]] = v
        with pytest.raises(RuntimeError, match=msg):
            H.call("ieagan_sn_backward", *args)

    for k in ("gsn", "W", "ctx", "dW"):
        bad("sn_backward: null pointer", **{k: None})
    bad("sn_backward: colsum needs dbias", dbias=None)
    bad("sn_backward: bad kind", kind=4)
    bad("sn_backward: out=0 in=45", out=0)
    bad("sn_backward: out=37 in=-1", inn=-1)
    bad("sn_backward: kind 1 with taps=9 cin=5 kpad=32", kpad=32)
    big = _bwd(0, (79, 256))
    with pytest.raises(RuntimeError, match="large layer needs a zeroed scratch float"):
        H.call("ieagan_sn_backward", big["dev"]["gsn"].data_ptr(), big["dev"]["W"].data_ptr(), 0, 79, 256, 1, 256, 0, big["dev"]["ctx"].data_ptr(),
               None, dW.ptr(), 0, None, None, 0, H.stream())
    torch.cuda.synchronize()
    assert torch.equal(dW.check("dW"), torch.ones(i["W"].shape)) and torch.equal(db.check("dbias"), torch.ones(i["nb"])), "a refused call wrote"


# =====================================================================================================
# ieagan_sn_backward_batched
# =====================================================================================================
def test_sn_backward_batched():
    """Five layers in one call, tables by hand: btab int64[12] = {weight offset (params == grad arena), out, in, taps, cin, kind, kpad,
    ctx offset, gsn offset in scratch, colsum offset in scratch or -1, bias offset in grad or -1, bias length};  work int32[2] = {layer,
    chunk of 2048 elements};  scratch[0, nlayers) = zeroed accumulators.  dW and dbias are ADDED into the gradient arena."""
    ins = [_bwd(k, s) for k, s, _ in S.BATCHED_LAYERS]
    g = S._gen(25)
    biases = [S._randn(g, i["nb"]) if hb else None for i, (_, _, hb) in zip(ins, S.BATCHED_LAYERS)]
    ptens = [t for i, b in zip(ins, biases) for t in ([i["W"]] + ([b] if b is not None else []))]
    params, poffs = _flat(ptens)
    grad0 = S._randn(g, params.numel())
    ctx_all, coffs = _flat([i["ctx"] for i in ins], gap=0.0)
    sc_tensors = [torch.zeros(64)] + [i["gsn"] for i in ins] + [i["colsum"] for i, b in zip(ins, biases) if b is not None]
    scratch, soffs = _flat(sc_tensors)
    btab, work, k, c = [], [], 0, 1 + len(ins)
    where = []
    for li, (i, b, (kind, shape, _)) in enumerate(zip(ins, biases, S.BATCHED_LAYERS)):
        ow = poffs[k]
        k += 1
        ob = cs = -1
        if b is not None:
            ob, cs = poffs[k], soffs[c]
            k, c = k + 1, c + 1
        btab.append([ow, i["out"], i["inn"], i["taps"], i["cin"], kind, i["kpad"], coffs[li], soffs[1 + li], cs, ob, i["nb"] if b is not None else 0])
        work += [[li, ch] for ch in range((i["out"] * i["inn"] + S.SNB_CHUNK - 1) // S.SNB_CHUNK)]
        where.append((ow, ob))
    assert [sum(1 for w in work if w[0] == li) for li in range(5)] == [7, 1, 1, 1, 1] and btab[4][9] == -1 and btab[1][10] == -1
    grad = Out((params.numel(),), fill=grad0)
    got = _call("ieagan_sn_backward_batched", [grad], torch.tensor(btab, dtype=torch.int64, device=DEV),
                torch.tensor(work, dtype=torch.int32, device=DEV), len(work), _dev(params), _dev(ctx_all), _dev(scratch), grad)[0]
    untouched = torch.ones(params.numel(), dtype=torch.bool)
    for (ow, ob), i, (kind, shape, hb) in zip(where, ins, S.BATCHED_LAYERS):
        n = i["W"].numel()
        untouched[ow:ow + n] = False
        dW = (got[ow:ow + n].double() - grad0[ow:ow + n].double()).view(i["W"].shape)
        _check("sn_backward_batched", "dW", (kind, shape), dW, i["ref64"][0], i["ref32"][0], BWD_TOL)
        if hb:
            untouched[ob:ob + i["nb"]] = False
            db = got[ob:ob + i["nb"]].double() - grad0[ob:ob + i["nb"]].double()
            _check("sn_backward_batched", "dbias", (kind, shape), db, i["ref64"][1], i["ref32"][1], BWD_TOL)
    assert untouched.sum() > 0 and _same_bits(got[untouched], grad0[untouched]), "the rest of the gradient arena moved"


# =====================================================================================================
# ieagan_sn_backward_stack
# =====================================================================================================
@pytest.mark.parametrize("inn", S.STACK_BWD_INS)
def test_sn_backward_stack(inn):
    """Block b handles stack layer b: gst [sum out][in], layers[b] = row of the layer table (F_W, F_OUT, F_IN, F_CTX are read), row0[b] =
    first row in gst, dst[b] = element offset of its gradient.  Overwriting into a flat [sum out, in] buffer, accumulating into an arena
    at scattered offsets; the reduction is ordered: two calls, the same bits."""
    ins = [_bwd(0, (o, inn)) for o in S.STACK_BWD_OUTS]
    params, poffs = _flat([i["W"] for i in ins])
    ctx_all, coffs = _flat([i["ctx"] for i in ins], gap=0.0)
    # a table with a row the call does not name in between, layers in another order than their rows
    rows = {0: 2, 1: 0, 2: 4, 3: 1}                                    # call position -> table row
    tab = torch.zeros(5, S.SN_FIELDS, dtype=torch.int64)
    for b, i in enumerate(ins):
        tab[rows[b], 0], tab[rows[b], 3], tab[rows[b], 4], tab[rows[b], 8] = poffs[b], i["out"], inn, coffs[b]
    row0, r = [], 0
    for i in ins:
        row0.append(r)
        r += i["out"]
    gst = torch.cat([i["gsn"] for i in ins])
    dev = dict(tab=_dev(tab), layers=torch.tensor([rows[b] for b in range(4)], dtype=torch.int32, device=DEV),
               row0=torch.tensor(row0, dtype=torch.int64, device=DEV), gst=_dev(gst), params=_dev(params), ctx=_dev(ctx_all))

    def run(dst, out, accumulate):
        return _call("ieagan_sn_backward_stack", [out], dev["tab"], dev["layers"], dev["row0"], torch.tensor(dst, dtype=torch.int64, device=DEV), 4,
                     dev["gst"], dev["params"], dev["ctx"], out, accumulate)[0]

    flat = run([r * inn for r in row0], Out((r, inn)), 0)
    again = run([r * inn for r in row0], Out((r, inn)), 0)
    assert _same_bits(flat, again), "two calls on the same inputs differ"
    for i, r0 in zip(ins, row0):
        _check("sn_backward_stack", "dW flat", (i["out"], inn), flat[r0:r0 + i["out"]], i["ref64"][0], i["ref32"][0], BWD_TOL)
    # accumulate: the layers' gradients in reverse order, 8-float aligned with gaps, in a pre-filled arena
    sizes = [i["W"].numel() for i in ins]
    _, doffs = _flat([torch.zeros(n) for n in reversed(sizes)] + [torch.zeros(5)])
    dst = list(reversed(doffs[:4]))
    total = doffs[4] + 8
    base0 = S._randn(S._gen(26, inn), total)
    got = run(dst, Out((total,), fill=base0), 1)
    untouched = torch.ones(total, dtype=torch.bool)
    for i, o in zip(ins, dst):
        n = i["W"].numel()
        untouched[o:o + n] = False
        dW = (got[o:o + n].double() - base0[o:o + n].double()).view(i["out"], inn)
        _check("sn_backward_stack", "dW arena", (i["out"], inn), dW, i["ref64"][0], i["ref32"][0], BWD_TOL)
    assert untouched.sum() >= 8 and _same_bits(got[untouched], base0[untouched]), "the rest of the arena moved"


def test_sn_backward_stack_bad_calls():
    H = _H()
    t = torch.zeros(64, device=DEV)
    out = Out((16,), fill=1.0)
    good = [t.data_ptr()] * 4 + [1] + [t.data_ptr()] * 3 + [out.ptr(), 0, H.stream()]
    for pos in (0, 1, 2, 3, 5, 6, 7, 8):
        with pytest.raises(RuntimeError, match="sn_backward_stack: null pointer"):
            H.call("ieagan_sn_backward_stack", *[None if j == pos else a for j, a in enumerate(good)])
    torch.cuda.synchronize()
    assert torch.equal(out.check("grad"), torch.ones(16))


# =====================================================================================================
# through ops.py
# =====================================================================================================
@pytest.mark.parametrize("shape", [(79, 256), (100, 200)], ids=str)
def test_sn_through_ops(shape):
    """SNBank.run + ops.sn_backward on either side of the 20000-element switch, with colsum and bias: the Python side's view of the
    tables, its path decision and its zeroed scratch float agree with the C side."""
    import ops
    i = S.fwd_inputs(0, shape)
    r64, r32 = S.forward_ref(i["W"].double(), i["u"].double(), S.EPS_MODEL, 0), S.forward_ref(i["W"], i["u"], S.EPS_MODEL, 0)
    flat, offs = _flat([i["W"], i["u"], i["sv"]])
    flat = _dev(flat)
    out, inn = shape
    Wv, uv, svv = flat[:out * inn].view(out, inn), flat[offs[1]:offs[1] + out], flat[offs[2]:offs[2] + 1]
    rec = ops.SNBank(flat, [("l", ops.KIND_PLAIN, Wv, uv, svv)]).run(True, S.EPS_MODEL)["l"]
    torch.cuda.synchronize()
    ctx = rec.ctx.cpu()
    sigma, u_new, _, v, _ = S.ctx_unpack(ctx, out, inn)
    _check("SNBank.run", "sigma", shape, sigma, r64["sigma"], r32["sigma"], FWD_TOL)
    _check("SNBank.run", "u", shape, uv.cpu(), r64["u_new"], r32["u_new"], FWD_TOL)
    _check("SNBank.run", "w_plain", shape, rec.w_plain.cpu(), r64["packs"][0], r32["packs"][0], FWD_TOL)
    assert _same_bits(svv.cpu(), sigma.reshape(1)) and _same_bits(uv.cpu(), u_new)
    b = S.bwd_inputs(0, shape)                                       # its gradient and column sums; the ctx record is the kernel's own
    b["ctx"] = torch.cat([ctx, torch.zeros(S.ctx_size(out, inn) - ctx.numel())])
    ref64, ref32 = S.backward_ref(b, 0, torch.float64), S.backward_ref(b, 0, torch.float32)
    bias = torch.zeros(out, device=DEV)
    dW, dbias = ops.sn_backward(_dev(b["gsn"]), Wv, rec, colsum=_dev(b["colsum"]).view(S.STAT_REPL, out), bias=bias)
    torch.cuda.synchronize()
    _check("ops.sn_backward", "dW", shape, dW.cpu(), ref64[0], ref32[0], BWD_TOL)
    _check("ops.sn_backward", "dbias", shape, dbias.cpu(), ref64[1], ref32[1], BWD_TOL)


def test_sn_pass_scratch_and_flush():
    """The path every training step takes: inside a backward pass the weight-gradient kernels get views of the pass's scratch arena
    (``sn_scratch``), ``sn_backward`` defers, and ``SNPass.flush`` (an autograd-engine callback) maps all layers into the flat gradient
    arena with ONE batched call, through the tables of ``SNBank._plan_backward``."""
    import layers, model, ops
    from arena import Arena
    specs = [(1, (37, 5, 9), True), (1, (64, 32, 1), False), (2, (37,), True)]
    ins = [_bwd(k, s) for k, s, _ in specs]
    shapes = [S.weight_shape(k, s) for k, s, _ in specs]
    net = torch.nn.Sequential(*[layers.SNConv2d(ws[1], ws[0], ws[2], padding=ws[2] // 2, bias=hb) for ws, (_, _, hb) in zip(shapes, specs)]).to(DEV)
    with torch.no_grad():
        for m, (k, s, _) in zip(net, specs):
            f = S.fwd_inputs(k, s)
            m.weight.copy_(f["W"])
            m.u0.copy_(f["u"][None])
    ar = Arena(net)
    grad0 = S._randn(S._gen(27), ar.attach_grads().numel())
    ar.grad.copy_(grad0)
    names = [n for n, _ in model._sn_children(net, "")]
    bank = ops.SNBank(ar.flat, [(n, m._sn_kind, m.weight, m.u0, m.sv0) for n, m in model._sn_children(net, "")], owner=ar, biases=model._sn_biases(net))
    recs = bank.run(False, S.EPS_MODEL)

    class Fill(torch.autograd.Function):                              # stands for the weight-gradient kernels of a backward pass
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            for n, i, (_, _, hb) in zip(names, ins, specs):
                ops.sn_scratch(recs[n], "w", i["gsn"].shape, DEV).copy_(i["dev"]["gsn"])
                if hb:
                    ops.sn_scratch(recs[n], "b", (S.STAT_REPL, i["nb"]), DEV).copy_(i["dev"]["colsum"].view(S.STAT_REPL, -1))
                assert recs[n].deferred and ops.sn_backward(None, None, recs[n]) == (None, None)
            return g

    with ops.direct_grads():
        Fill.apply(torch.zeros(1, device=DEV, requires_grad=True)).sum().backward()
    torch.cuda.synchronize()
    got, untouched = ar.grad.cpu(), torch.ones(ar.n_param, dtype=torch.bool)
    offs = {id(p): o for p, o, _ in ar.param_slices}
    for n, m, i, (kind, shape, hb) in zip(names, net, ins, specs):
        c = recs[n].ctx.cpu()                                         # the kernel's own record is the input of both sides
        j = dict(i, ctx=torch.cat([c, torch.zeros(S.ctx_size(i["out"], i["inn"]) - c.numel())]))
        ref64, ref32 = S.backward_ref(j, kind, torch.float64), S.backward_ref(j, kind, torch.float32)
        for name, p, k in (("dW", m.weight, 0),) + ((("dbias", m.bias, 1),) if hb else ()):
            o, cnt = offs[id(p)], p.numel()
            untouched[o:o + cnt] = False
            _check("SNPass.flush", name, (kind, shape), (got[o:o + cnt].double() - grad0[o:o + cnt].double()).view(ref64[k].shape), ref64[k], ref32[k], BWD_TOL)
    assert _same_bits(got[untouched], grad0[untouched]), "the rest of the gradient arena moved"
