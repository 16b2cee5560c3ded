"""Plain restatement of the batched spectral normalisation of csrc/sn.hip: the checker of tests/test_sn_gpu.py, itself pinned against fp64
``torch.autograd`` and ``F.normalize`` in tests/test_sn_reference.py.

Written from the header comments of csrc/sn.hip (the three phases, the ctx record, the consumer layouts of the four kinds, the tables of
the batched backward), not from its code.  Every function computes in the dtype of its inputs: called with fp64 tensors it is the
reference, called with the same values in fp32 it is the "ordered fp32 chain" yardstick that the GPU tests print next to the kernel's
error.  Nothing here imports the product package.

Shapes.  A weight is given in the parameter's own shape: kind 0 ``[out, in]``; kind 1 ``[Cout, Cin, k, k]`` (taps = k * k, in = Cin * taps);
kind 2 ``[C, 1, 3, 3]`` (out = C, in = 9); kind 3 ``[1, C, 3, 3]`` (out = 1, in = 9 C).  Its matrix form is ``W.reshape(out, in)``."""
import torch

from small_ops_reference import _gen, _randn, rel_err      # noqa: F401  (rel_err: the error measure of both suites)

STAT_REPL = 32      # replicas of a bias column-sum buffer (csrc/common.h)
SN_FIELDS = 16      # int64 fields per row of the layer table
SNB_FIELDS = 12     # int64 fields per row of the batched-backward table
SNB_CHUNK = 2048    # elements per work item of the batched backward
FUSED_MAX = 20000   # layers of up to this many elements take the one-block backward


def kpad_of(k):
    """Row length of a bf16 conv pack: the next multiple of 32."""
    return (k + 31) // 32 * 32


def dims(W, kind):
    """-> (out, in, taps, cin) of a weight in its parameter shape."""
    out = W.shape[0]
    inn = W.numel() // out
    taps = W.shape[-1] * W.shape[-2] if W.dim() == 4 else 1
    cin = W.shape[1] if W.dim() == 4 else inn
    return out, inn, taps, cin


# ---------------------------------------------------------------------------------------------------
# forward: one power iteration
# ---------------------------------------------------------------------------------------------------
def power_iteration(W2d, u, eps):
    """-> (sigma, u_new, v_raw, v, t):  v_raw = u W,  v = v_raw / max(|v_raw|, eps),  t = W v,  tt = |t|^2,
    sigma = tt / max(sqrt(tt), eps),  u_new = t / max(sqrt(tt), eps)."""
    v_raw = (u[:, None] * W2d).sum(0)
    v = v_raw / torch.sqrt((v_raw * v_raw).sum()).clamp_min(eps)
    t = (W2d * v[None, :]).sum(1)
    tt = (t * t).sum()
    un = torch.sqrt(tt).clamp_min(eps)
    return tt / un, t / un, v_raw, v, t


# ---------------------------------------------------------------------------------------------------
# consumer layouts
# ---------------------------------------------------------------------------------------------------
def to_consumer(P, kind):
    """A tensor in the parameter's shape -> the layout in which the consumer of the normalised weight reads it (and hands back its
    gradient): kind 0 [out][in];  kind 1 [out][kpad] with k = tap * cin + c and zeros in k >= taps * cin;  kinds 2, 3 [9][C]."""
    out, inn, taps, cin = dims(P, kind)
    if kind == 0:
        return P.reshape(out, inn)
    if kind == 1:
        r = torch.zeros(out, kpad_of(taps * cin), dtype=P.dtype)
        r[:, :taps * cin] = P.reshape(out, cin, taps).permute(0, 2, 1).reshape(out, taps * cin)
        return r
    C = out if kind == 2 else cin
    return P.reshape(C, 9).t().contiguous()


def from_consumer(g, shape, kind):
    """The inverse of ``to_consumer`` (padding columns are dropped unread)."""
    shape = tuple(shape)
    out = shape[0]
    if kind == 0:
        return g.reshape(shape)
    if kind == 1:
        cin, taps = shape[1], shape[2] * shape[3]
        return g[:, :taps * cin].reshape(out, taps, cin).permute(0, 2, 1).reshape(shape)
    return g.reshape(9, -1).t().reshape(shape)


def dgrad_pack(P):
    """Kind 1: [cin][kpad2] with k' = (taps - 1 - tap) * out + o, zeros in k' >= taps * out (the flipped, transposed filter)."""
    out, inn, taps, cin = dims(P, 1)
    r = torch.zeros(cin, kpad_of(taps * out), dtype=P.dtype)
    r[:, :taps * out] = P.reshape(out, cin, taps).flip(2).permute(1, 2, 0).reshape(cin, taps * out)
    return r


def normalised(W, sigma, kind):
    """W / sigma in the consumer's layout(s): a tensor, or for kind 1 the pair (forward pack, dgrad pack) -- unrounded."""
    Wn = W / sigma
    return (to_consumer(Wn, 1), dgrad_pack(Wn)) if kind == 1 else to_consumer(Wn, kind)


# ---------------------------------------------------------------------------------------------------
# backward through W / sigma with u', v constant
# ---------------------------------------------------------------------------------------------------
def sn_backward(gsn, W, sigma, u_new, v, kind):
    """``gsn`` in the consumer's layout -> dW = g / sigma - (<g, W> / sigma^2) u'^T v in the parameter's shape."""
    g = from_consumer(gsn, W.shape, kind)
    inner = (g * W).sum()
    return g / sigma - (inner / (sigma * sigma)) * (u_new[:, None] * v[None, :]).reshape(W.shape)


def bias_fold(colsum, nb):
    """[STAT_REPL * nb] replicated column sums -> [nb]."""
    return colsum.reshape(STAT_REPL, nb).sum(0)


# ---------------------------------------------------------------------------------------------------
# the ctx record of one layer: [0] sigma, [8, 8+out) u', then v_raw [in], v [in], t [out]; rounded up to 8 floats
# ---------------------------------------------------------------------------------------------------
def ctx_size(out, inn):
    return (8 + 2 * out + 2 * inn + 7) // 8 * 8


def ctx_pack(out, inn, sigma, u_new, v_raw, v, t, fill=0.0):
    c = torch.full((ctx_size(out, inn),), fill, dtype=torch.float32)
    c[0] = float(sigma)
    c[8:8 + out] = u_new.float()
    c[8 + out:8 + out + inn] = v_raw.float()
    c[8 + out + inn:8 + out + 2 * inn] = v.float()
    c[8 + out + 2 * inn:8 + 2 * out + 2 * inn] = t.float()
    return c


def ctx_unpack(c, out, inn):
    """-> (sigma, u_new, v_raw, v, t) views of one record."""
    return c[0], c[8:8 + out], c[8 + out:8 + out + inn], c[8 + out + inn:8 + out + 2 * inn], c[8 + out + 2 * inn:8 + 2 * out + 2 * inn]


def ctx_unwritten(out, inn):
    """Bool mask over one record: the slots no phase writes ([1, 8) and the alignment tail)."""
    m = torch.zeros(ctx_size(out, inn), dtype=torch.bool)
    m[1:8] = True
    m[8 + 2 * out + 2 * inn:] = True
    return m


# ---------------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------------
def bf16_neighbours(ref64):
    """-> (rne, below, above) as fp32 tensors holding bf16 values: the fp64 reference rounded to nearest-even in ONE rounding, and the bf16
    values one step nearer to / farther from zero.  (Integer arithmetic on the bit patterns: no double rounding through fp32.)"""
    a = ref64.double().abs()
    m = (a.float().view(torch.int32) >> 16).long()                  # bf16 magnitude bits near |ref|

    def val(bits):
        return (bits.clamp_min(0).int() << 16).view(torch.float32).double()

    cand = torch.stack([m - 1, m, m + 1]).clamp_min(0)
    dist = (val(cand) - a).abs()
    best = dist.min(0).values
    tie = dist == best                                              # nearest; of two equally near ones the even pattern
    score = torch.where(tie, (cand & 1), torch.full_like(cand, 2))
    pick = score.argmin(0, keepdim=True)
    r = cand.gather(0, pick)[0]
    sign = torch.where(torch.signbit(ref64.double()), -1.0, 1.0)
    return tuple((val(b) * sign).float() for b in (r, r - 1, r + 1))


def bf16_bits_value(bits16):
    """int16 bit patterns -> fp32 values."""
    return (bits16.int() << 16).view(torch.float32)


# ---------------------------------------------------------------------------------------------------
# case lists and inputs (fp32 CPU tensors, seeded by the shape), shared by the CPU test of this module and the GPU tests
# ---------------------------------------------------------------------------------------------------
# (kind, shape): kind 0 (out, in); kind 1 (Cout, Cin, taps); kinds 2, 3 (C,)
FWD_CASES = [
    (0, (1, 3)),            # fewer elements than blocks share the packing loop; a single row
    (0, (33, 7)),           # second row chunk of one row (three waves idle in phase 2); in < 32
    (0, (37, 385)),         # 5-row remainder of the 8-row batches; in = 6 * 64 + 1
    (0, (20, 1001)),        # three 384-column rounds in phase 2, four 256-strides in phase 1, ragged 32-column tile in phase 1b
    (0, (257, 33)),         # 9 row chunks: the 8-way split of phase 1b with empty shares
    (0, (290, 40)),         # 10 row chunks: ... with a short share
    (1, (48, 32, 9)),       # no padding in either pack
    (1, (37, 5, 9)),        # kpad 64 > 45, kpad2 352 > 333, ragged last row chunk in the dgrad pack
    (1, (70, 3, 1)),        # kpad 32 > 3, kpad2 96 > 70, three row chunks
    (1, (16, 64, 1)),       # 1x1, exact
    (2, (16,)), (2, (37,)),  # [C][1][3][3] -> [9][C], one and two row chunks
    (3, (16,)), (3, (37,)),  # [1][C][3][3] -> [9][C], out = 1
]
MODE_CASES = [(0, (37, 385)), (1, (37, 5, 9))]                      # eps = 1e-6, training = 0, weight * 1e-9 at eps = 1e-6
STACK_LAYERS = [(0, (24, 20)), (0, (40, 20)), (0, (8, 20))]         # the stacked kind-0 layers of the all-layers bank
EPS_MODEL = 1e-12
EPS_BIG = 1e-6
TINY = 1e-9

# every forward shape on the path its size selects: (20, 1001) has 20020 elements and takes the multi-block one
BWD_FUSED_CASES = [c for c in FWD_CASES if c != (0, (20, 1001))] + [(0, (100, 200))]      # ... and exactly 20000 elements
BWD_LARGE_CASES = [
    (0, (20, 1001)),
    (0, (79, 256)),         # the smallest such shape above 20000
    (0, (20001, 1)),
    (0, (300, 70)),         # a two-block bias fold
    (0, (1030, 513)),       # grid-stride rounds beyond 512 blocks x 4 in flight, with a remainder
    (1, (64, 40, 9)),
]
# the five layers of the batched-backward call: (kind, shape, has bias)
BATCHED_LAYERS = [
    (1, (48, 32, 9), True),     # 6.75 chunks of 2048
    (1, (64, 32, 1), False),    # exactly one chunk
    (1, (37, 5, 9), True),      # a partial chunk, padded kpad
    (2, (37,), True),
    (3, (16,), False),          # colsum = -1
]
STACK_BWD_OUTS = (1, 24, 40, 130)
STACK_BWD_INS = (20, 128)
GSN_PAD = 7.0               # what the padding columns of a kind-1 gradient hold: never read into a result


def weight_shape(kind, shape):
    if kind == 0:
        return tuple(shape)
    if kind == 1:
        k = {9: 3, 1: 1}[shape[2]]
        return (shape[0], shape[1], k, k)
    return (shape[0], 1, 3, 3) if kind == 2 else (1, shape[0], 3, 3)


def fwd_inputs(kind, shape, scale=1.0):
    """-> W (parameter shape, entries ~ N(0, 1 / in) * scale), u [out], sv [1]."""
    ws = weight_shape(kind, shape)
    g = _gen(21, kind, *shape)
    out = ws[0]
    inn = 1
    for s in ws[1:]:
        inn *= s
    return dict(W=_randn(g, *ws) * (scale / inn ** 0.5), u=_randn(g, out), sv=torch.ones(1))


def forward_ref(W, u, eps, kind):
    """Everything the forward leaves behind, in the dtype of ``W``: dict(sigma, u_new, v_raw, v, t, packs = tuple of consumer layouts)."""
    out, inn, taps, cin = dims(W, kind)
    sigma, u_new, v_raw, v, t = power_iteration(W.reshape(out, inn), u, eps)
    p = normalised(W, sigma, kind)
    return dict(sigma=sigma, u_new=u_new, v_raw=v_raw, v=v, t=t, packs=p if kind == 1 else (p,))


def bwd_inputs(kind, shape, eps=EPS_MODEL):
    """Inputs of one backward call: the forward's W, the fp32 ctx record of the fp64 forward, the consumer-layout gradient (kind 1: its
    padding columns hold GSN_PAD), previous contents of dW / dbias for the accumulating forms and replicated bias column sums."""
    i = fwd_inputs(kind, shape)
    W = i["W"]
    out, inn, taps, cin = dims(W, kind)
    f = forward_ref(W.double(), i["u"].double(), eps, kind)
    ctx = ctx_pack(out, inn, f["sigma"], f["u_new"], f["v_raw"], f["v"], f["t"])
    g = _gen(22, kind, *shape)
    gsn = to_consumer(_randn(g, *W.shape), kind).clone()
    if kind == 1:
        gsn[:, taps * cin:] = GSN_PAD
    nb = 1 if kind == 3 else out
    return dict(W=W, ctx=ctx, gsn=gsn, dw0=_randn(g, *W.shape), colsum=_randn(g, STAT_REPL * nb), db0=_randn(g, nb), nb=nb,
                out=out, inn=inn, taps=taps, cin=cin, kpad=kpad_of(taps * cin) if kind == 1 else 0)


def backward_ref(i, kind, dtype):
    """(dW, dbias fold) of ``bwd_inputs`` in ``dtype``; the fp32 ctx record is an input of both sides."""
    sigma, u_new, _, v, _ = ctx_unpack(i["ctx"].to(dtype), i["out"], i["inn"])
    return sn_backward(i["gsn"].to(dtype), i["W"].to(dtype), sigma, u_new, v, kind), bias_fold(i["colsum"].to(dtype), i["nb"])


def stack_bwd_inputs(inn):
    """The layers of one stacked-backward call: a list of ``bwd_inputs``-like dicts (kind 0, the same ``in``)."""
    return [bwd_inputs(0, (o, inn)) for o in STACK_BWD_OUTS]
