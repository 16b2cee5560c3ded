"""Plain restatements of the small fp32 operations around the Relational Reasoning Module and the two network heads: the checker of
tests/test_small_ops_gpu.py, itself pinned against fp64 ``torch.autograd`` in tests/test_small_ops_reference.py.

Written from the formulas in the header comments of csrc/rrm_fused.hip, csrc/small_ops.hip and csrc/bn_elem.hip and from the reference
model (RRM.py:10-16, 66-109; model.py:912-935), with explicit sums instead of library layers.  Every function computes in the dtype of
its inputs: called with fp64 tensors it is the reference, called with the same values in fp32 it is the "ordered fp32 chain" yardstick
that the GPU tests print next to the kernel's error.  Nothing here imports the product package."""
import torch

L2_EPS = 1e-12      # F.normalize's clamp on the norm


def rel_err(got, ref, floor=0.0):
    """max|got - ref| / max|ref| in fp64 over ALL elements (an all-zero reference is compared absolutely).  ``floor``: a lower limit of the
    denominator, for the two outputs that are identically zero in exact arithmetic (the tangent projection of a 1-vector: embed_norm_bwd at
    D = 1, d beta of the normalised LayerNorm at K = 1) -- what fp64 leaves there is its own rounding, so the scale is that of the terms."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = max(ref.abs().max().item(), floor)
    d = (got - ref).abs().max().item()
    return d / scale if scale > 0 else d


# ---------------------------------------------------------------------------------------------------
# LayerNorm (biased variance, eps inside the root), optionally followed by F.normalize(., dim=1)
# ---------------------------------------------------------------------------------------------------
def layer_norm(x, g, b, eps=1e-5, l2norm=False):
    """-> (y, xhat, rstd):  xhat = (x - mean) * rstd,  u = xhat * g + b,  y = u  or  u / max(|u|, 1e-12)."""
    K = x.shape[1]
    mean = x.sum(1, keepdim=True) / K
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / K + eps)
    xhat = d * rstd
    u = xhat * g + b
    if l2norm:
        u = u / torch.sqrt((u * u).sum(1, keepdim=True)).clamp_min(L2_EPS)
    return u, xhat, rstd[:, 0]


def layer_norm_bwd(dy, xhat, rstd, g, l2_beta=None, dres=None):
    """-> (dx, dg, dbeta).  ``l2_beta`` (the LayerNorm's beta): the forward ended with F.normalize, ``dy`` is the gradient of the
    normalised row and is first mapped to the gradient of u = xhat * g + beta:  du = (dy - y <dy, y>) / |u|  (|u| clamped like the
    forward; below the clamp the norm is a constant and du = dy / 1e-12).  ``dres``: gradient of a residual path, added to dx."""
    K = dy.shape[1]
    du = dy
    if l2_beta is not None:
        u = xhat * g + l2_beta
        nrm = torch.sqrt((u * u).sum(1, keepdim=True))
        clamped = nrm < L2_EPS
        n = nrm.clamp_min(L2_EPS)
        proj = torch.where(clamped, torch.zeros_like(nrm), (dy * u).sum(1, keepdim=True) / (n * n))
        du = (dy - u * proj) / n
    dxh = du * g
    m1 = dxh.sum(1, keepdim=True) / K
    m2 = (dxh * xhat).sum(1, keepdim=True) / K
    dx = rstd[:, None] * (dxh - m1 - xhat * m2)
    if dres is not None:
        dx = dx + dres
    return dx, (du * xhat).sum(0), du.sum(0)


# ---------------------------------------------------------------------------------------------------
# y = [relu](LN?(x) W^T + b) [+ res]
# ---------------------------------------------------------------------------------------------------
def linear(x, w, b=None, res=None, ln_g=None, ln_b=None, relu=False, eps=1e-5):
    """-> (y, xhat, rstd, xn): ``xn`` is the GEMM input (x, or xhat * ln_g + ln_b with the LayerNorm prologue); the residual is added
    AFTER the ReLU."""
    xhat = rstd = None
    xn = x
    if ln_g is not None:
        xn, xhat, rstd = layer_norm(x, ln_g, ln_b, eps)
    y = xn @ w.t()
    if b is not None:
        y = y + b
    if relu:
        y = torch.where(y > 0, y, torch.zeros_like(y))
    if res is not None:
        y = y + res
    return y, xhat, rstd, xn


def linear_bwd(dy, w, xn=None, xhat=None, ln_g=None, ln_b=None, ymask=None):
    """-> (dx, dw, db) with dy' = dy where ``ymask`` > 0 (the forward's post-ReLU output), else 0:  dx = dy' W (the gradient of the GEMM
    input: of the LayerNorm OUTPUT in the prologue form),  dw = dy'^T xn,  db = column sums of dy'.  ``xn`` None: xhat * ln_g + ln_b."""
    if xn is None:
        xn = xhat * ln_g + ln_b
    g = dy if ymask is None else torch.where(ymask > 0, dy, torch.zeros_like(dy))
    return g @ w, g.t() @ xn, g.sum(0)


# ---------------------------------------------------------------------------------------------------
# class proxies: F.normalize(F.embedding(y, W), dim=1)
# ---------------------------------------------------------------------------------------------------
def embed_norm(y, w):
    """-> (p, inv):  p[m] = W[y[m]] * inv[m],  inv[m] = 1 / max(|W[y[m]]|, 1e-12)."""
    rows = torch.stack([w[int(c)] for c in y])
    inv = 1.0 / torch.sqrt((rows * rows).sum(1)).clamp_min(L2_EPS)
    return rows * inv[:, None], inv


def embed_norm_bwd(y, p, inv, dp, classes):
    """-> dW [classes, D]:  dW[y[m]] += (dp[m] - p[m] <dp[m], p[m]>) * inv[m]  (a scatter-add over the rows)."""
    dw = torch.zeros(classes, dp.shape[1], dtype=dp.dtype)
    row = (dp - p * (dp * p).sum(1, keepdim=True)) * inv[:, None]
    for m, c in enumerate(y):
        dw[int(c)] += row[m]
    return dw


# ---------------------------------------------------------------------------------------------------
# attention core on the packed projection: token row = [head][q | k | v][hd]
# ---------------------------------------------------------------------------------------------------
def _split_qkv(qkv, heads):
    B, S, E3 = qkv.shape
    hd = E3 // (3 * heads)
    t = qkv.reshape(B, S, heads, 3, hd).permute(3, 0, 2, 1, 4)      # [3][B][H][S][hd]
    return t[0], t[1], t[2], hd


def attention(qkv, heads):
    """-> (out [B, S, H * hd], att [B, H, S, S]):  att = softmax_j(q_i . k_j / sqrt(hd)),  out_i = sum_j att_ij v_j."""
    q, k, v, hd = _split_qkv(qkv, heads)
    B, S = qkv.shape[:2]
    s = torch.einsum("bhid,bhjd->bhij", q, k) / (hd ** 0.5)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    att = e / e.sum(-1, keepdim=True)
    out = torch.einsum("bhij,bhjd->bhid", att, v)
    return out.permute(0, 2, 1, 3).reshape(B, S, heads * hd), att


def attention_bwd(qkv, att, dout, heads):
    """-> dqkv:  dv_j = sum_i att_ij do_i;  da_ij = do_i . v_j;  ds_ij = att_ij (da_ij - sum_l att_il da_il) / sqrt(hd);
    dq_i = sum_j ds_ij k_j;  dk_j = sum_i ds_ij q_i."""
    q, k, v, hd = _split_qkv(qkv, heads)
    B, S = qkv.shape[:2]
    do = dout.reshape(B, S, heads, hd).permute(0, 2, 1, 3)
    da = torch.einsum("bhid,bhjd->bhij", do, v)
    ds = att * (da - (att * da).sum(-1, keepdim=True)) / (hd ** 0.5)
    dq = torch.einsum("bhij,bhjd->bhid", ds, k)
    dk = torch.einsum("bhij,bhid->bhjd", ds, q)
    dv = torch.einsum("bhij,bhid->bhjd", att, do)
    return torch.stack([dq, dk, dv], 0).permute(1, 3, 2, 0, 4).reshape(B, S, heads * 3 * hd)


# ---------------------------------------------------------------------------------------------------
# glue on [N, HW, C] / [N, H, W, C] maps
# ---------------------------------------------------------------------------------------------------
def relu_sum_pool(x):
    """[N, HW, C] -> [N, C]:  sum over the pixels of max(x, 0)."""
    return torch.where(x > 0, x, torch.zeros_like(x)).sum(1)


def relu_sum_pool_bwd(x, dh):
    """-> dx [N, HW, C] = dh[n, c] where x > 0, else 0 (so +0.0 and -0.0 both get 0)."""
    return torch.where(x > 0, dh[:, None, :].expand_as(x), torch.zeros_like(x))


def res_bwd(g, Cr, Ca, mode, Hr, Wr):
    """Gradient of a residual operand that lived at another resolution.  g [N, H, W, Cg] -> dr [N, Hr, Wr, Cr]: channels [0, Ca) are
    the sum of the 2x2 block of g (mode 1: H = 2 Hr) or 0.25 * the covering pixel of g (mode 2: H = Hr / 2); channels [Ca, Cr) are 0."""
    N = g.shape[0]
    dr = torch.zeros(N, Hr, Wr, Cr, dtype=g.dtype)
    a = g[..., :Ca]
    if mode == 1:
        dr[..., :Ca] = a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
    else:
        for dy in (0, 1):
            for dx in (0, 1):
                dr[:, dy::2, dx::2, :Ca] = 0.25 * a
    return dr


def channel_stats(x):
    """[..., C] -> [2, C]: per-channel sum and sum of squares."""
    x2 = x.reshape(-1, x.shape[-1])
    return torch.stack([x2.sum(0), (x2 * x2).sum(0)])


# ---------------------------------------------------------------------------------------------------
# the case lists and their inputs (fp32 CPU tensors, seeded by the shape), shared by the CPU test of this module and the GPU tests
# ---------------------------------------------------------------------------------------------------
# (M, K, N, LayerNorm prologue, ReLU, bias, residual)
SLIN_FWD_CASES = [
    (40, 128, 384, True, False, True, False),      # the RRM qkv projection
    (33, 36, 130, True, True, True, False),        # K16 = 48 zero padding, ragged last m-tile, a 2-column n-tile, waves with n0 >= N
    (5, 4, 1, False, False, True, False),          # minimum K, N = 1
    (16, 132, 64, False, False, False, True),      # 9 k-steps: one batch of 8 and a remainder
    (160, 1536, 72, True, True, False, True),      # the 6 x 256 staging limit of gamma / beta
    (3, 1540, 20, True, False, False, False),      # the K > 1536 tail loop, K16 != K
    (17, 2048, 16, True, False, False, False),     # the entry's K limit: 147 712 B of dynamic LDS
    (17, 2048, 16, False, False, True, False),     # ... and without the prologue
]
# (M, K, N, LayerNorm form of the GEMM input, ReLU mask, outputs, dx_zeroed)
SLIN_BWD_CASES = [
    (40, 128, 384, True, False, "xwb", 0),
    (33, 36, 130, True, True, "xwb", 0),           # ragged N (guarded columns), ragged k-tile
    (5, 4, 1, False, False, "xwb", 0),
    (41, 64, 48, True, True, "xwb", 0),            # N % 16 == 0 with a masked remainder batch of 3 steps
    (19, 132, 2560, False, False, "xwb", 1),       # 5 split ranges, float atomics into the zeroed dX
    (19, 132, 2560, False, False, "xwb", 0),       # the same reduction as one range of 160 steps
    (19, 132, 2064, False, False, "xwb", 1),       # the last range is a single 16-column step
    (19, 132, 2048, False, True, "xwb", 1),        # the split threshold itself: 4 whole ranges, masked
    (40, 128, 70, False, False, "b", 0),
    (40, 128, 70, True, True, "b", 0),             # db only, LayerNorm form: no GEMM input is read
    (40, 128, 70, False, False, "x", 0),
    (40, 128, 70, True, False, "wb", 0),
    (40, 128, 70, False, False, "w", 0),
    (1, 64, 32, False, False, "xwb", 0),
    (3, 64, 32, True, True, "xwb", 0),
    (160, 64, 32, False, False, "xwb", 0),
]
LN_CASES = [(M, K, l2) for K in (1, 3, 255, 256, 257, 1024) for M in (1, 40) for l2 in (False, True)] + [(40, 257, "zero")]
EMBED_CASES = [(D, kind) for D in (1, 130, 1024) for kind in ("distinct", "same", "zero_row")]
EMBED_M, EMBED_CLASSES, EMBED_ZERO_CLASS = 40, 48, 5
# (B, S, heads, hd, scale of qkv)
ATTENTION_CASES = [
    (4, 40, 2, 64, 1),
    (2, 1, 2, 64, 1),
    (2, 37, 2, 64, 1),                             # the j + 4 <= S tail
    (1, 64, 2, 64, 1),                             # S = SMAX: 16 staged affinities per thread
    (3, 7, 2, 6, 1),                               # hd % 4 != 0: the scalar kernels
    (1, 40, 4, 128, 30),                           # softmax with large logits
    (1, 59, 1, 128, 1),                            # the largest LDS footprint the entries accept: 152 456 B in the backward
]
CONST_ROW = 1.5     # the all-constant input row: sums of <= 2048 copies and their mean are exact in fp32, so xhat is exactly 0


def _gen(*key):
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k)) % (1 << 31)
    return torch.Generator().manual_seed(seed)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


def grid(gen, *shape):
    """Multiples of 1/8 in [-8, 8]: exact in bf16, and fp32 sums of thousands of them (or of their squares) have one right answer."""
    return torch.randint(-64, 65, shape, generator=gen).float() / 8


def slin_fwd_inputs(M, K, N, ln, relu, bias, res):
    g = _gen(1, M, K, N)
    d = dict(x=_randn(g, M, K), w=_randn(g, N, K) / K ** 0.5, b=_randn(g, N) if bias else None, res=_randn(g, M, N) if res else None,
             ln_g=1 + 0.5 * _randn(g, K) if ln else None, ln_b=0.5 * _randn(g, K) if ln else None, relu=relu, eps=1e-5)
    if ln and M >= 2:
        d["x"][1] = CONST_ROW
    return d


def slin_bwd_inputs(M, K, N, ln, mask):
    """The mask is a post-ReLU forward output (fp32, many exact zeros) with some elements overwritten by negative values and -0.0."""
    g = _gen(2, M, K, N)
    d = dict(dy=_randn(g, M, N), w=_randn(g, N, K) / K ** 0.5, xn=None, xhat=None, ln_g=None, ln_b=None, ymask=None)
    if ln:
        d.update(xhat=_randn(g, M, K), ln_g=1 + 0.5 * _randn(g, K), ln_b=0.5 * _randn(g, K))
        xn = d["xhat"] * d["ln_g"] + d["ln_b"]
    else:
        xn = d["xn"] = _randn(g, M, K)
    if mask:
        y = torch.relu(xn @ d["w"].t() + _randn(g, N))
        y.view(-1)[::7] = -1.0
        y.view(-1)[3::11] = -0.0
        d["ymask"] = y
    return d


def ln_inputs(M, K, l2):
    """x (row 1 constant when there is one), gamma, beta, dy, dres and the accumulators' previous contents.  l2 == "zero": gamma = beta = 0,
    so every u = xhat * gamma + beta is exactly 0 and F.normalize's clamp decides the result."""
    g = _gen(3, M, K, int(bool(l2)))
    d = dict(x=2 * _randn(g, M, K) + 0.3, g=1 + 0.5 * _randn(g, K), b=0.5 * _randn(g, K), dy=_randn(g, M, K), dres=_randn(g, M, K),
             dg0=_randn(g, K), dbeta0=_randn(g, K), eps=1e-5)
    if M >= 2:
        d["x"][1] = CONST_ROW
    if l2 == "zero":
        d["g"].zero_()
        d["b"].zero_()
    return d


def embed_inputs(D, kind):
    g = _gen(4, D)
    w = _randn(g, EMBED_CLASSES, D)
    w[EMBED_ZERO_CLASS] = 0
    live = [c for c in range(EMBED_CLASSES) if c != EMBED_ZERO_CLASS]
    if kind == "distinct":
        y = torch.tensor(live[:EMBED_M])
    elif kind == "same":
        y = torch.full((EMBED_M,), 7)
    else:
        y = torch.tensor([(EMBED_ZERO_CLASS if m % 4 == 0 else live[m % 9]) for m in range(EMBED_M)])
    return dict(y=y.long(), w=w, dp=_randn(g, EMBED_M, D), dw0=_randn(g, EMBED_CLASSES, D))


def attention_inputs(B, S, heads, hd, scale):
    """scale == 1: normal values.  scale > 1 (large logits): multiples of scale / 8 with |value| <= 2 scale, whose inner products are exact in
    fp32 -- the rounding of an fp32 inner product grows with the logit (std ~ scale^2 here), so with inexact logits no fp32 softmax holds a
    fixed bound on a row whose two largest logits are close; what the case is about is the max-subtraction, and that it still exercises."""
    g = _gen(5, B, S, heads, hd)
    shape = (B, S, heads * 3 * hd)
    qkv = _randn(g, *shape) if scale == 1 else torch.randint(-16, 17, shape, generator=g).float() * (scale / 8)
    return dict(qkv=qkv, dout=_randn(g, B, S, heads * hd))
