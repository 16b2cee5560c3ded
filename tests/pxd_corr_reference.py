"""NumPy restatement of the intra-event correlations, the checker of ``utils.pxd_region_counts``, ``utils.PXDCorrelations`` and
``utils.pxd_correlation_distance`` (tests only).  Plain on purpose: dense images, the O(E^2) definition of the ranks, Python integers.

* digits: the pixel rule of ``utils.pxd_digits`` on the dense images -- ``q = uint8(min(max(v, 0), 255)) > 0 and v >= threshold``;
* regions: a digit at row ``r``, column ``c`` of image ``n`` is event ``n // S``, sensor ``n % S``, ``ru = r * RU // H``, ``rv = c * RV // W``
  (integers), column ``(s * RU + ru) * RV + rv`` of ``R = S * RU * RV``;
* ``rank2[e, k] = 2 * #{e' : x[e', k] < x[e, k]} + #{e' : x[e', k] == x[e, k]} + 1``;
* moments ``n``, ``sum[k]``, ``gram[i, j]`` of a table in Python integers (object arrays);
* ``cov_ij = n * G_ij - s_i * s_j`` in integers, ``rho_ij = float(cov_ij) / sqrt(float(var_i) * float(var_j))``, NaN when a variance is 0
  or ``n < 2``.
"""
import numpy as np


def digit_mask(images, threshold=0.0):
    v = np.asarray(images)
    if v.dtype == np.uint8:
        return (v > 0) & (v.astype(np.float32) >= np.float32(threshold))
    q = np.clip(np.nan_to_num(v.astype(np.float32), nan=0.0), 0, 255).astype(np.uint8)
    return (q > 0) & (v >= np.float32(threshold))


def region_counts(images, regions, n_sensors, threshold=0.0):
    """int32 ``[E, R]`` of the dense ``images [N, H, W]``."""
    (N, H, W), (RU, RV), S = np.shape(images), regions, n_sensors
    assert N % S == 0 and 1 <= RU <= H and 1 <= RV <= W
    x = np.zeros((N // S, S * RU * RV), np.int32)
    for n, r, c in zip(*np.nonzero(digit_mask(images, threshold))):
        x[n // S, ((n % S) * RU + (r * RU) // H) * RV + (c * RV) // W] += 1
    return x


def region_areas(H, W, regions):
    """Pixels of every region of one sensor, ``[RU * RV]``: ``#{r : r * RU // H == ru} * #{c : c * RV // W == rv}``."""
    RU, RV = regions
    rows = [sum(1 for r in range(H) if r * RU // H == ru) for ru in range(RU)]
    cols = [sum(1 for c in range(W) if c * RV // W == rv) for rv in range(RV)]
    return np.array([a * b for a in rows for b in cols], np.int32)


def rank2(x):
    x = np.asarray(x)
    out = np.empty(x.shape, np.int32)
    for e in range(x.shape[0]):
        out[e] = 2 * (x < x[e]).sum(0) + (x == x[e]).sum(0) + 1
    return out


def moments(x):
    """``(n, sum [R], gram [R, R])`` of a table ``[E, R]`` in Python integers."""
    xo = np.asarray(x).astype(object)
    R = xo.shape[1]
    gram = xo.T.dot(xo) if xo.shape[0] else np.zeros((R, R), object)
    return int(xo.shape[0]), xo.sum(0) if xo.shape[0] else np.zeros(R, object), gram


def coefficients(n, total, gram):
    R = len(total)
    rho = np.full((R, R), np.nan, np.float64)
    var = [int(n) * int(gram[i][i]) - int(total[i]) * int(total[i]) for i in range(R)]
    for i in range(R):
        for j in range(R):
            if n >= 2 and var[i] != 0 and var[j] != 0:
                cov = int(n) * int(gram[i][j]) - int(total[i]) * int(total[j])
                rho[i, j] = np.float64(float(cov)) / np.sqrt(np.float64(float(var[i])) * np.float64(float(var[j])))
    return rho


def result(x, regions, shape):
    """What ``PXDCorrelations.result()`` returns for the accumulated table ``x [E, R]``."""
    x = np.asarray(x, np.int32)
    n, s, g = moments(x)
    r2 = rank2(x)
    _, rs, rg = moments(r2)
    return dict(gram=g.astype(np.int64), sum=s.astype(np.int64), rank_gram=rg.astype(np.int64), rank_sum=rs.astype(np.int64), counts=x, n_events=n,
                regions=tuple(regions), shape=tuple(shape), pearson=coefficients(n, s, g), spearman=coefficients(n, rs, rg), rank2=r2)


def distance(real, fake):
    for k in ("regions", "shape"):
        if tuple(real[k]) != tuple(fake[k]):
            raise ValueError(k)
    if np.shape(real["spearman"]) != np.shape(fake["spearman"]):
        raise ValueError("columns")
    R = np.shape(real["spearman"])[0]
    pairs = [(i, j) for i in range(R) for j in range(i + 1, R)]

    def diffs(name):
        use = [(i, j) for i, j in pairs if not np.isnan(real[name][i, j])]
        r = np.array([real[name][i, j] for i, j in use], np.float64)
        f = np.array([0.0 if np.isnan(fake[name][i, j]) else fake[name][i, j] for i, j in use], np.float64)
        return r, f
    (pr, pf), (sr, sf) = diffs("pearson"), diffs("spearman")
    nan = float("nan")
    return dict(pearson_rms=float(np.sqrt(np.mean((pf - pr) ** 2))) if pr.size else nan,
                spearman_rms=float(np.sqrt(np.mean((sf - sr) ** 2))) if sr.size else nan,
                spearman_max_abs=float(np.abs(sf - sr).max()) if sr.size else nan,
                spearman_strength_err=float(np.abs(sf).mean() - np.abs(sr).mean()) if sr.size else nan)


def planted(E, S, H, W, shared, regions=(1, 1), seed=0):
    """Deterministic uint8 events ``[E * S, H, W]`` (``S >= 3``, ``E >= 3``).  Every sensor image draws ``Poisson(m * H * W / 40)`` lit pixels
    (charges 7 .. 255) with a gamma(2, 1) multiplicity ``m`` -- one per event with ``shared``, one per sensor image without: every
    single-sensor distribution is the same, the sensors of an event hang together only with ``shared``.  Planted on top: sensor 1 of event 2
    is fully lit, and the first region of the last sensor (on the grid ``regions``) holds exactly one digit in every event -- column
    ``constant_column(S, regions)`` never varies."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    x = np.zeros((E * S, H, W), np.uint8)
    for e in range(E):
        m_event = rng.gamma(2.0, 1.0)
        for s in range(S):
            m = m_event if shared else rng.gamma(2.0, 1.0)
            k = min(int(rng.poisson(m * H * W / 40.0)), H * W)
            at = rng.choice(H * W, size=k, replace=False)
            x[e * S + s].reshape(-1)[at] = rng.integers(7, 256, size=k)
    x[2 * S + 1] = rng.integers(7, 256, size=(H, W))
    RU, RV = regions
    rows = [r for r in range(H) if r * RU // H == 0]
    cols = [c for c in range(W) if c * RV // W == 0]
    for e in range(E):
        x[e * S + S - 1][np.ix_(rows, cols)] = 0
        x[e * S + S - 1, 0, 0] = 200
    return x


def constant_column(S, regions):
    return (S - 1) * regions[0] * regions[1]


# E events of S x H x W on a grid.  A: every offset unaligned, neither 13 nor 37 divides, runs of a wave's step cross region, row, image and
# event boundaries.  B: E > 64 and R > 64, neither a multiple of 64: every edge tile of the rank and Gram kernels.
SHAPES = {"A": (7, 3, 13, 37, (2, 3)), "B": (70, 40, 8, 24, (1, 2))}
THRESHOLD = 7.0
_CACHE = {}


def case(name, shared=True, seed=0):
    """``(images, counts, result)`` of the planted sample of a shape, computed once and read-only."""
    key = (name, shared, seed)
    if key not in _CACHE:
        E, S, H, W, regions = SHAPES[name]
        x = planted(E, S, H, W, shared, regions, seed)
        counts = region_counts(x, regions, S, THRESHOLD)
        for a in (x, counts):
            a.setflags(write=False)
        _CACHE[key] = (x, counts, result(counts, regions, (H, W)))
    return _CACHE[key]


def as_f32(x):
    """The uint8 images as fp32 images with the same digits at a threshold of 7: lit pixels gain a fraction (and 255 becomes 300.5, which
    the pixel rule clips), dark pixels get values that are no digit -- negative, below 1, below the threshold, NaN."""
    v = x.astype(np.float32)
    v[x > 0] += np.float32(0.5)
    v[x == 255] = np.float32(300.5)
    dark = np.nonzero(x.reshape(-1) == 0)[0]
    fill = np.array([-3.0, 0.75, 6.9375, np.nan, 0.0], np.float32)
    v.reshape(-1)[dark] = fill[np.arange(dark.size) % fill.size]
    return v
