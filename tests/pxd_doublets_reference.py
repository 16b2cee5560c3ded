"""NumPy checker of ``utils.pxd_space_points``, ``utils.pxd_doublets`` and ``utils.PXDDoubletStatistics`` (tests only), on top of the hit
checker ``pxd_hits_reference`` (which decides the hits, their order and their fp32 positions).

Space points in Python integers (object arrays): ``lu = int(rint(float32(u) * float32(16)))``, ``X_c = origin_c + ((u_axis_c * lu + v_axis_c *
lv + 2**29) >> 30)``, ``r = math.isqrt(x**2 + y**2)``.  Doublets by a plain double loop over the hits of each event: the outer loop over the
inner hits in Python, the loop over the outer hits of the event in int64 NumPy (every product is below 2**63 by the bounds that
``tests/test_pxd_doublets.py`` asserts, where this loop is also pinned against a brute force in Python ``int`` / ``fractions.Fraction``).
"""
import functools
import math

import numpy as np

import pxd_hits_reference as HR
import pxd_reference as R

COUNTERS, PARTNER_BINS, EVENT_BINS = 5, 64, 251
TILE = 256              # rows of a workgroup = records of an LDS tile of csrc/pxd_doublets.hip


def windows(dphi, z0_mm, unit_mm=5e-4):
    return int(round(math.tan(dphi) * 4096)), int(round(z0_mm / unit_mm * 16))


def isqrt_by_double(s):
    """The device's recipe: the double root, corrected by +-1 with integer tests."""
    q = int(math.sqrt(float(s)))
    q -= 1 if q * q > s else 0
    q += 1 if (q + 1) * (q + 1) <= s else 0
    return q


def space_points(sensor, u, v, counts, placement):
    """``x, y, z, r`` (int64, from Python integers), ``sensor``, ``role`` and ``offsets`` of the hits ``u`` / ``v`` (fp32, geometry units) on the
    sensors ``sensor``; ``placement``: anything with ``origin``, ``u_axis``, ``v_axis`` ``[S, 3]`` and ``layer [S]``."""
    lu = np.rint(np.asarray(u, np.float32) * np.float32(16)).astype(np.int64).astype(object)
    lv = np.rint(np.asarray(v, np.float32) * np.float32(16)).astype(np.int64).astype(object)
    o, ua, va = (np.asarray(getattr(placement, k)).astype(object)[sensor] for k in ("origin", "u_axis", "v_axis"))
    X = [[int(o[a, c]) + ((int(ua[a, c]) * int(lu[a]) + int(va[a, c]) * int(lv[a]) + 2 ** 29) >> 30) for c in range(3)] for a in range(len(sensor))]
    X = np.array(X, dtype=object).reshape(-1, 3)
    r = [math.isqrt(int(p[0]) ** 2 + int(p[1]) ** 2) for p in X]
    assert all(abs(int(c)) < 2 ** 23 for p in X for c in p)
    x, y, z = (X[:, c].astype(np.int64) for c in range(3))
    role = np.asarray(placement.layer, np.int64)[sensor]
    return dict(x=x, y=y, z=z, r=np.array(r, np.int64), sensor=np.asarray(sensor, np.int64), role=role,
                offsets=np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]), total=len(sensor))


def passes(xa, ya, za, ra, xb, yb, zb, rb, tan_q12, z0_sub):
    """The two windows for one inner hit against arrays of outer hits (int64)."""
    dot = xa * xb + ya * yb
    cross = np.abs(xa * yb - ya * xb)
    return (dot > 0) & ((cross << 12) <= tan_q12 * dot) & (rb > ra) & (np.abs(za * rb - zb * ra) <= z0_sub * (rb - ra))


def doublets(pt, pairs, tan_q12, z0_sub, n_sensors):
    """Everything of the contract of ``ieagan_pxd_doublets`` for the space points ``pt``: ``inner`` / ``outer`` (ascending), ``partners``
    per hit row, ``event_doublets``, ``total``."""
    off, S = pt["offsets"], n_sensors
    E = (len(off) - 1) // S
    pairs = np.asarray(pairs)
    inner, outer = [], []
    partners, event_doublets = np.zeros(pt["total"], np.int64), np.zeros(E, np.int64)
    for e in range(E):
        lo, hi = int(off[e * S]), int(off[(e + 1) * S])
        rows = np.arange(lo, hi)
        out_rows = rows[pt["role"][lo:hi] == 1]
        xb, yb, zb, rb, sb = (pt[k][out_rows] for k in ("x", "y", "z", "r", "sensor"))
        for a in rows[pt["role"][lo:hi] == 0]:
            ok = passes(pt["x"][a], pt["y"][a], pt["z"][a], pt["r"][a], xb, yb, zb, rb, tan_q12, z0_sub) & (pairs[pt["sensor"][a], sb] != 0)
            found = out_rows[ok]
            inner += [a] * found.size
            outer += found.tolist()
            partners[a] = found.size
            event_doublets[e] += found.size
    return dict(inner=np.array(inner, np.int64), outer=np.array(outer, np.int64), partners=partners, event_doublets=event_doublets, total=len(inner))


def event_bin(d):
    d = np.asarray(d, np.int64)
    return np.where(d < 1, 0, np.where(d < 7, 1, 2 + np.minimum(d - 7, 248)))


def tables(pt, db, layer, n_sensors):
    """The int64 table ``ieagan_pxd_doublet_stats`` adds for one batch, without the overflow word."""
    S, off = n_sensors, pt["offsets"]
    per_image = np.diff(off).reshape(-1, S)
    layer = np.asarray(layer)
    n_in, n_out = per_image[:, layer == 0].sum(1), per_image[:, layer == 1].sum(1)
    t = np.zeros(COUNTERS + S * S + PARTNER_BINS + EVENT_BINS, np.int64)
    t[:COUNTERS] = per_image.shape[0], n_in.sum(), n_out.sum(), db["total"], (n_in * n_out).sum()
    np.add.at(t[COUNTERS:COUNTERS + S * S], pt["sensor"][db["inner"]] * S + pt["sensor"][db["outer"]], 1)
    np.add.at(t[COUNTERS + S * S:COUNTERS + S * S + PARTNER_BINS], np.minimum(db["partners"][pt["role"] == 0], PARTNER_BINS - 1), 1)
    np.add.at(t[COUNTERS + S * S + PARTNER_BINS:], event_bin(db["event_doublets"]), 1)
    return t


def result(t, n_sensors):
    """A table as the part of ``PXDDoubletStatistics.result()`` that ``distance`` reads."""
    S = n_sensors
    ratio = lambda a, b: float(a) / float(b) if b > 0 else float("nan")
    return dict(doublets_per_event=ratio(t[3], t[0]), acceptance=ratio(t[3], t[4]), sensor_pairs=t[COUNTERS:COUNTERS + S * S].reshape(S, S),
                partners_spectrum=t[COUNTERS + S * S:COUNTERS + S * S + PARTNER_BINS])


def distance(real, fake):
    rel = lambda r, f: abs(f - r) / r if r == r and r > 0 and f == f else float("nan")
    w1 = lambda a, b: float(np.abs(np.cumsum(b / b.sum()) - np.cumsum(a / a.sum())).sum()) if a.sum() > 0 and b.sum() > 0 else float("nan")
    pr, pf = real["sensor_pairs"].astype(np.float64), fake["sensor_pairs"].astype(np.float64)
    return dict(doublet_rate_rel_err=rel(real["doublets_per_event"], fake["doublets_per_event"]), acceptance_rel_err=rel(real["acceptance"], fake["acceptance"]),
                partners_w1=w1(real["partners_spectrum"].astype(np.float64), fake["partners_spectrum"].astype(np.float64)),
                sensor_pair_l1=float(np.abs(pf / pf.sum() - pr / pr.sum()).sum()) if pr.sum() > 0 and pf.sum() > 0 else float("nan"))


def chain(images, geometry, placement, tan_q12, z0_sub, threshold=0.0, seed_cut=0, charge_cut=0, head_tail=3):
    """``(clusters, positions, hits, points, doublets)`` of ``images [N, H, W]`` (host); ``geometry``: anything with ``u_pitch``, ``v_pitch``,
    ``kind``."""
    images = np.asarray(images)
    N, H, W = images.shape
    S = len(geometry.kind)
    cl, pos, hits = HR.reco_hits(images, (geometry.u_pitch, geometry.v_pitch, geometry.kind), head_tail, threshold, seed_cut, charge_cut)
    sensor = cl["first"][pos["cluster"]].astype(np.int64) // (H * W) % S
    pt = space_points(sensor, hits["u"], hits["v"], pos["counts"], placement)
    return cl, pos, hits, pt, doublets(pt, placement.pairs, tan_q12, z0_sub, S)


# ---- the shapes the host and the device tests share ------------------------------------------------------------------------------------
class Tables:
    """A geometry or a placement as plain arrays (the host tests need no torch)."""

    def __init__(self, **arrays):
        vars(self).update(arrays)


def uniform_geometry(shape, u_pitch, v_pitch, n_sensors, unit_mm=5e-4):
    return Tables(u_pitch=np.full((1, shape[0]), u_pitch, np.int64), v_pitch=np.full((1, shape[1]), v_pitch, np.int64),
                  kind=np.zeros(n_sensors, np.int64), unit_mm=unit_mm)


def barrel(geometry, radii, ladders, per_ladder=1, unit_mm=5e-4):
    """``utils.PXDPlacement.barrel`` restated: the float tables and their one rounding."""
    origin, ua, va, layer = [], [], [], []
    for L in (0, 1):
        for j in range(ladders[L]):
            phi = 2.0 * np.pi * j / ladders[L]
            for k in range(per_ladder):
                length = float(geometry.v_pitch[geometry.kind[len(layer)]].sum()) * unit_mm
                origin.append([radii[L] * np.cos(phi), radii[L] * np.sin(phi), (k - (per_ladder - 1) / 2.0) * length])
                ua.append([-np.sin(phi), np.cos(phi), 0.0])
                va.append([0.0, 0.0, 1.0])
                layer.append(L)
    layer = np.array(layer)
    return Tables(origin=np.rint(np.array(origin) / unit_mm * 16).astype(np.int64), u_axis=np.rint(np.array(ua) * 2.0 ** 30).astype(np.int64),
                  v_axis=np.rint(np.array(va) * 2.0 ** 30).astype(np.int64), layer=layer,
                  pairs=((layer[:, None] == 0) & (layer[None, :] == 1)).astype(np.uint8), unit_mm=unit_mm)


# the default shape of the device tests: 3 events x 4 sensors (2 inner ladders, 2 outer ladders) of 13 x 37 cells of 100 x 120 units, on
# barrels of 14 and 22 mm; the windows are tight enough for both outcomes of both tests to occur (the tests assert that)
DEFAULT = dict(shape=(12, 13, 37), pitch=(100, 120), n_sensors=4, radii=(14.0, 22.0), ladders=(2, 2), dphi=0.02, z0_mm=1.5)


@functools.lru_cache(maxsize=None)
def default_case(kind="u8", threshold=0.0):
    """The default case and its checker result, computed once and shared: ``(images, geometry, placement, (tan_q12, z0_sub), chain(...))``."""
    n, h, w = DEFAULT["shape"]
    ev = (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(n, h, w, seed=57, p_hit=0.3)
    g = uniform_geometry((h, w), *DEFAULT["pitch"], DEFAULT["n_sensors"])
    p = barrel(g, DEFAULT["radii"], DEFAULT["ladders"])
    win = windows(DEFAULT["dphi"], DEFAULT["z0_mm"])
    return ev, g, p, win, chain(ev, g, p, *win, threshold=threshold)
