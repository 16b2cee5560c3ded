"""NumPy checker of ``utils.pxd_hits`` (tests only), on top of the cluster checker ``pxd_clusters_reference`` and the reconstruction checker
``pxd_reco_reference`` (which decides the accepted clusters and their order).

Per cluster, in int64 (``np.add.at`` / ``np.minimum.at``): the physical moments ``pu = sum q * u_x2[row]``, ``pv = sum q * v_x2[column]``
with the tables of the cluster's sensor type, the first row ``u_start`` and column ``v_start``, and the charges in the first / last row and
column of its extent.  Per accepted cluster and axis the rule of ``utils.pxd_hits`` verbatim: centre of gravity ``m / (2 Q)`` below
``head_tail`` cells, else head-tail ``((x2[lo] + x2[hi]) D + 2 (q_tail p[hi] - q_head p[lo]) (s - 2)) / (4 D)`` with ``D = Q - q_head -
q_tail``, clamped in integers to ``[x2[lo] - p[lo], x2[hi] + p[hi]] / 2``; one float64 division of two exact integers rounded to float32.
``tests/test_pxd_hits.py`` pins this against a brute force over the dense sub-image of every cluster with ``fractions.Fraction``.
"""
import numpy as np

import pxd_reco_reference as RR

HT_U, HT_V, CLAMP_U, CLAMP_V = 1, 2, 4, 8


def two_type_geometry(shape, split, n_sensors, utils=None):
    """The two-type test geometry for ``n_sensors`` sensors of ``shape = (H, W)``: type 0 (even sensors) u pitch 101, v pitch 111 below column
    ``split`` and 121 from it on; type 1 (odd sensors) u pitch 97, v pitch 131 / 109.  ``(u_pitch, v_pitch, kind)``, or the ``PXDGeometry``
    of them when the ``utils`` module is given."""
    H, W = shape
    u = np.array([[101] * H, [97] * H])
    v = np.array([[111] * split + [121] * (W - split), [131] * split + [109] * (W - split)])
    kind = np.arange(n_sensors) % 2
    return (u, v, kind) if utils is None else utils.PXDGeometry(u, v, kind)


def x2_of(pitch):
    """Doubled, centred cell centres of pitch rows ``[K, L]``: ``2 * sum(pitch[:k]) + pitch[k] - sum(pitch)``."""
    p = np.asarray(pitch, np.int64)
    return 2 * (np.cumsum(p, 1) - p) + p - p.sum(1, keepdims=True)


def per_cluster(cl, shape, u_pitch, v_pitch, kind):
    """int64 tables per cluster of a ``clusters_of_digits`` dict: ``pu``, ``pv``, ``u_start``, ``v_start``, ``qh_u``, ``qt_u``, ``qh_v``,
    ``qt_v`` and ``type``."""
    N, H, W = shape
    S, T = len(kind), cl["total"]
    ux2, vx2 = x2_of(u_pitch), x2_of(v_pitch)
    idx = cl["index"].astype(np.int64)
    rem = idx % (H * W)
    r, c, q, lab = rem // W, rem % W, cl["digit_charge"].astype(np.int64), cl["label"].astype(np.int64)
    t = np.asarray(kind, np.int64)[(idx // (H * W)) % S]
    out = {k: np.zeros(T, np.int64) for k in ("pu", "pv", "qh_u", "qt_u", "qh_v", "qt_v")}
    np.add.at(out["pu"], lab, q * ux2[t, r])
    np.add.at(out["pv"], lab, q * vx2[t, c])
    u_start, v_start = np.full(T, H, np.int64), np.full(T, W, np.int64)
    np.minimum.at(u_start, lab, r)
    np.minimum.at(v_start, lab, c)
    np.add.at(out["qh_u"], lab, np.where(r == u_start[lab], q, 0))
    np.add.at(out["qt_u"], lab, np.where(r == (u_start + cl["size_u"] - 1)[lab], q, 0))
    np.add.at(out["qh_v"], lab, np.where(c == v_start[lab], q, 0))
    np.add.at(out["qt_v"], lab, np.where(c == (v_start + cl["size_v"] - 1)[lab], q, 0))
    first = cl["first"].astype(np.int64)
    assert np.array_equal(u_start, first % (H * W) // W)          # digits ascend in raster order: the first digit lies in the first row
    return dict(out, u_start=u_start, v_start=v_start, type=np.asarray(kind, np.int64)[(first // (H * W)) % S])


def axis(m, Q, lo, s, qh, qt, x2, p, head_tail):
    """The rule along one axis for arrays of clusters (``x2`` / ``p``: the rows ``[clusters, L]`` of their types) ->
    ``(position float32, used head-tail, clamped, num, den, lower, upper)``."""
    j = np.arange(len(m))
    hi = lo + s - 1
    xlo, xhi, plo, phi = x2[j, lo], x2[j, hi], p[j, lo], p[j, hi]
    ht = (s >= head_tail) if head_tail else np.zeros(len(m), bool)
    D = Q - qh - qt
    assert (D[ht] >= (s - 2)[ht]).all() and (Q > 0).all()
    num = np.where(ht, (xlo + xhi) * D + 2 * (qt * phi - qh * plo) * (s - 2), m)
    den = np.where(ht, 4 * D, 2 * Q)
    lower, upper = xlo - plo, xhi + phi
    below, above = 2 * num < den * lower, 2 * num > den * upper
    num = np.where(below, lower, np.where(above, upper, num))
    den = np.where(below | above, 2, den)
    assert (np.abs(num) < 2 ** 53).all() and (den > 0).all()
    return (num.astype(np.float64) / den.astype(np.float64)).astype(np.float32), ht, below | above, num, den, lower, upper


def hits(cl, pos, shape, geometry, head_tail=3):
    """Everything of the contract of ``ieagan_pxd_hits`` for the clusters ``cl`` and accepted list ``pos`` (``pxd_reco_reference.positions``)
    of an ``[N, H, W]`` batch; ``geometry = (u_pitch [K, H], v_pitch [K, W], kind [S])``.  The per-cluster tables, and per hit ``u``, ``v``,
    ``flags``; for the tests' own assertions also ``ht_u`` / ``ht_v`` / ``clamp_u`` / ``clamp_v``, the bounds ``lower_*`` / ``upper_*``
    (doubled units) and ``straddle`` (the cluster's columns lie on both sides of a pitch change)."""
    u_pitch, v_pitch, kind = (np.asarray(a, np.int64) for a in geometry)
    pc = per_cluster(cl, shape, u_pitch, v_pitch, kind)
    j = pos["cluster"].astype(np.int64)
    t, Q = pc["type"][j], cl["charge"].astype(np.int64)[j]
    su, sv = cl["size_u"].astype(np.int64)[j], cl["size_v"].astype(np.int64)[j]
    u, ht_u, cu, _, _, lo_u, up_u = axis(pc["pu"][j], Q, pc["u_start"][j], su, pc["qh_u"][j], pc["qt_u"][j], x2_of(u_pitch)[t], u_pitch[t], head_tail)
    v, ht_v, cv, _, _, lo_v, up_v = axis(pc["pv"][j], Q, pc["v_start"][j], sv, pc["qh_v"][j], pc["qt_v"][j], x2_of(v_pitch)[t], v_pitch[t], head_tail)
    n = np.arange(j.size)
    straddle = v_pitch[t][n, pc["v_start"][j]] != v_pitch[t][n, pc["v_start"][j] + sv - 1]
    flags = (ht_u * HT_U + ht_v * HT_V + cu * CLAMP_U + cv * CLAMP_V).astype(np.uint8)
    return dict(pc, u=u, v=v, flags=flags, ht_u=ht_u, ht_v=ht_v, clamp_u=cu, clamp_v=cv, lower_u=lo_u, upper_u=up_u, lower_v=lo_v, upper_v=up_v,
                straddle=straddle, total=int(j.size))


def reco_hits(images, geometry, head_tail=3, threshold=0.0, seed_cut=0, charge_cut=0):
    """``(clusters, positions, hits)`` of ``images`` ``[N, H, W]`` (fp32 or uint8, host)."""
    cl, pos = RR.reco(images, threshold, seed_cut, charge_cut)
    return cl, pos, hits(cl, pos, np.asarray(images).shape, geometry, head_tail)
