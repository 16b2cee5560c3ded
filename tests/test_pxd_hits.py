"""PXD hits, host side: the checker (tests/pxd_hits_reference.py) against an independent brute force over the dense sub-image of every
cluster in exact rationals, ``utils.PXDGeometry``, a hand case, the hit file and the C ABI of ``ieagan_pxd_hits`` (no GPU needed).  The device
side is tests/test_pxd_hits_gpu.py."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import pxd_clusters_reference as CR
import pxd_hits_reference as HR
import pxd_reco_reference as RR
import pxd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _hip, ctypes.CDLL(_hip.LIB_PATH)


def _nearest_float32(f, exact):
    """``f`` (float32) is a float32 nearest to the rational ``exact``: neither neighbour of ``f`` is closer."""
    f = np.float32(f)
    err = abs(Fraction(float(f)) - exact)
    return all(err <= abs(Fraction(float(np.nextafter(f, np.float32(side)))) - exact) for side in (-np.inf, np.inf))


def _brute_axis(profile, lo, pitch, head_tail):
    """The rule along one axis from the projected charges ``profile`` of the cells ``lo .. lo + len(profile) - 1`` of a sensor with cell
    pitches ``pitch``, in exact rationals and in the physical form: centres ``x_k``, not doubled ones.  -> (position, head-tail, clamped)."""
    total = sum(pitch)
    centre = lambda k: Fraction(sum(pitch[:k])) + Fraction(pitch[k], 2) - Fraction(total, 2)
    s, Q = len(profile), sum(profile)
    hi = lo + s - 1
    assert profile[0] > 0 and profile[-1] > 0
    ht = bool(head_tail) and s >= head_tail
    if ht:
        q_centre = Fraction(Q - profile[0] - profile[-1], s - 2)
        x = (centre(lo) + centre(hi)) / 2 + Fraction(profile[-1] * pitch[hi] - profile[0] * pitch[lo]) / (2 * q_centre)
    else:
        x = sum(Fraction(q) * centre(lo + k) for k, q in enumerate(profile)) / Q
    lower, upper = centre(lo) - Fraction(pitch[lo], 2), centre(hi) + Fraction(pitch[hi], 2)
    return min(max(x, lower), upper), ht, not lower <= x <= upper


@pytest.mark.parametrize("head_tail", [3, 4, 0])
@pytest.mark.parametrize("case", ["random_7x13x37", "structured_4x64x96"])
def test_checker_equals_a_brute_force_in_exact_rationals(case, head_tail):
    if case == "random_7x13x37":
        ev, split = R.synthetic_u8(7, 13, 37, seed=32, p_hit=0.3), 18
    else:
        ev, split = CR.cached_structured(4, 64, 96, 21, "u8")[0], 40
    n, h, w = ev.shape
    geometry = HR.two_type_geometry((h, w), split, n)
    u_pitch, v_pitch, kind = geometry
    cl, pos, hits = HR.reco_hits(ev, geometry, head_tail)
    assert hits["total"] == cl["total"] > 0
    lab = np.full(ev.size, -1, np.int64)
    lab[cl["index"].astype(np.int64)] = cl["label"]
    lab = lab.reshape(ev.shape)
    q = RR.dense_charge(cl, ev.shape).astype(np.int64)
    image = cl["first"].astype(np.int64) // (h * w)
    seen = dict(ht_u=0, ht_v=0, clamp_u=0, clamp_v=0, straddle=0)
    for j in range(cl["total"]):
        k = int(image[j])
        rows, cols = np.nonzero(lab[k] == j)
        sub = np.where(lab[k] == j, q[k], 0)[rows.min():rows.max() + 1, cols.min():cols.max() + 1]
        t = int(kind[k % len(kind)])
        xu, ht_u, cu = _brute_axis(sub.sum(1).tolist(), int(rows.min()), u_pitch[t].tolist(), head_tail)
        xv, ht_v, cv = _brute_axis(sub.sum(0).tolist(), int(cols.min()), v_pitch[t].tolist(), head_tail)
        assert _nearest_float32(hits["u"][j], xu) and _nearest_float32(hits["v"][j], xv), (j, hits["u"][j], float(xu), hits["v"][j], float(xv))
        assert hits["flags"][j] == ht_u * HR.HT_U + ht_v * HR.HT_V + cu * HR.CLAMP_U + cv * HR.CLAMP_V, j
        assert hits["v_start"][j] == cols.min() and hits["u_start"][j] == rows.min()
        assert (hits["qh_u"][j], hits["qt_u"][j], hits["qh_v"][j], hits["qt_v"][j]) == (sub[0].sum(), sub[-1].sum(), sub[:, 0].sum(), sub[:, -1].sum())
        straddle = v_pitch[t][cols.min()] != v_pitch[t][cols.max()]
        assert straddle == hits["straddle"][j]
        for name, on in (("ht_u", ht_u), ("ht_v", ht_v), ("clamp_u", cu), ("clamp_v", cv), ("straddle", straddle)):
            seen[name] += int(on)
    print(f"{case} head_tail {head_tail}: {cl['total']} clusters, {seen}")
    if head_tail == 3:
        assert seen["ht_u"] > 0 and seen["ht_v"] > 0 and seen["straddle"] > 0
        if case == "random_7x13x37":
            assert cl["total"] == 208 and seen["clamp_u"] > 0 and seen["clamp_v"] > 0
    if head_tail == 0:
        assert (hits["flags"] == 0).all()
    # a hit lies inside the extent of its cluster, hence inside its sensor
    assert (2 * hits["u"].astype(np.float64) >= hits["lower_u"]).all() and (2 * hits["u"].astype(np.float64) <= hits["upper_u"]).all()
    assert (2 * hits["v"].astype(np.float64) >= hits["lower_v"]).all() and (2 * hits["v"].astype(np.float64) <= hits["upper_v"]).all()


def test_hand_case_across_the_pitch_change():
    """One row of charges 10, 20, 40 at the columns 23, 24, 25 of a 64-wide sensor whose pitch changes from 111 to 121 at column 24."""
    ev = np.zeros((1, 8, 64), np.uint8)
    ev[0, 3, 23:26] = (10, 20, 40)
    geometry = (np.full((1, 8), 101), np.array([[111] * 24 + [121] * 40]), np.zeros(1, np.int64))
    assert HR.x2_of(geometry[1])[0, 23:26].tolist() == [-2287, -2055, -1813]
    cl, pos, hits = HR.reco_hits(ev, geometry)
    assert cl["total"] == 1 and hits["flags"].tolist() == [HR.HT_V] and hits["v_start"].tolist() == [23]
    lo, s, Q, qh, qt = hits["v_start"], cl["size_v"].astype(np.int64), cl["charge"].astype(np.int64), hits["qh_v"], hits["qt_v"]
    _, _, _, num, den, _, _ = HR.axis(hits["pv"], Q, lo, s, qh, qt, HR.x2_of(geometry[1]), np.asarray(geometry[1]), 3)
    assert (num.tolist(), den.tolist()) == ([-74540], [80]) and hits["v"].tolist() == [-931.75]
    assert hits["u"].tolist() == [(2 * 3 * 101 + 101 - 808) / 2.0]            # one row: its centre, by the centre of gravity
    _, _, cog = HR.reco_hits(ev, geometry, head_tail=0)
    want = (10 * -2287 + 20 * -2055 + 40 * -1813) / 140.0
    assert cog["flags"].tolist() == [0] and cog["v"][0] == np.float32(want) and round(want, 2) == -974.93


def test_geometry_tables_and_checks():
    import utils
    g = utils.PXDGeometry.belle2()
    assert (g.K, g.H, g.W, g.S) == (2, 250, 768, 40) and g.unit_mm == 5e-4
    assert g.u_length.tolist() == [25000, 25000] and g.v_length.tolist() == [89600, 122880]
    assert (g.u_length[0] * g.unit_mm, g.v_length[0] * g.unit_mm, g.v_length[1] * g.unit_mm) == pytest.approx((12.5, 44.8, 61.44), rel=1e-12)
    assert g.kind.tolist() == [0] * 16 + [1] * 24 and all(getattr(g, k).dtype == np.int32 for k in g.TABLES)
    assert g.v_pitch[0, [0, 255, 256, 767]].tolist() == [110, 110, 120, 120] and g.v_pitch[1, [255, 256]].tolist() == [140, 170]
    assert np.array_equal(g.v_x2, HR.x2_of(g.v_pitch)) and np.array_equal(g.u_x2, HR.x2_of(g.u_pitch))
    assert g.v_x2[0, 0] == 110 - 89600 and g.v_x2[0, -1] == 89600 - 120 and g.u_x2[0, 0] == -24900
    for bad in ((250, 767), (64, 64)):
        with pytest.raises(ValueError, match="250 x 768"):
            utils.PXDGeometry.belle2(bad)
    with pytest.raises(ValueError):
        utils.PXDGeometry.belle2(n_sensors=20)
    for h, w, pu, pv in ((250, 768, 100, 110), (13, 37, 101, 7), (1, 2, 3, 4095)):           # odd lengths and odd pitches included
        u = utils.PXDGeometry.uniform((h, w), pu, pv, n_sensors=3)
        assert (u.K, u.H, u.W, u.S) == (1, h, w, 3) and np.array_equal(u.u_x2, -u.u_x2[:, ::-1]) and np.array_equal(u.v_x2, -u.v_x2[:, ::-1])
        assert np.array_equal(u.v_x2[0], pv * (2 * np.arange(w) + 1 - w))
    assert utils.PXDGeometry(np.full((1, 4), 5), np.full((1, 6), 7)).kind.tolist() == [0] * 40
    ok_u, ok_v = np.full((2, 4), 5), np.full((2, 6), 7)
    for args, msg in (((np.full((2, 4), 0), ok_v, [0, 1]), "outside 1 .. 4095"), ((ok_u, np.full((2, 6), 4096), [0, 1]), "outside 1 .. 4095"),
                      ((np.full((1, 512), 2048), np.full((1, 6), 7), [0]), "2\\*\\*20"), ((ok_u, ok_v, [0, 2]), "outside the 2 type"),
                      ((ok_u, ok_v, [-1, 0]), "outside the 2 type"), ((ok_u, ok_v, None), "need a kind"), ((ok_u, np.full((3, 6), 7), [0]), "not integer arrays"),
                      ((np.full(4, 5), np.full(6, 7), [0]), "not integer arrays"), ((ok_u.astype(float), ok_v, [0]), "not integer arrays"),
                      ((ok_u, ok_v, [[0, 1]]), "kind")):
        with pytest.raises(ValueError, match=msg):
            utils.PXDGeometry(*args)
    assert utils.PXDGeometry(np.full((1, 511), 2048), np.full((1, 6), 7)).u_length[0] == 2 ** 20 - 2048      # the longest that passes


def test_hit_file_round_trip(tmp_path):
    import utils
    assert list(utils.HIT_COLUMNS) == ["event_offsets", "sensor", "u_mm", "v_mm", "charge", "seed", "size", "size_u", "size_v", "flags"]
    rng = np.random.Generator(np.random.PCG64(5))
    n = 17
    cols = dict(sensor=rng.integers(0, 40, n), u_mm=rng.uniform(-6.25, 6.25, n), v_mm=rng.uniform(-30, 30, n), charge=rng.integers(1, 70000, n),
                seed=rng.integers(1, 256, n), size=rng.integers(1, 3000, n), size_u=rng.integers(1, 250, n), size_v=rng.integers(1, 768, n),
                flags=rng.integers(0, 16, n))
    path = os.path.join(str(tmp_path), "hits.npz")
    utils.write_hits(path, [0, 5, 5, 17], unit_mm=5e-4, **cols)
    back = utils.read_hits(path)
    assert set(back) == set(utils.HIT_COLUMNS) | {"unit_mm"} and back["unit_mm"] == 5e-4 and back["event_offsets"].tolist() == [0, 5, 5, 17]
    for k, v in cols.items():
        assert back[k].dtype == utils.HIT_COLUMNS[k] and np.array_equal(back[k], v.astype(utils.HIT_COLUMNS[k])), k
    utils.write_hits(path, [0, 0], **{k: v[:0] for k, v in cols.items()})              # events without a hit
    assert utils.read_hits(path)["u_mm"].size == 0
    for over, msg in ((dict(event_offsets=[1, 17]), "start at 0"), (dict(event_offsets=[0, 9, 5, 17]), "not decrease"),
                      (dict(event_offsets=[0, 16]), "has 17 entries"), (dict(sensor=cols["sensor"] + 250), "uint8"),
                      (dict(size=cols["size"] + 70000), "uint16"), (dict(flags=-cols["flags"] - 1), "uint8")):
        args = {**cols, "event_offsets": [0, 5, 5, 17], **over}
        with pytest.raises(ValueError, match=msg):
            utils.write_hits(path, **args)
    np.savez(path, event_offsets=np.zeros(1, np.int64))
    with pytest.raises(ValueError, match="no hit file"):
        utils.read_hits(path)


def test_hits_entry_points_are_declared_exported_and_bound():
    _hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    for sym in ("ieagan_pxd_hits", "ieagan_pxd_hits_scratch"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTS and sym in _hip._SIGS, sym
    sig = _hip._SIGS["ieagan_pxd_hits"]
    assert len(sig) == 35 and sig[21] is ctypes.c_long and sig[:16] == [ctypes.c_void_p] * 16 and sig[23:] == [ctypes.c_void_p] * 12
    lib.ieagan_abi_version.restype = ctypes.c_int
    assert lib.ieagan_abi_version() == _hip.ABI_VERSION == int(re.search(r"#define IEAGAN_ABI_VERSION (\d+)", header).group(1))
    import utils
    for name in ("pxd_hits", "PXDHits", "PXDGeometry", "HIT_COLUMNS", "write_hits", "read_hits"):
        assert hasattr(utils, name), name


def test_hits_launcher_rejects_bad_arguments_before_any_launch():
    _, lib = _lib()
    lib.ieagan_last_error.restype = ctypes.c_char_p
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    buf = (ctypes.c_longlong * 64)()
    a = ctypes.addressof(buf)
    fn = lib.ieagan_pxd_hits
    fn.argtypes, fn.restype = [vp] * 16 + [i, i, i, i, i, l, i] + [vp] * 12, i
    good = dict(index=a, charge=a, label=a, digit_total=a, first=a, ccharge=a, size_u=a, size_v=a, cluster_total=a, cluster=a, accepted_total=a,
                u_x2=a, u_pitch=a, v_x2=a, v_pitch=a, kind=a, N=4, H=2, W=2, n_sensors=2, K=1, capacity=4, head_tail=3, pu=a, pv=a, v_start=a,
                qh_u=a, qt_u=a, qh_v=a, qt_v=a, u=a, v=a, flags=a, scratch=None, stream=None)
    bad = [(dict(N=0), "N = 0"), (dict(H=0), "bad image size"), (dict(N=40000, H=250, W=768), "int32 flat index"),
           (dict(H=4096, W=4096), "int32 cluster charge"), (dict(N=3), "not a multiple"), (dict(n_sensors=0), "not a multiple"),
           (dict(K=0), "K = 0"), (dict(capacity=-1), "negative"), (dict(head_tail=1), "head_tail = 1"), (dict(head_tail=2), "head_tail = 2"),
           (dict(head_tail=-3), "head_tail = -3"), (dict(digit_total=None), "digit_total / cluster_total / accepted_total"),
           (dict(accepted_total=a + 2), "digit_total / cluster_total / accepted_total"), (dict(kind=None), "geometry table"),
           (dict(v_x2=a + 1), "geometry table"), (dict(label=None), "index / charge / label is NULL"),
           (dict(size_v=None), "cluster table or the accepted list is NULL"), (dict(cluster=None), "cluster table or the accepted list is NULL"),
           (dict(pu=None), "output array is NULL"), (dict(flags=None), "output array is NULL"), (dict(qt_v=a + 2), "4-byte aligned"),
           (dict(u=a + 1), "4-byte aligned"), (dict(pv=a + 4), "8-byte aligned")]
    for over, msg in bad:
        assert fn(*dict(good, **over).values()) != 0, over
        assert msg in lib.ieagan_last_error().decode(), (over, lib.ieagan_last_error().decode())
    lib.ieagan_pxd_hits_scratch.restype = ctypes.c_long
    lib.ieagan_pxd_hits_scratch.argtypes = [i, i, i, l]
    assert lib.ieagan_pxd_hits_scratch(40, 250, 768, 480000) == 0           # every intermediate is an output of the call


def test_hits_surface_has_no_cpu_fallback():
    """Without a device the call is an error, never a host computation; with one, the same call is refused for its ``head_tail``."""
    import torch
    import utils
    error, msg = (ValueError, "head_tail = 2") if torch.cuda.is_available() else (RuntimeError, "no CPU fallback")
    with pytest.raises(error, match=msg):
        utils.pxd_hits(torch.zeros(40, 4, 4), utils.PXDGeometry.uniform((4, 4), 100, 110), head_tail=2)
