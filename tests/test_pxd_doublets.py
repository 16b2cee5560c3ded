"""PXD space points and doublets, host side: the checker (tests/pxd_doublets_reference.py) against a brute force in Python ``int`` /
``fractions.Fraction``; the integer bounds the kernels rely on, at the corners of the allowed ranges; the square root by "double root, then
correct"; ``utils.PXDPlacement``; planted tracks; the second header and its entry points; the launchers' refusals; the argument refusals
of ``validate.py`` (no GPU needed).  The device side is tests/test_pxd_doublets_gpu.py."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import pxd_doublets_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_checker_against_a_brute_force_in_exact_rationals():
    ev, g, p, (tan_q12, z0_sub), (cl, pos, hits, pt, db) = DR.default_case()
    S, (N, H, W) = 4, ev.shape
    assert N // S == 3 and pt["total"] == pos["total"] > 0
    sensor = cl["first"][pos["cluster"]].astype(np.int64) // (H * W) % S
    points = []
    for a in range(pt["total"]):
        s = int(sensor[a])
        lu, lv = (Fraction(float(np.float32(x))) * 16 for x in (hits["u"][a], hits["v"][a]))
        lu, lv = (math.floor(x) if x - math.floor(x) < Fraction(1, 2) or (x - math.floor(x) == Fraction(1, 2) and math.floor(x) % 2 == 0)
                  else math.floor(x) + 1 for x in (lu, lv))                       # round to nearest, ties to even
        X = [int(p.origin[s, c]) + math.floor(Fraction(int(p.u_axis[s, c]) * lu + int(p.v_axis[s, c]) * lv, 2 ** 30) + Fraction(1, 2)) for c in range(3)]
        r = int(pt["r"][a])
        assert r * r <= X[0] ** 2 + X[1] ** 2 < (r + 1) ** 2                      # the floor of the root, by its definition
        assert X == [int(pt[k][a]) for k in "xyz"] and int(pt["sensor"][a]) == s and int(pt["role"][a]) == int(p.layer[s])
        points.append((X, r, s))
    image = np.repeat(np.arange(N), pos["counts"])
    assert np.array_equal(pt["offsets"], np.searchsorted(image, np.arange(N + 1)))          # hits are stored image by image
    found = []
    for a, (Xa, ra, sa) in enumerate(points):
        for b, (Xb, rb, sb) in enumerate(points):
            if image[a] // S != image[b] // S or p.layer[sa] != 0 or p.layer[sb] != 1 or not p.pairs[sa, sb]:
                continue
            dot, cross = Xa[0] * Xb[0] + Xa[1] * Xb[1], abs(Xa[0] * Xb[1] - Xa[1] * Xb[0])
            if dot <= 0 or Fraction(cross, dot) > Fraction(tan_q12, 4096) or rb <= ra:
                continue
            if abs(Fraction(Xa[2] * rb - Xb[2] * ra, rb - ra)) <= z0_sub:           # the line through both hits in (r, z), at r = 0
                found.append((a, b))
    assert found == list(zip(db["inner"].tolist(), db["outer"].tolist())) and len(found) == db["total"] > 0
    assert np.array_equal(db["partners"], np.bincount([a for a, _ in found], minlength=pt["total"]))
    assert np.array_equal(db["event_doublets"], np.bincount([image[a] // S for a, _ in found], minlength=3))


def test_every_bound_holds_at_the_corners_of_the_allowed_ranges():
    C = 2 ** 23 - 1                                 # the largest coordinate
    R = math.isqrt(2 * C * C)                       # and radius
    tan_q12, z0_sub = 32768, 2 ** 23 - 1
    assert R < 2 ** 24                              # fits the 24 bits of a tile record beside the sensor
    for xa, ya, xb, yb in ((C, C, C, C), (C, -C, C, C), (-C, -C, -C, -C), (C, C, -C, C)):
        dot, cross = xa * xb + ya * yb, abs(xa * yb - ya * xb)
        assert abs(dot) < 2 ** 47 and cross < 2 ** 47 and cross << 12 < 2 ** 63 and abs(tan_q12 * dot) < 2 ** 63
    for za, zb, ra, rb in ((C, -C, R - 1, R), (-C, C, 0, R), (C, C, R, R)):
        assert abs(za * rb - zb * ra) < 2 ** 48 and z0_sub * abs(rb - ra) < 2 ** 48 < 2 ** 63
    lu = 2 ** 23 - 1                                # |u * 16| of a sensor below 2**20 units long
    assert 2 * 2 ** 30 * lu + 2 ** 29 < 2 ** 54 < 2 ** 63 and 2 * C * C < 2 ** 47 < 2 ** 53
    # the largest rows of both comparisons, through the checker's int64 form: no wrap
    big = np.array([C], np.int64)
    assert DR.passes(big[0], big[0], big[0], np.int64(R - 1), big, big, -big, np.array([R], np.int64), tan_q12, z0_sub).tolist() == [False]
    assert DR.passes(big[0], big[0], big[0], np.int64(R - 1), big, big, big, np.array([R], np.int64), tan_q12, z0_sub).tolist() == [True]


def test_the_square_root_by_double_root_and_correction_is_isqrt():
    top = math.isqrt(2 ** 47 - 1)                   # k up to 2**23 * sqrt(2)
    rng = np.random.Generator(np.random.PCG64(5))
    ks = set(rng.integers(1, top + 1, 20000).tolist()) | {1, 2, 3, top - 1, top, 2 ** 23, 2 ** 23 - 1, 94906265 % top}
    for k in ks:
        for s in (k * k - 1, k * k, k * k + 1):
            if s < 2 ** 47:
                assert DR.isqrt_by_double(s) == math.isqrt(s), s
    for s in (0, 1, 2, 2 ** 47 - 1):
        assert DR.isqrt_by_double(s) == math.isqrt(s), s


def _frame(phi, tilt):
    n = np.array([np.cos(phi), np.sin(phi), 0.0])
    u = np.array([-np.sin(phi), np.cos(phi), 0.0])
    v = np.cross(n, u)
    return u * np.cos(tilt) + v * np.sin(tilt), v * np.cos(tilt) - u * np.sin(tilt)


def test_placement_refusals_round_trip_and_the_nominal_barrel():
    import utils
    P = utils.PXDPlacement
    o, a, layer = np.zeros((3, 3), np.int64), np.tile(np.array([2 ** 30, 0, 0]), (3, 1)), np.array([0, 1, -1])
    ok = P(o, a, a, layer)
    assert ok.S == 3 and ok.pairs.tolist() == [[0, 1, 0], [0, 0, 0], [0, 0, 0]] and ok.origin.dtype == np.int32 and ok.pairs.dtype == np.uint8
    assert P(o, a, a, layer, np.ones((3, 3))).pairs.tolist() == ok.pairs.tolist()           # outside inner x outer: zeroed
    for args, what in (((o[:2], a, a, layer), "not integer arrays"), ((o, a, a[:, :2], layer), "not integer arrays"), ((o, a, a, layer[:2]), "not integer arrays"),
                       ((o.astype(np.float64), a, a, layer), "not integer arrays"), ((o, a, a, np.array([0, 2, 1])), "outside -1 .. 1"),
                       ((o, a, a, np.array([-2, 0, 1])), "outside -1 .. 1"), ((o, a + 1, a, layer), "beyond 2..30"), ((o, a, -a - 1, layer), "beyond 2..30"),
                       ((o + 2 ** 23, a, a, layer), "centre reaches 2..23"), ((o, a, a, layer, np.ones((2, 3))), r"pairs \(2, 3\) is not"),
                       ((np.zeros((256, 3), np.int64), np.zeros((256, 3), np.int64), np.zeros((256, 3), np.int64), np.zeros(256, np.int64)), "more than 255")):
        with pytest.raises(ValueError, match=what):
            P(*args)
    # the corner check needs the half lengths of a geometry: at construction when one is given, else on first use
    g = utils.PXDGeometry.uniform((64, 64), 100, 120, 3)
    far = o + np.array([2 ** 23 - 16 * 3200, 0, 0])              # the centre is inside, the corner along +x (u) is at 2**23
    av = np.tile(np.array([0, 2 ** 30, 0]), (3, 1))
    with pytest.raises(ValueError, match="corner of sensor 0 reaches 2..23"):
        P(far, a, av, layer, geometry=g)
    late = P(far, a, av, layer)
    with pytest.raises(ValueError, match="corner of sensor 0 reaches"):
        late.check_corners(g)
    P(far - np.array([1, 0, 0]), a, av, layer, geometry=g)
    with pytest.raises(ValueError, match="3 sensors in units of"):
        ok.check_corners(utils.PXDGeometry.uniform((64, 64), 100, 120, 4))
    # from_float: an orthonormal frame comes back to within 1 sub-unit over a sensor
    frames = [_frame(phi, tilt) for phi, tilt in ((0.3, 0.0), (2.0, 0.2), (-1.1, -0.4))]
    origin = np.array([[14.0, 1.0, -3.0], [-22.0, 5.0, 30.0], [0.5, -14.0, 0.0]])
    f = P.from_float(origin, [fr[0] for fr in frames], [fr[1] for fr in frames], layer, geometry=g)
    assert np.array_equal(f.origin, np.rint(origin / 5e-4 * 16)) and np.abs(f.u_axis).max() <= 2 ** 30
    lu, lv = 16 * 3200, -16 * 3840                  # a corner of the sensor, sub-units
    for s, (u, v) in enumerate(frames):
        exact = origin[s] / 5e-4 * 16 + u * lu + v * lv
        got = f.origin[s].astype(np.int64) + ((f.u_axis[s].astype(np.int64) * lu + f.v_axis[s].astype(np.int64) * lv + 2 ** 29) >> 30)
        assert np.abs(got - exact).max() <= 1.0, s
        assert abs(np.dot(f.u_axis[s] / 2.0 ** 30, f.v_axis[s] / 2.0 ** 30)) < 1e-8
    # belle2: 16 + 24 sensors at 14 and 22 mm, the order of create_g1.py:95, every inner sensor pairs with every outer one
    gb = utils.PXDGeometry.belle2()
    b = P.belle2(gb)
    radius = np.hypot(b.origin[:, 0].astype(np.float64), b.origin[:, 1].astype(np.float64))
    assert np.abs(radius[:16] - 14.0 / 5e-4 * 16).max() <= 1.0 and np.abs(radius[16:] - 22.0 / 5e-4 * 16).max() <= 1.0
    assert b.layer.tolist() == [0] * 16 + [1] * 24 and int(b.pairs.sum()) == 16 * 24 and b.pairs[:16, 16:].all()
    assert b.origin[0, 2] == -b.origin[1, 2] == -int(gb.v_length[0]) * 8 and b.origin[16, 2] == -b.origin[17, 2] == -int(gb.v_length[1]) * 8
    phi = np.arctan2(b.origin[:, 1], b.origin[:, 0]) % (2 * np.pi)
    assert np.allclose(phi[:16], np.repeat(np.arange(8) * 2 * np.pi / 8, 2), atol=1e-6) and np.allclose(phi[16:], np.repeat(np.arange(12) * 2 * np.pi / 12, 2), atol=1e-6)
    assert (b.v_axis == np.array([0, 0, 2 ** 30])).all() and "from memory" in P.belle2.__doc__ and "basf2" in P.belle2.__doc__
    assert b.same_as(P.belle2(gb)) and not b.same_as(P.belle2(gb, radii=(14.0, 22.5)))
    with pytest.raises(ValueError, match="are not the 40 sensors"):
        P.barrel(gb, (14.0, 22.0), (8, 11))
    # the checker's barrel is the package's
    gd = DR.uniform_geometry((13, 37), 100, 120, 4)
    d = DR.barrel(gd, (14.0, 22.0), (2, 2))
    assert P(d.origin, d.u_axis, d.v_axis, d.layer).same_as(P.barrel(utils.PXDGeometry.uniform((13, 37), 100, 120, 4), (14.0, 22.0), (2, 2), 1))
    for dphi, z0, what in ((0.0, 1.0, "tan_q12 = 0"), (1.5, 1.0, "outside 1 .. 32768"), (-0.1, 1.0, "tan_q12"), (0.3, -1.0, "z0_sub"), (0.3, 263.0, "z0_sub")):
        with pytest.raises(ValueError, match=what):
            utils.pxd_doublet_windows(dphi, z0)
    assert utils.pxd_doublet_windows() == DR.windows(0.3, 10.0) == (1267, 320000) and utils.pxd_doublet_windows(math.atan(8.0), 0.0) == (32768, 0)


def _planted(n_events=6, tracks=5, seed=2):          # a seed at which no two planted pixels touch (asserted below)
    """Straight lines from ``(0, 0, z_v)`` through one inner and one outer ladder at azimuth 0 (two sensors of 64 x 64 cells of 50 x 60 um
    each), one single-pixel hit per crossing: ``(images, geometry, placement, planted)``, ``planted`` = the (inner, outer) flat pixel indices
    of every track."""
    Hc, Wc, pu, pv, unit, radii, z0_mm = 64, 64, 100, 120, 5e-4, (14.0, 22.0), 2.0
    g = DR.uniform_geometry((Hc, Wc), pu, pv, 4)
    p = DR.barrel(g, radii, (1, 1), 2)
    rng = np.random.Generator(np.random.PCG64(seed))
    ev = np.zeros((n_events * 4, Hc, Wc), np.uint8)
    planted = []
    for e in range(n_events):
        z_v = rng.uniform(-z0_mm / 2, z0_mm / 2)
        for _ in range(tracks):
            phi, slope = rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1)          # the ladder is 3.2 mm wide at 14 / 22 mm; dz / dr
            pixels = []
            for L in (0, 1):
                # the ladder plane x = R: the line (t cos phi, t sin phi, z_v + slope t) meets it at t = R / cos phi
                t = radii[L] / math.cos(phi)
                u_mm, z_mm = t * math.sin(phi), z_v + slope * t
                k = 0 if z_mm < 0 else 1            # the sensors of a ladder are centred at -+ half a length
                v_mm = z_mm - (k - 0.5) * Wc * pv * unit
                row, col = math.floor((u_mm / unit + Hc * pu / 2) / pu), math.floor((v_mm / unit + Wc * pv / 2) / pv)
                assert 0 <= row < Hc and 0 <= col < Wc
                n = e * 4 + 2 * L + k
                ev[n, row, col] = 100
                pixels.append((n * Hc + row) * Wc + col)
            planted.append(tuple(pixels))
    return ev, g, p, planted, z0_mm


def test_planted_tracks_are_found_and_shuffling_the_outer_hits_lowers_the_acceptance():
    """By construction, with no measured number.  A planted hit is the centre of the pixel its line crosses, so it sits within half a pitch
    of the line: 25 um along u, 30 um along v.  Azimuth: the two crossings of a line through the z axis have the same azimuth, so the hits
    differ by at most 0.025 / 14 + 0.025 / 22 < 0.003 rad (+ 31 nm of rounding): ``dphi = 0.01`` has a slack of three.  Beam line: the line
    through the two hits meets r = 0 at ``(z_a r_b - z_b r_a) / (r_b - r_a)``; 30 um on each z moves that by at most 0.03 (22 + 14) / 8 =
    0.135 mm, and the shift of r by the 25 um (u du / R <= 1.2 * 0.025 / 14 mm) by less than 0.02 mm: with ``|z_v| <= z0 / 2`` and
    ``z0 = 2 mm`` the slack is 1 mm against 0.16."""
    import utils
    ev, g, p, planted, z0_mm = _planted()
    win = DR.windows(0.01, z0_mm)
    cl, pos, _, pt, db = DR.chain(ev, g, p, *win)
    first = cl["first"][pos["cluster"]].astype(np.int64)
    assert (cl["size"][pos["cluster"]] == 1).all() and len(set(sum(planted, ()))) == 2 * len(planted) == pt["total"]
    row_of = {int(f): a for a, f in enumerate(first)}
    found = set(zip(db["inner"].tolist(), db["outer"].tolist()))
    assert all((row_of[i], row_of[o]) in found for i, o in planted)
    # the same hits with the outer sensors of the events rotated by one event: every per-sensor statistic is unchanged
    shuffled = ev.reshape(-1, 4, 64, 64).copy()
    shuffled[:, 2:] = np.roll(shuffled[:, 2:], 1, axis=0)
    _, _, _, spt, sdb = DR.chain(shuffled.reshape(ev.shape), g, p, *win)
    real, fake = (DR.result(DR.tables(a, b, p.layer, 4), 4) for a, b in ((pt, db), (spt, sdb)))
    assert np.array_equal(np.sort(np.diff(pt["offsets"])), np.sort(np.diff(spt["offsets"])))
    print(f"planted {len(planted)} found {db['total']} acceptance {real['acceptance']:.3f}, shuffled {sdb['total']} acceptance {fake['acceptance']:.3f}")
    assert fake["acceptance"] < real["acceptance"]
    full = lambda r: dict(r, tan_q12=win[0], z0_sub=win[1], shape=(64, 64), **{k: getattr(p, k) for k in utils.PXDPlacement.TABLES})
    d = utils.pxd_doublet_distance(full(real), full(fake))
    assert d == DR.distance(real, fake) and d["acceptance_rel_err"] == (real["acceptance"] - fake["acceptance"]) / real["acceptance"] > 0
    assert all(v == 0.0 for v in utils.pxd_doublet_distance(full(real), full(real)).values())
    for change, what in ((dict(tan_q12=5), "tan_q12"), (dict(z0_sub=1), "z0_sub"), (dict(shape=(64, 65)), "shape"), (dict(layer=np.array([0, 0, 1, -1])), "placement table layer"),
                         (dict(origin=p.origin + 1), "placement table origin")):
        with pytest.raises(ValueError, match=what):
            utils.pxd_doublet_distance(full(real), dict(full(fake), **change))
    empty = dict(full(real), doublets_per_event=0.0, acceptance=float("nan"), sensor_pairs=np.zeros((4, 4), np.int64), partners_spectrum=np.zeros(64, np.int64))
    assert all(math.isnan(v) for v in utils.pxd_doublet_distance(empty, full(fake)).values())


def _lib():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    lib.ieagan_last_error.restype = ctypes.c_char_p
    return _hip, lib


def test_the_second_header_declares_exactly_the_tracking_entry_points():
    _hip, lib = _lib()
    tracking = open(os.path.join(ROOT, "include", "ieagan_pxd_tracking.h")).read()
    first = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    declared = re.findall(r"^(?:int|long|const char\*) (ieagan_\w+)\(", tracking, re.M)
    assert declared == ["ieagan_pxd_space_points", "ieagan_pxd_doublets_scratch", "ieagan_pxd_doublets", "ieagan_pxd_doublet_stats"]
    assert sorted(declared) == sorted(_hip.EXPORTS_TRACKING) == sorted(_hip._SIGS_TRACKING) and '#include "ieagan_hip.h"' in tracking
    for sym in declared:
        assert hasattr(lib, sym), sym
        assert sym not in _hip.EXPORTS and sym not in _hip._SIGS and not re.search(r"\b%s\b" % sym, first), sym
    points, scratch, doublets, stats = (_hip._SIGS_TRACKING[s] for s in declared)
    assert (len(points), len(scratch), len(doublets), len(stats)) == (24, 3, 23, 14)
    assert [k for k, t in enumerate(points) if t is ctypes.c_long] == [15] and [k for k, t in enumerate(doublets) if t is ctypes.c_long] == [11, 14]
    assert [k for k, t in enumerate(stats) if t is ctypes.c_long] == [10] and scratch[2] is ctypes.c_long
    # the first header and its binding are what they were
    assert len(re.findall(r"^(?:int|long|const char\*) ieagan_\w+\(", first, re.M)) == len(_hip.EXPORTS) == 90
    lib.ieagan_abi_version.restype = ctypes.c_int
    assert lib.ieagan_abi_version() == _hip.ABI_VERSION == 12 and "IEAGAN_ABI_VERSION" not in tracking.replace("IEAGAN_ABI_VERSION is unchanged", "")
    bound = _hip.lib()
    assert bound.ieagan_pxd_doublets_scratch.restype is ctypes.c_long and bound.ieagan_pxd_doublets.restype is ctypes.c_int
    assert "pxd_doublets" in open(os.path.join(ROOT, "iea-gan_amd", "csrc", "build.sh")).read()
    assert "ieagan_pxd_tracking.h" in open(os.path.join(ROOT, "README.md")).read()
    import utils
    for name in ("PXDPlacement", "PXDSpacePoints", "pxd_space_points", "PXDDoublets", "pxd_doublets", "pxd_doublet_windows", "PXDDoubletStatistics",
                 "pxd_doublet_distance"):
        assert hasattr(utils, name), name


def _refusals(lib, sigs, name, args, scalars, cases):
    fn = getattr(lib, name)
    fn.argtypes = sigs[name]
    buf = (ctypes.c_longlong * 256)()
    p = ctypes.addressof(buf)
    good = {k: scalars.get(k, p + 64 * i) for i, k in enumerate(args)}           # distinct, 8-byte aligned addresses inside buf
    for change, text in cases(p):
        rc = fn(*dict(good, **change).values(), None)
        msg = lib.ieagan_last_error().decode()
        assert rc != 0 and msg.startswith(name[len("ieagan_"):] + ": ") and text in msg, (change, msg)
    assert len(good) + 1 == len(sigs[name])
    return good


SHAPE = lambda p: [(dict(N=0), "N = 0 outside 1 .. 65535"), (dict(N=65536), "outside 1 .. 65535"), (dict(n_sensors=0), "n_sensors = 0 outside 1 .. 255"),
                   (dict(N=512, n_sensors=256), "n_sensors = 256 outside 1 .. 255"), (dict(n_sensors=3), "N = 4 is not a multiple of n_sensors = 3"),
                   (dict(capacity=-1), "capacity = -1 is negative")]


def test_the_space_point_launcher_rejects_bad_arguments_before_any_launch():
    _hip, lib = _lib()
    args = ("cluster accepted_total first cluster_total counts u v origin u_axis v_axis layer N H W n_sensors capacity x y z r sensor role "
            "offsets").split()
    scalars = dict(N=4, H=8, W=12, n_sensors=2, capacity=16)

    def cases(p):
        out = SHAPE(p) + [(dict(H=0), "bad image size"), (dict(W=-1), "bad image size"), (dict(N=64, n_sensors=64, H=8192, W=8192), "does not fit the int32 flat index")]
        out += [(dict([(k, None)]), "accepted_total / cluster_total is NULL or misaligned") for k in ("accepted_total", "cluster_total")]
        out += [(dict(accepted_total=p + 2), "accepted_total / cluster_total is NULL or misaligned")]
        out += [(dict([(k, None)]), "a placement table is NULL or not 4-byte aligned") for k in ("origin", "u_axis", "v_axis", "layer")]
        out += [(dict(layer=p + 1), "a placement table is NULL or not 4-byte aligned")]
        out += [(dict([(k, None)]), "counts / offsets is NULL or not 4-byte aligned") for k in ("counts", "offsets")] + [(dict(offsets=p + 2), "counts / offsets is NULL")]
        out += [(dict([(k, None)]), "cluster / first / u / v is NULL with capacity 16") for k in ("cluster", "first", "u", "v")]
        out += [(dict([(k, None)]), "an output array is NULL with capacity 16") for k in ("x", "y", "z", "r", "sensor", "role")]
        out += [(dict([(k, p + 2)]), "an int32 / fp32 array is not 4-byte aligned") for k in ("cluster", "first", "u", "v", "x", "y", "z", "r", "sensor")]
        return out
    assert list(_refusals(lib, _hip._SIGS_TRACKING, "ieagan_pxd_space_points", args, scalars, cases)) == args


def test_the_doublet_launchers_reject_bad_arguments_before_any_launch():
    _hip, lib = _lib()
    args = "x y z r sensor role offsets accepted_total pairs N n_sensors capacity tan_q12 z0_sub doublet_capacity partners event_doublets pair_doublets total inner outer scratch".split()
    scalars = dict(N=4, n_sensors=2, capacity=16, tan_q12=1267, z0_sub=320000, doublet_capacity=8)

    def cases(p):
        out = SHAPE(p) + [(dict(doublet_capacity=-1), "doublet_capacity = -1 is negative"), (dict(tan_q12=0), "tan_q12 = 0 outside 1 .. 32768"),
                          (dict(tan_q12=32769), "tan_q12 = 32769 outside"), (dict(tan_q12=-5), "tan_q12 = -5 outside"), (dict(z0_sub=-1), "z0_sub = -1 outside"),
                          (dict(z0_sub=2 ** 23), "z0_sub = 8388608 outside 0 .. 2^23 - 1"), (dict(accepted_total=None), "accepted_total is NULL or misaligned"),
                          (dict(accepted_total=p + 2), "accepted_total is NULL or misaligned"), (dict(pairs=None), "pairs is NULL"),
                          (dict(scratch=None), "scratch (ieagan_pxd_doublets_scratch int32 words) is NULL"), (dict(scratch=p + 2), "scratch (")]
        out += [(dict([(k, None)]), "offsets / event_doublets / pair_doublets / total is NULL or not 4-byte aligned") for k in ("offsets", "event_doublets", "pair_doublets", "total")]
        out += [(dict(total=p + 1), "offsets / event_doublets / pair_doublets / total is NULL")]
        out += [(dict([(k, None)]), "a space-point array is NULL with capacity 16") for k in ("x", "y", "z", "r", "sensor", "role")]
        out += [(dict(partners=None), "partners is NULL with capacity 16")] + [(dict([(k, None)]), "inner / outer is NULL with doublet_capacity 8") for k in ("inner", "outer")]
        out += [(dict([(k, p + 2)]), "an int32 array is not 4-byte aligned") for k in ("x", "y", "z", "r", "sensor", "partners", "inner", "outer")]
        return out
    assert list(_refusals(lib, _hip._SIGS_TRACKING, "ieagan_pxd_doublets", args, scalars, cases)) == args
    scratch = lib.ieagan_pxd_doublets_scratch
    scratch.argtypes, scratch.restype = _hip._SIGS_TRACKING["ieagan_pxd_doublets_scratch"], ctypes.c_long
    assert scratch(40, 40, 480000) == 4 * (480000 // 256 + 1 + 1) and scratch(12, 4, 0) == 4 * 4 and scratch(0, 4, 16) == scratch(4, 0, 16) == scratch(4, 2, -1) == 0
    args = "role offsets accepted_total digit_total layer partners event_doublets pair_doublets N n_sensors capacity tables overflow".split()
    scalars = dict(N=4, n_sensors=2, capacity=16)

    def cases(p):
        out = SHAPE(p) + [(dict([(k, None)]), "accepted_total / digit_total is NULL or misaligned") for k in ("accepted_total", "digit_total")]
        out += [(dict(digit_total=p + 2), "digit_total is NULL or misaligned")]
        out += [(dict([(k, None)]), "offsets / layer / event_doublets / pair_doublets is NULL or not 4-byte aligned") for k in ("offsets", "layer", "event_doublets", "pair_doublets")]
        out += [(dict([(k, v)]), "tables / overflow is NULL or not 8-byte aligned") for k in ("tables", "overflow") for v in (None, p + 4)]
        out += [(dict([(k, None)]), "role / partners is NULL with capacity 16") for k in ("role", "partners")] + [(dict(partners=p + 2), "partners is not 4-byte aligned")]
        return out
    assert list(_refusals(lib, _hip._SIGS_TRACKING, "ieagan_pxd_doublet_stats", args, scalars, cases)) == args


def test_host_side_refusals_come_before_any_device_call(monkeypatch):
    import _hip
    import utils

    def no_device(*a, **k):
        raise AssertionError("a device call before the host checks were done")
    monkeypatch.setattr(_hip, "call", no_device)
    g = utils.PXDGeometry.uniform((13, 37), 100, 120, 4)
    p = utils.PXDPlacement.barrel(g, (14.0, 22.0), (2, 2), 1)
    for kw, error, what in ((dict(dphi=0.0), ValueError, "tan_q12"), (dict(z0_mm=-1.0), ValueError, "z0_sub"), (dict(seed_cut=-1), ValueError, "is negative"),
                            (dict(n_sensors=5), ValueError, "the placement has 4 sensors, not 5")):
        with pytest.raises(error, match=what):
            utils.PXDDoubletStatistics(p, g, **dict(dict(n_sensors=4), **kw))
    with pytest.raises(TypeError, match="expects a PXDPlacement and a PXDGeometry"):
        utils.PXDDoubletStatistics(g, p, n_sensors=4)
    acc = utils.PXDDoubletStatistics(p, g, n_sensors=4)
    assert (acc.tan_q12, acc.z0_sub) == (1267, 320000) and acc.tables is None and acc.hits == []
    with pytest.raises(RuntimeError, match="PXDDoubletStatistics.result.. before any update"):
        acc.result()


def test_validate_refuses_bad_doublet_arguments():
    import validate
    base = ["--compare", "somewhere", "--synthetic", "2", "--resolution", "64", "--H_base", "1"]
    for extra, what in ((["--dphi", "0.2"], "--dphi needs --doublets"), (["--z0", "5"], "--z0 needs --doublets"),
                        (["--uniform_pitch", "50", "60"], "--uniform_pitch needs --doublets"), (["--doublets", "--dphi", "0"], "--dphi / --z0: .*tan_q12"),
                        (["--doublets", "--z0", "-1"], "--dphi / --z0: .*z0_sub"), (["--doublets"], "give the cell size with --uniform_pitch"),
                        (["--doublets", "--uniform_pitch", "50.25", "60"], "multiple of 0.5 um")):
        with pytest.raises(SystemExit, match=what):
            validate.run(base + extra)
    with pytest.raises(SystemExit):                         # argparse: one value
        validate.run(base + ["--doublets", "--dphi"])
