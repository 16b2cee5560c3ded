"""Cluster reconstruction, host side: the checker (tests/pxd_reco_reference.py) against ``scipy.ndimage.center_of_mass``, the integer bin
rule at its edges, the C ABI of the reconstruction kernels and ``utils.pxd_map_distance`` on hand-built tables (no GPU needed).  The
device side is tests/test_pxd_reco_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import pxd_clusters_reference as CR
import pxd_reco_reference as RR
import pxd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _hip, ctypes.CDLL(_hip.LIB_PATH)


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("threshold", [0.0, 7.0])
@pytest.mark.parametrize("case", ["structured_4x64x96", "random_7x13x37"])
def test_checker_equals_scipy_center_of_mass(case, kind, threshold):
    """Observed here: EQUAL after rounding both to float32 in every case (scipy sums q * r and q in float64, where the integer sums are
    exact, and divides once), so the test asserts equality and does not use the 1-ulp allowance."""
    ndimage = pytest.importorskip("scipy.ndimage")
    if case == "structured_4x64x96":
        ev, _ = CR.cached_structured(4, 64, 96, 21, kind)
    else:
        ev = (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(7, 13, 37, seed=32, p_hit=0.3)
    cl, pos = RR.reco(ev, threshold)
    n, h, w = ev.shape
    assert pos["total"] == cl["total"] > 0 and np.array_equal(pos["cluster"], np.arange(cl["total"]))      # no cut: every cluster, in order
    q = RR.dense_charge(cl, ev.shape).astype(np.float64)
    lab = np.zeros(ev.size, np.int64)
    lab[cl["index"].astype(np.int64)] = cl["label"].astype(np.int64) + 1
    lab = lab.reshape(ev.shape)
    image = cl["first"].astype(np.int64) // (h * w)
    worst = 0
    for k in range(n):
        ids = np.nonzero(image == k)[0]
        if ids.size == 0:
            continue
        com = np.asarray(ndimage.center_of_mass(q[k], lab[k], ids + 1), np.float64).reshape(-1, 2).astype(np.float32)
        for got, want in ((pos["u"][ids], com[:, 0]), (pos["v"][ids], com[:, 1])):
            worst = max(worst, int(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()))
    print(f"{case} {kind} cut {threshold}: {cl['total']} clusters, largest difference to scipy {worst} ulp of float32")
    assert worst == 0
    # a position lies inside the extent of its cluster
    assert (pos["u"] >= 0).all() and (pos["u"] <= h - 1).all() and (pos["v"] >= 0).all() and (pos["v"] <= w - 1).all()


def test_cut_keeps_cluster_order_and_counts():
    ev, _ = CR.cached_structured(4, 64, 96, 21, "u8")
    cl, every = RR.reco(ev, 0.0)
    _, some = RR.reco(ev, 0.0, seed_cut=100, charge_cut=150)
    keep = (cl["seed"] >= 100) & (cl["charge"] >= 150)
    assert 0 < some["total"] == keep.sum() < every["total"] and np.array_equal(some["cluster"], np.nonzero(keep)[0])
    assert np.array_equal(some["u"], every["u"][keep]) and np.array_equal(some["v"], every["v"][keep])
    assert some["counts"].sum() == some["total"] and (some["counts"] <= cl["counts"]).all()
    _, none = RR.reco(ev, 0.0, seed_cut=256)
    assert none["total"] == 0 and none["cluster"].size == 0 and (none["counts"] == 0).all()


def test_bin_rule_at_its_edges():
    h, w = 250, 768
    px = [(9, 5, 10), (10, 5, 10),              # two pixels of equal charge straddling row 10: u = 9.5 -> bin 0
          (10, 100, 77),                        # u = 10.0: exactly on the edge -> bin 1;  v = 100 -> bin 6
          (40, 15, 8), (40, 16, 8),             # v = 15.5 -> bin 0
          (60, 16, 9),                          # v = 16.0: exactly on the edge -> bin 1
          (249, 767, 255),                      # u = H - 1 -> bin 24, v = W - 1 -> bin 47
          (0, 300, 1)]                          # u = 0 -> bin 0
    index = np.array(sorted(r * w + c for r, c, _ in px), np.int32)
    charge = np.array([q for _, _, q in sorted(px, key=lambda t: t[0] * w + t[1])], np.uint8)
    cl = CR.clusters_of_digits(index, charge, (1, h, w))
    pos = RR.positions(cl, (1, h, w))
    assert cl["total"] == 6
    assert pos["u"].tolist() == [0.0, 9.5, 10.0, 40.0, 60.0, 249.0] and pos["v"].tolist() == [300.0, 5.0, 100.0, 15.5, 16.0, 767.0]
    bu, bv = RR.bins(pos["mu"], pos["mv"], cl["charge"], h, w)
    assert bu.tolist() == [0, 0, 1, 4, 6, 24] and bv.tolist() == [18, 0, 6, 0, 1, 47]
    # the float form of the rule would put the same clusters into the same bins here; the integer form does not depend on that
    assert np.array_equal(bu, np.floor(pos["u"].astype(np.float64) / h * 25)) and np.array_equal(bv, np.floor(pos["v"].astype(np.float64) / w * 48))
    m = RR.maps(cl, pos, (1, h, w), 1)
    assert m["count_map"].sum() == 6 and m["count_map"][0, 0, 0] == 1 and m["count_map"][0, 24, 47] == 1 and m["charge_map"][0, 0, 0] == 20
    assert m["charge_map"].sum() == int(charge.sum()) and m["u_profile"][0, 0] == 2 and m["v_profile"][0, 0] == 2
    assert m["clusters"].tolist() == [[6]]


def test_moments_need_64_bits():
    """The figures of the all-hit image of the cluster tests, computed on the host: any narrower accumulation wraps."""
    ev = np.random.Generator(np.random.PCG64(2)).integers(8, 255, (1, 250, 768))
    ev[0, 100, 300] = 255
    q = ev[0].astype(np.int64)
    mu, mv = int((q * np.arange(250)[:, None]).sum()), int((q * np.arange(768)[None, :]).sum())
    assert mu == 3138994938 > 2 ** 31 and mv == 9666396989 > 2 ** 32


def test_reco_entry_points_are_declared_exported_and_bound():
    _hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    for sym in ("ieagan_pxd_cluster_positions", "ieagan_pxd_cluster_positions_scratch", "ieagan_pxd_cluster_maps"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTS and sym in _hip._SIGS, sym
    assert len(_hip._SIGS["ieagan_pxd_cluster_positions"]) == 23 and _hip._SIGS["ieagan_pxd_cluster_positions"][11] is ctypes.c_long
    assert len(_hip._SIGS["ieagan_pxd_cluster_maps"]) == 17 and _hip._SIGS["ieagan_pxd_cluster_maps"][12] is ctypes.c_long
    lib.ieagan_abi_version.restype = ctypes.c_int
    assert lib.ieagan_abi_version() == _hip.ABI_VERSION == 12
    assert re.search(r"#define\s+IEAGAN_ABI_VERSION\s+12\b", header)
    lib.ieagan_pxd_cluster_positions_scratch.restype = ctypes.c_long
    lib.ieagan_pxd_cluster_positions_scratch.argtypes = [ctypes.c_int] * 3 + [ctypes.c_long]
    for cap in (0, 1, 1000, 480000, 40 * 250 * 768):
        assert 4 <= lib.ieagan_pxd_cluster_positions_scratch(40, 250, 768, cap) <= 4096, cap         # the wave slots alone
    assert lib.ieagan_pxd_cluster_positions_scratch(0, 250, 768, 10) == 0
    assert (_hip.PXD_MAP_U, _hip.PXD_MAP_V) == (RR.MAP_U, RR.MAP_V) == (25, 48)
    import utils
    for name in ("pxd_cluster_positions", "PXDClusterPositions", "PXDClusterMaps", "pxd_map_distance"):
        assert hasattr(utils, name), name


def test_reco_launchers_reject_bad_arguments_before_any_launch():
    _, lib = _lib()
    lib.ieagan_last_error.restype = ctypes.c_char_p
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    buf = (ctypes.c_longlong * 64)()
    a = ctypes.addressof(buf)
    fn = lib.ieagan_pxd_cluster_positions
    fn.argtypes, fn.restype = [vp] * 8 + [i, i, i, l, i, i] + [vp] * 9, i
    good = dict(index=a, charge=a, label=a, digit_total=a, first=a, ccharge=a, seed=a, cluster_total=a, N=1, H=2, W=2, capacity=4, seed_cut=0,
                charge_cut=0, mu=a, mv=a, cluster=a, u=a, v=a, counts=a, total=a, scratch=a, stream=None)
    bad = [(dict(N=0), "N = 0"), (dict(H=0), "bad image size"), (dict(N=40000, H=250, W=768), "int32 flat index"),
           (dict(H=4096, W=4096), "int32 cluster charge"), (dict(capacity=-1), "negative"), (dict(seed_cut=-1), "seed_cut = -1"),
           (dict(charge_cut=-5), "charge_cut = -5"), (dict(digit_total=None), "digit_total / cluster_total"),
           (dict(cluster_total=None), "digit_total / cluster_total"), (dict(label=None), "index / charge / label is NULL"),
           (dict(seed=None), "cluster table is NULL"), (dict(mu=None), "output array is NULL"), (dict(u=None), "output array is NULL"),
           (dict(cluster=a + 2), "4-byte aligned"), (dict(mv=a + 4), "8-byte aligned"), (dict(counts=None), "counts / total"),
           (dict(scratch=None), "scratch")]
    for over, msg in bad:
        assert fn(*dict(good, **over).values()) != 0, over
        assert msg in lib.ieagan_last_error().decode(), (over, lib.ieagan_last_error().decode())
    fn = lib.ieagan_pxd_cluster_maps
    fn.argtypes, fn.restype = [vp] * 8 + [i, i, i, i, l] + [vp] * 4, i
    good = dict(cluster=a, accepted_total=a, first=a, ccharge=a, mu=a, mv=a, cluster_total=a, digit_total=a, N=4, H=2, W=2, n_sensors=2,
                capacity=4, count=a, charge=a, overflow=a, stream=None)
    bad = [(dict(N=3), "not a multiple"), (dict(n_sensors=0), "not a multiple"), (dict(capacity=-1), "negative"),
           (dict(cluster=None), "is NULL with capacity"), (dict(mu=None), "is NULL with capacity"), (dict(mv=a + 4), "8-byte aligned"),
           (dict(accepted_total=None), "accepted_total"), (dict(digit_total=None), "accepted_total"), (dict(count=a + 4), "8-byte aligned"),
           (dict(charge=None), "8-byte aligned"), (dict(overflow=None), "8-byte aligned")]
    for over, msg in bad:
        assert fn(*dict(good, **over).values()) != 0, over
        assert msg in lib.ieagan_last_error().decode(), (over, lib.ieagan_last_error().decode())


def _tables(cells, clusters, S=2, shape=(250, 768)):
    """Hand-built ``PXDClusterMaps.result()`` tables: ``cells`` = list of (sensor, u bin, v bin, count)."""
    count = np.zeros((S, 25, 48), np.int64)
    for s, bu, bv, n in cells:
        count[s, bu, bv] += n
    return dict(count_map=count, charge_map=10 * count, u_profile=count.sum(2), v_profile=count.sum(1), clusters=np.asarray(clusters, np.int32),
                n_events=len(clusters), shape=shape)


def test_map_distance_on_hand_built_tables():
    import utils
    a = _tables([(0, 0, 0, 6), (0, 3, 10, 2), (1, 24, 47, 4)], [[5, 1], [3, 3]])
    assert utils.pxd_map_distance(a, a) == dict(accepted_rate_rel_err=0.0, u_profile_w1=0.0, v_profile_w1=0.0, map_tv=0.0)
    # every cluster one u bin further (the last one bin back): the pooled u profile moves by one bin of 250 / 25 = 10 pixels for 8 of 12
    # clusters up and 4 of 12 down; the v profile does not move; no sensor shares a cell with itself: total variation 1
    b = _tables([(0, 1, 0, 6), (0, 4, 10, 2), (1, 23, 47, 4)], [[5, 1], [3, 3]])
    d = utils.pxd_map_distance(a, b)
    assert d["u_profile_w1"] == pytest.approx(10.0, abs=1e-12) and d["v_profile_w1"] == 0.0 and d["map_tv"] == 1.0
    assert d["accepted_rate_rel_err"] == 0.0
    # one v bin of 768 / 48 = 16 pixels for everything; the counts of the two sides differ by a factor that must not matter
    c = _tables([(0, 0, 1, 60), (0, 3, 11, 20), (1, 24, 46, 40)], [[5, 1], [3, 3]])
    d = utils.pxd_map_distance(a, c)
    assert d["u_profile_w1"] == 0.0 and d["map_tv"] == 1.0
    # pooled: 2/3 of the clusters move up one bin and 1/3 down one bin -> |CDF difference| sums to 2/3 + 1/3 = 1 bin
    assert d["v_profile_w1"] == pytest.approx(16.0, abs=1e-12)
    # total variation of one sensor: real {A: 3/4, B: 1/4}, fake {A: 1/4, B: 3/4} -> 0.5 * (1/2 + 1/2) = 1/2; the other sensor equal -> mean 1/4
    e = _tables([(0, 2, 2, 3), (0, 5, 5, 1), (1, 7, 7, 2)], [[4, 2]])
    f = _tables([(0, 2, 2, 1), (0, 5, 5, 3), (1, 7, 7, 8)], [[4, 2]])
    assert utils.pxd_map_distance(e, f)["map_tv"] == 0.25
    # rate: real means (4, 2) per image, fake (2, 4): relative errors 1/2 and 1 -> 3/4
    g = _tables([(0, 2, 2, 3), (0, 5, 5, 1), (1, 7, 7, 2)], [[2, 4]])
    assert utils.pxd_map_distance(e, g)["accepted_rate_rel_err"] == 0.75
    # a fake sensor without a cluster counts as 1; a sensor without real clusters does not count at all
    h = _tables([(0, 2, 2, 3), (0, 5, 5, 1)], [[4, 0]])
    d = utils.pxd_map_distance(e, h)
    assert d["map_tv"] == 0.5 and d["accepted_rate_rel_err"] == 0.5
    d = utils.pxd_map_distance(h, e)
    assert d["map_tv"] == 0.0 and d["accepted_rate_rel_err"] == 0.0
    # a side without any cluster: NaN profiles; no real cluster at all: everything NaN
    z = _tables([], [[0, 0]])
    d = utils.pxd_map_distance(e, z)
    assert np.isnan(d["u_profile_w1"]) and np.isnan(d["v_profile_w1"]) and d["map_tv"] == 1.0 and d["accepted_rate_rel_err"] == 1.0
    d = utils.pxd_map_distance(z, e)
    assert all(np.isnan(v) for v in d.values()) and set(d) == {"accepted_rate_rel_err", "u_profile_w1", "v_profile_w1", "map_tv"}


def test_reco_surface_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import utils
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils.pxd_cluster_positions(torch.zeros(40, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils.PXDClusterMaps().update(torch.zeros(40, 4, 4))
    with pytest.raises(ValueError, match="negative"):
        utils.PXDClusterMaps(seed_cut=-1)
