"""Cluster-level validation, host side: the checker (tests/pxd_clusters_reference.py) against ``scipy.ndimage.label``, the C ABI of the
cluster kernels, ``utils.pxd_cluster_distance`` on hand-built tables and the bin rules at their edges (no GPU needed).  The device side
is tests/test_pxd_clusters_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import pxd_clusters_reference as CR
import pxd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("threshold", [0.0, 7.0])
@pytest.mark.parametrize("case", ["structured_4x64x96", "random_7x13x37"])
def test_checker_equals_scipy_label(case, kind, threshold):
    pytest.importorskip("scipy")
    if case == "structured_4x64x96":
        ev, _ = CR.cached_structured(4, 64, 96, 21, kind)
    else:
        ev = (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(7, 13, 37, seed=32, p_hit=0.3)
    cl = CR.clusters(ev, threshold)
    labels, total = CR.scipy_labels(ev, threshold)
    print(f"{case} {kind} cut {threshold}: digits {cl['label'].size} clusters {cl['total']} (scipy {total}) largest {cl['size'].max()}")
    assert cl["total"] == total and cl["label"].size == labels.size
    assert np.array_equal(cl["label"], labels)                         # same components AND same numbering
    assert np.array_equal(cl["size"], np.bincount(labels, minlength=total))
    assert cl["size"].sum() == labels.size and cl["counts"].sum() == total
    assert np.array_equal(cl["first"], cl["index"][np.unique(labels, return_index=True)[1]])
    if case == "random_7x13x37" and threshold == 0.0:
        assert cl["size"].max() >= 20                                  # p_hit = 0.3: real multi-pixel clusters, not singletons


def test_structured_event_holds_its_shapes():
    ev, plants = CR.cached_structured(4, 64, 96, 21, "f32")
    cl = CR.clusters(ev, 0.0)
    at = lambda name: int(cl["label"][np.searchsorted(cl["index"], plants[name][0])])
    for name in ("snake", "spiral", "u", "diagonal", "corner0_3", "corner1_3", "corner2_3", "corner3_3"):
        assert cl["size"][at(name)] == plants[name][1], name
    assert plants["snake"][1] == 21 * 96 + 20 and cl["size_u"][at("snake")] == 41 and cl["size_v"][at("snake")] == 96
    assert cl["seed"][at("snake")] == 255
    d = at("diagonal")
    assert cl["size_u"][d] == cl["size_v"][d] == cl["size"][d] == 62
    for pair in ("wrap", "image", "column"):
        assert at(pair + "_a") != at(pair + "_b"), pair
        assert abs(plants[pair + "_a"][0] - plants[pair + "_b"][0]) in (1, 96)          # adjacent in flat index / one row apart
    cut = CR.clusters(ev, 7.0)
    pos = np.searchsorted(cut["index"], plants["diagonal"][0])
    assert cut["size"][cut["label"][pos]] == 31 and cl["size"][d] == 62                    # the 6.9 ADU pixel splits the chain at the cut


def test_cluster_entry_points_are_declared_exported_and_bound():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for sym in ("ieagan_pxd_clusters", "ieagan_pxd_clusters_scratch", "ieagan_pxd_cluster_stats"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTS and sym in _hip._SIGS, sym
    assert len(_hip._SIGS["ieagan_pxd_clusters"]) == 18 and _hip._SIGS["ieagan_pxd_clusters"][6] is ctypes.c_long
    assert len(_hip._SIGS["ieagan_pxd_cluster_stats"]) == 16
    lib.ieagan_abi_version.restype = ctypes.c_int
    assert lib.ieagan_abi_version() == _hip.ABI_VERSION == 12
    assert re.search(r"#define\s+IEAGAN_ABI_VERSION\s+12\b", header)
    lib.ieagan_pxd_clusters_scratch.restype = ctypes.c_long
    lib.ieagan_pxd_clusters_scratch.argtypes = [ctypes.c_int] * 3 + [ctypes.c_long]
    for cap in (0, 1, 1000, 480000, 40 * 250 * 768):
        s = lib.ieagan_pxd_clusters_scratch(40, 250, 768, cap)
        assert 9 * cap < s <= 9 * cap + 4096, (cap, s)                  # parent, rank, seven accumulators a digit; the wave slots
    assert lib.ieagan_pxd_clusters_scratch(0, 250, 768, 10) == 0
    assert sum(n for _, n in _hip.PXD_CLUSTER_COLUMNS.values()) == _hip.PXD_CLUSTER_BINS == 640


def test_launchers_reject_bad_arguments_before_any_launch():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    lib.ieagan_last_error.restype = ctypes.c_char_p
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    buf = (ctypes.c_longlong * 64)()
    a = ctypes.addressof(buf)
    fn = lib.ieagan_pxd_clusters
    fn.argtypes, fn.restype = [vp, vp, vp, i, i, i, l] + [vp] * 11, i
    good = dict(index=a, charge=a, digit_total=a, N=1, H=2, W=2, capacity=4, label=a, first=a, size=a, ccharge=a, seed=a, size_u=a, size_v=a,
                counts=a, total=a, scratch=a, stream=None)
    bad = [(dict(N=0), "N = 0"), (dict(H=0), "bad image size"), (dict(N=40000, H=250, W=768), "int32 flat index"),
           (dict(H=4096, W=4096), "int32 cluster charge"), (dict(capacity=-1), "negative"), (dict(digit_total=None), "digit_total"),
           (dict(index=None), "index / charge is NULL"), (dict(seed=None), "output table is NULL"), (dict(label=a + 2), "4-byte aligned"),
           (dict(counts=None), "counts / total"), (dict(scratch=None), "scratch")]
    for over, msg in bad:
        assert fn(*dict(good, **over).values()) != 0, over
        assert msg in lib.ieagan_last_error().decode(), (over, lib.ieagan_last_error().decode())
    fn = lib.ieagan_pxd_cluster_stats
    fn.argtypes, fn.restype = [vp] * 8 + [i, i, i, i, l, vp, vp, vp], i
    good = dict(first=a, size=a, ccharge=a, seed=a, size_u=a, size_v=a, cluster_total=a, digit_total=a, N=4, H=2, W=2, n_sensors=2, capacity=4,
                tables=a, overflow=a, stream=None)
    bad = [(dict(N=3), "not a multiple"), (dict(n_sensors=0), "not a multiple"), (dict(first=None), "cluster table is NULL"),
           (dict(cluster_total=None), "cluster_total"), (dict(tables=a + 4), "8-byte aligned"), (dict(overflow=None), "8-byte aligned")]
    for over, msg in bad:
        assert fn(*dict(good, **over).values()) != 0, over
        assert msg in lib.ieagan_last_error().decode(), (over, lib.ieagan_last_error().decode())


def _tables(size_bins, charge_bins, seed_bins, clusters, S=2):
    """Hand-built ``PXDClusterStatistics.result()`` tables: ``*_bins`` = list of (sensor, bin, count)."""
    t = dict(size_spectrum=np.zeros((S, 64), np.int64), charge_spectrum=np.zeros((S, 256), np.int64), seed_spectrum=np.zeros((S, 256), np.int64),
             size_u_spectrum=np.zeros((S, 32), np.int64), size_v_spectrum=np.zeros((S, 32), np.int64), clusters=np.asarray(clusters, np.int32))
    for key, items in (("size_spectrum", size_bins), ("charge_spectrum", charge_bins), ("seed_spectrum", seed_bins)):
        for s, b, n in items:
            t[key][s, b] += n
    return t


def test_cluster_distance_on_hand_built_tables():
    import utils
    a = _tables([(0, 0, 6), (1, 2, 2)], [(0, 10, 3), (1, 20, 5)], [(0, 100, 4), (1, 30, 4)], [[3, 1], [5, 3]])
    d = utils.pxd_cluster_distance(a, a)
    assert d == dict(cluster_rate_rel_err=0.0, size_w1=0.0, cluster_charge_w1=0.0, seed_w1=0.0)
    # every spectrum moved up by one bin: one pixel, 8 ADU, one ADU
    b = _tables([(0, 1, 6), (1, 3, 2)], [(0, 11, 3), (1, 21, 5)], [(0, 101, 4), (1, 31, 4)], [[3, 1], [5, 3]])
    d = utils.pxd_cluster_distance(a, b)
    assert d["size_w1"] == 1.0 and d["cluster_charge_w1"] == 8.0 and d["seed_w1"] == 1.0 and d["cluster_rate_rel_err"] == 0.0
    # pooled over the sensors and normalised: real = {bin 0: 3/4, bin 2: 1/4}, fake = {bin 0: 1/4, bin 2: 3/4} -> |CDF difference| = 1/2 in
    # bins 0 and 1 -> W1 = 1; the counts of the two sides differ by a factor that must not matter
    c = _tables([(0, 0, 10), (1, 2, 30)], [(0, 10, 1)], [(0, 100, 1)], [[2, 4], [2, 4]])
    assert utils.pxd_cluster_distance(a, c)["size_w1"] == 1.0
    # rate: real means (4, 2) clusters per image, fake (2, 4): relative errors 1/2 and 1 -> mean 3/4
    assert utils.pxd_cluster_distance(a, c)["cluster_rate_rel_err"] == 0.75
    # a sensor without real clusters does not count; a side without any cluster gives NaN distances
    e = _tables([(0, 0, 1)], [(0, 0, 1)], [(0, 9, 1)], [[1, 0]])
    f = _tables([(0, 0, 1)], [(0, 0, 1)], [(0, 9, 1)], [[2, 7]])
    assert utils.pxd_cluster_distance(e, f)["cluster_rate_rel_err"] == 1.0
    z = _tables([], [], [], [[0, 0]])
    d = utils.pxd_cluster_distance(e, z)
    assert np.isnan(d["size_w1"]) and np.isnan(d["cluster_charge_w1"]) and np.isnan(d["seed_w1"]) and d["cluster_rate_rel_err"] == 1.0
    assert np.isnan(utils.pxd_cluster_distance(z, e)["cluster_rate_rel_err"])


def test_bin_rules_at_their_edges():
    assert CR.size_bin([1, 2, 63, 64, 65, 192000]).tolist() == [0, 1, 62, 63, 63, 63]
    assert CR.charge_bin([0, 7, 8, 2039, 2040, 2047, 2048, 48960000]).tolist() == [0, 0, 1, 254, 255, 255, 255, 255]
    assert CR.extent_bin([1, 31, 32, 33, 768]).tolist() == [0, 30, 31, 31, 31]
    # the same rules through the spectra of a hand-built cluster table: two sensors, clusters of image 0 and image 3 (sensor 1)
    cl = dict(first=np.array([0, 3, 3 * 4 + 1], np.int32), size=np.array([63, 64, 65], np.int32), charge=np.array([2039, 2040, 2048], np.int32),
              seed=np.array([0, 255, 7], np.uint8), size_u=np.array([32, 33, 1], np.int32), size_v=np.array([1, 32, 33], np.int32),
              counts=np.array([2, 0, 0, 1], np.int32))
    sp = CR.spectra(cl, (4, 2, 2), 2)
    assert sp["size_spectrum"][0, 62] == 1 and sp["size_spectrum"][0, 63] == 1 and sp["size_spectrum"][1, 63] == 1
    assert sp["charge_spectrum"][0, 254] == 1 and sp["charge_spectrum"][0, 255] == 1 and sp["charge_spectrum"][1, 255] == 1
    assert sp["seed_spectrum"][0, 0] == 1 and sp["seed_spectrum"][0, 255] == 1 and sp["seed_spectrum"][1, 7] == 1
    assert sp["size_u_spectrum"][0, 31] == 2 and sp["size_u_spectrum"][1, 0] == 1
    assert sp["size_v_spectrum"][0, 0] == 1 and sp["size_v_spectrum"][0, 31] == 1 and sp["size_v_spectrum"][1, 31] == 1
    assert all(sp[k].sum() == 3 for k in sp if k != "clusters") and sp["clusters"].tolist() == [[2, 0], [0, 1]]


def test_cluster_surface_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import utils
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils.pxd_clusters(torch.zeros(40, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils.PXDClusterStatistics().update(torch.zeros(40, 4, 4))
