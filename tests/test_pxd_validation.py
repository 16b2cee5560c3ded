"""Detector-level validation, host side: the C ABI of the statistics kernel, the bin rule, the three distances and the new
train options (no GPU needed).  The device side is tests/test_pxd_validation_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pxd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pxd_stats_is_declared_exported_and_bound():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for sym in ("ieagan_pxd_stats", "ieagan_pxd_stats_scratch"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTS and sym in _hip._SIGS, sym
    lib.ieagan_abi_version.restype = ctypes.c_int
    assert lib.ieagan_abi_version() == _hip.ABI_VERSION == 12
    assert int(re.search(r"#define IEAGAN_ABI_VERSION (\d+)", header).group(1)) == 12
    # the scratch query is plain host code: two 4-byte words per (image, workgroup of the image), a capped grid
    lib.ieagan_pxd_stats_scratch.restype = ctypes.c_long
    lib.ieagan_pxd_stats_scratch.argtypes = [ctypes.c_int] * 3
    for n, h, w in ((40, 250, 768), (80, 250, 768), (7, 13, 37), (40, 58, 64)):
        s = lib.ieagan_pxd_stats_scratch(n, h, w)
        assert s > 0 and s % (2 * n) == 0 and (s // 2) <= 2048 + n, (n, h, w, s)
    assert lib.ieagan_pxd_stats_scratch(0, 250, 768) == 0


def test_bin_edges_and_index_rule_equal_numpy_histogram():
    import utils
    edges = utils.pxd_bin_edges()
    assert edges.shape == (252,) and edges.dtype == np.float64
    assert np.array_equal(edges, np.array([-1.0, 1.0, 7.0] + list(np.linspace(8, 256, 249))))
    assert np.array_equal(edges, R.EDGES)
    f = np.float32
    vals = []
    for e in edges:                 # every edge value and its float32 neighbours, inside the histogram's range
        vals += [f(e), np.nextafter(f(e), f(-10)), np.nextafter(f(e), f(1000))]
    vals += [f(0), f(0.999), f(6.78), f(6.99), f(7.5), f(254.99)]
    vals = np.array([v for v in vals if -1 <= v <= 256], np.float32)
    assert len(vals) > 740
    idx = utils.pxd_bin_index(vals)
    for v, b in zip(vals, idx):
        h = np.histogram(np.array([v], np.float64), edges)[0]
        assert h.sum() == 1 and h[b] == 1, (v, b, int(np.argmax(h)))
    u8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(np.bincount(utils.pxd_bin_index(u8), minlength=251), np.histogram(u8, edges)[0])


def _tables(hit_values, n_sensors=4, pixels=10000, events=1):
    """Hand-made result tables: every sensor of every event carries the same hits ``hit_values`` (ADU) on ``pixels`` pixels."""
    import utils
    hv = np.asarray(hit_values, np.float64)
    spec = np.bincount(utils.pxd_bin_index(hv), minlength=251).astype(np.int64)
    spec[0] += pixels - len(hv)
    return dict(spectrum=np.tile(spec * events, (n_sensors, 1)), occupancy=np.full(n_sensors, len(hv) / pixels),
                mean_charge=np.full(n_sensors, hv.mean()), n_events=events)


def test_pxd_distance_on_hand_made_tables():
    import utils
    rng = np.random.Generator(np.random.PCG64(5))
    hv = rng.integers(8, 201, 500).astype(np.float64)
    a = _tables(hv)
    d = utils.pxd_distance(a, _tables(hv))
    assert d == {"occ_rel_err": 0.0, "charge_rel_err": 0.0, "spectrum_w1": 0.0}
    d = utils.pxd_distance(a, _tables(hv + 10))
    assert abs(d["spectrum_w1"] - 10.0) <= 1e-12, d
    assert d["occ_rel_err"] == 0.0 and abs(d["charge_rel_err"] - 10.0 / hv.mean()) <= 1e-12
    d = utils.pxd_distance(a, _tables(np.concatenate([hv, hv])))          # twice the hits in every sensor
    assert d["occ_rel_err"] == 1.0 and d["charge_rel_err"] == 0.0 and d["spectrum_w1"] == 0.0
    # sensors without real hits do not enter the means; a fake sensor without a hit counts with charge 0
    b = _tables(hv)
    a2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    a2["occupancy"][0], a2["mean_charge"][0] = 0.0, np.nan
    b["mean_charge"][1] = np.nan
    d = utils.pxd_distance(a2, b)
    assert d["occ_rel_err"] == 0.0 and abs(d["charge_rel_err"] - 1.0 / 3.0) <= 1e-15


def test_restatement_on_a_hand_counted_image():
    """The checker itself on an image small enough to count by hand."""
    img = np.zeros((2, 2, 3), np.float32)
    img[0] = [[0.0, 6.9, 7.0], [8.5, 255.0, 0.5]]
    img[1] = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    s = R.get_stats(img, n_sensors=2)
    assert s["hits"].tolist() == [[3, 0]] and s["charge"][0, 0] == 7.0 + 8.5 + 255.0
    assert s["spectrum"][0, 0] == 3 and s["spectrum"][0, 2] == 1 and s["spectrum"][0, 3] == 1 and s["spectrum"][0, 250] == 1
    assert s["spectrum"][1].tolist() == [6] + [0] * 250
    assert s["occupancy"].tolist() == [0.5, 0.0] and s["mean_charge"][0] == (7.0 + 8.5 + 255.0) / 3 and np.isnan(s["mean_charge"][1])
    assert s["occ_overflow"] == 1 and s["occ_hist"][0] == 1 and s["occ_hist"].sum() == 1


def test_validation_options_are_typed_and_off_by_default():
    import train
    from defaults import default_config
    c = default_config()
    assert (c["val_every"], c["val_events"], c["val_threshold"]) == (0, 100, 7.0)
    assert type(c["val_every"]) is int and type(c["val_events"]) is int and type(c["val_threshold"]) is float
    cfg = train.parse(["--val_every", "2", "--val_events", "3"])
    assert cfg["val_every"] == 2 and type(cfg["val_every"]) is int
    assert cfg["val_events"] == 3 and type(cfg["val_events"]) is int
    assert cfg["val_threshold"] == 7.0
    assert train.parse(["--val_threshold", "5"])["val_threshold"] == 5.0


def test_statistics_have_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import utils
    acc = utils.PXDStatistics(n_sensors=2, threshold=7.0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.update(torch.zeros(2, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        acc.result()
