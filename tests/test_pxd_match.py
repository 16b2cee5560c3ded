"""Signal-hit matching, host side: the two forms of the checker (tests/pxd_match_reference.py) agree on the planted overlay pairs and on
structured events under a sparse background, and have the properties the rule promises (a true overlay loses no digit and splits no
cluster; an empty background changes nothing; a planted background pixel, a saturating one and a planted bridge are flagged as such; two
unrelated events lose hits); the bin rules against ``fractions.Fraction`` and the stated float64 recipe; the C ABI of the three entry
points, the launchers' refusals and the host-side refusals of ``utils.pxd_match`` (no GPU needed).  The device side is
tests/test_pxd_match_gpu.py."""
import ctypes
import os
import re
import subprocess
import sys
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

import pxd_hits_reference as HR
import pxd_match_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 13, 37), (2, 40, 259)]


def _both_forms(signal, mixed, geometry, **kw):
    m = MR.match(signal, mixed, geometry, **kw)
    assert MR.same_tables(m["clusters"], MR.dense(m["cs"], m["cm"], m["shape"]))
    return m


def _is_true_overlay(m):
    """A connected set stays connected in a superset: every digit found, in one mixed cluster; every hit matched to a hit."""
    pc, cs, h = m["clusters"], m["cs"], m["hits"]
    assert np.array_equal(pc["found"], cs["size"]) and np.array_equal(pc["lo"], pc["hi"]) and (pc["lo"] >= 0).all()
    assert pc["signal_size"].sum() == cs["index"].size and pc["signal_charge"].sum() == cs["digit_charge"].astype(np.int64).sum()
    assert (pc["signal_size"] <= m["cm"]["size"]).all() and (pc["signal_charge"] <= m["cm"]["charge"]).all()
    assert pc["n_signal"].sum() == cs["total"]
    assert h["matched"].all() and (h["mixed_hit"] >= 0).all()
    same = h["matched"] & ~h["changed"]
    assert (h["du"][same] == 0).all() and (h["dv"][same] == 0).all()         # the same integer moments go in


@pytest.mark.parametrize("S,H,W", SHAPES)
def test_the_two_forms_agree_on_the_planted_overlay_pairs(S, H, W):
    m = MR.cached_match("planted", S, H, W)
    assert MR.same_tables(m["clusters"], MR.dense(m["cs"], m["cm"], m["shape"]))
    _is_true_overlay(m)
    h = m["hits"]
    # the planted pairs show every outcome: unchanged, changed and shared hits
    assert (~h["changed"]).any() and h["changed"].any() and h["shared"].any() and (h["n_signal"] >= 2).any()
    assert np.array_equal(h["shared"], h["n_signal"] >= 2)
    # pair 2 (random + empty): nothing changes; pair 3 (an event over itself): every cluster keeps its pixels and gains charge
    # (a pixel of 255 stays 255)
    e3 = h["event"] == 3
    assert not h["changed"][h["event"] == 2].any() and h["changed"][e3].any()
    assert np.array_equal(h["signal_size"][e3], h["size"][e3]) and np.array_equal(h["changed"][e3], h["mixed_charge"][e3] > h["charge"][e3])
    t = MR.tables(h, S)
    assert np.array_equal(t[:, 0], t[:, 1] + t[:, 4]) and t[:, 4].sum() == 0 and t[:, 0].sum() == h["cluster"].size
    assert t[:, MR.RES_U:MR.RES_V].sum() == t[:, MR.RES_V:MR.PURITY].sum() == t[:, 2].sum() and t[:, MR.PURITY:].sum() == t[:, 1].sum()


def test_the_two_forms_agree_on_structured_events_under_a_sparse_background():
    S, H, W = 2, 40, 259
    for threshold, cuts in ((0.0, (0, 0)), (7.0, (20, 30))):
        m = MR.cached_match("structured", S, H, W, threshold, *cuts)
        assert MR.same_tables(m["clusters"], MR.dense(m["cs"], m["cm"], m["shape"]))
        _is_true_overlay(m)
        h = m["hits"]
        big = h["size"] >= 100                                  # the snake, the spiral and the U: they span many waves of a digit walk
        assert big.sum() >= 3 and h["matched"][big].all() and h["changed"].any() and (~h["changed"]).any()


def _small(S=2, H=24, W=48):
    """Two signal clusters on sensor 0 of a 2 x 24 x 48 event, two rows apart in the same columns, and one on sensor 1."""
    x = np.zeros((S, H, W), np.uint8)
    x[0, 5, 10:13] = (30, 200, 40)
    x[0, 8, 10:13] = (25, 90, 35)
    x[1, 3, 7:9] = (60, 50)
    return x, HR.two_type_geometry((H, W), W // 3, S)


def test_an_empty_background_changes_nothing():
    for signal, geometry in (_small(), (MR.planted_case(7, 13, 37)[0], HR.two_type_geometry((13, 37), 12, 7))):
        m = _both_forms(signal, signal.copy(), geometry)
        _is_true_overlay(m)
        h = m["hits"]
        assert h["cluster"].size > 0 and (h["flags"] == MR.MATCHED).all() and not h["du"].any() and not h["dv"].any()
        assert np.array_equal(h["mixed_hit"], np.arange(h["cluster"].size)) and (h["n_signal"] == 1).all()
        assert np.array_equal(h["signal_charge"], h["charge"]) and np.array_equal(h["mixed_charge"], h["charge"])
        assert (MR.purity_bin(h["signal_charge"], h["mixed_charge"]) == 31).all()


def test_a_background_pixel_on_a_signal_pixel_changes_the_charge_alone():
    signal, geometry = _small()
    bg = np.zeros_like(signal)
    bg[0, 5, 10] = 17               # on the first pixel of cluster 0: 30 + 17
    bg[0, 8, 11] = 250              # on the seed of cluster 1: 90 + 250 saturates at 255
    m = _both_forms(signal, MR.overlay(signal, bg), geometry)
    _is_true_overlay(m)
    h = m["hits"]
    assert h["flags"].tolist() == [MR.MATCHED | MR.CHANGED, MR.MATCHED | MR.CHANGED, MR.MATCHED]
    assert np.array_equal(m["cm"]["size"], m["cs"]["size"]) and np.array_equal(h["signal_size"], h["size"])
    assert h["mixed_charge"].tolist() == [270 + 17, 150 + 165, 110] and h["signal_charge"].tolist() == [270, 150, 110]
    assert h["du"][:2].tolist() == [0.0, 0.0] and h["dv"][0] < 0 and h["dv"][1] != 0 and h["du"][2] == h["dv"][2] == 0
    # the centre of gravity moved towards the pixel that gained charge, by the float64 recipe
    want = np.float32(np.float64(m["hm"]["v"][0]) - np.float64(m["hs"]["v"][0]))
    assert h["dv"][0] == want and m["hm"]["v"][0] < m["hs"]["v"][0]


def test_a_bridge_between_two_signal_clusters_is_shared_and_changed_on_both():
    signal, geometry = _small()
    bg = np.zeros_like(signal)
    bg[0, 6:8, 11] = (9, 9)         # rows 6 and 7 between the clusters in rows 5 and 8
    m = _both_forms(signal, MR.overlay(signal, bg), geometry, head_tail=0)       # centre of gravity: the position lies between the two
    _is_true_overlay(m)
    h = m["hits"]
    both = MR.MATCHED | MR.CHANGED | MR.SHARED
    assert h["flags"].tolist() == [both, both, MR.MATCHED] and h["n_signal"].tolist() == [2, 2, 1]
    assert h["mixed_hit"].tolist() == [0, 0, 1] and h["match"].tolist() == [0, 0, 1]
    assert h["signal_size"].tolist() == [6, 6, 2] and h["signal_charge"].tolist() == [420, 420, 110] and h["mixed_charge"].tolist() == [438, 438, 110]
    assert h["du"][0] > 0 > h["du"][1]          # the merged cluster lies between the two
    t = MR.tables(h, 2)
    assert t[0, :5].tolist() == [2, 2, 2, 2, 0] and t[1, :5].tolist() == [1, 1, 0, 0, 0]


@pytest.mark.parametrize("S,H,W", SHAPES)
def test_two_unrelated_events_lose_hits(S, H, W):
    m = MR.cached_match("planted", S, H, W, unrelated=True)
    assert MR.same_tables(m["clusters"], MR.dense(m["cs"], m["cm"], m["shape"]))
    pc, h = m["clusters"], m["hits"]
    assert (pc["found"] < m["cs"]["size"]).any() and (pc["found"] == 0).any() and (pc["lo"] < pc["hi"]).any()
    assert np.array_equal(pc["lo"] == -1, pc["found"] == 0) and np.array_equal(pc["hi"] == -1, pc["found"] == 0)
    assert (~h["matched"]).any() and (h["mixed_hit"][~h["matched"]] >= -1).all()
    assert (h["du"][~h["matched"]] == 0).all() and (h["dv"][~h["matched"]] == 0).all()
    assert (h["flags"][h["match"] < 0] == 0).all() and (h["mixed_hit"][h["match"] < 0] == -1).all()
    t = MR.tables(h, S)
    assert np.array_equal(t[:, 0], t[:, 1] + t[:, 4]) and t[:, 4].sum() == (~h["matched"]).sum() > 0
    assert np.array_equal(t[:, 0], np.bincount(h["sensor"], minlength=S))


def test_with_cuts_a_match_must_itself_be_a_hit():
    """A signal cluster that passes the cuts and is found whole in a mixed cluster that does not (the unrelated mixed cluster is another
    one, with a smaller seed) has a match, no mixed hit and is lost."""
    S, H, W = 2, 24, 48
    signal, mixed = np.zeros((S, H, W), np.uint8), np.zeros((S, H, W), np.uint8)
    signal[0, 4, 4:6] = (40, 30)
    mixed[0, 4, 4:6] = (10, 12)
    m = _both_forms(signal, mixed, HR.two_type_geometry((H, W), 16, S), seed_cut=20, charge_cut=0)
    h = m["hits"]
    assert m["pm"]["total"] == 0 and h["match"].tolist() == [0] and h["found"].tolist() == [2] and h["mixed_hit"].tolist() == [-1]
    assert h["flags"].tolist() == [0] and MR.tables(h, S)[0, :5].tolist() == [1, 0, 0, 0, 1]


def test_purity_bins_against_fractions():
    rng = np.random.Generator(np.random.PCG64(5))
    qm = rng.integers(1, 2 ** 31 - 1, 4000)
    qs = np.concatenate([rng.integers(0, qm[:3000] + 1), qm[3000:] * np.arange(1000) // 999])      # 0 .. qm, both ends and k / 32 nearby
    qm[:33], qs[:33] = 32 * 1000, 1000 * np.arange(33)                                               # exactly on every bin edge
    got = MR.purity_bin(qs, qm)
    want = [min(int(32 * Fraction(int(a), int(b))), 31) for a, b in zip(qs, qm)]
    assert got.tolist() == want and got[:33].tolist() == list(range(32)) + [31] and got.min() == 0 and got.max() == 31


def test_residual_bins_against_the_float64_recipe():
    w = 10
    r = np.array([0.0, -0.0, 9.999999, 10.0, -1e-9, -10.0, -10.000001, 309.99, 310.0, 1e9, -320.0, -320.0001, -1e9, 5.0, 15.0], np.float64)
    assert MR.residual_bin(r, w).tolist() == [32, 32, 32, 33, 31, 31, 30, 62, 63, 63, 0, 0, 0, 32, 33]
    # differences of fp32 positions, as the kernel forms them
    rng = np.random.Generator(np.random.PCG64(6))
    a, b = rng.normal(0, 200, 5000).astype(np.float32), rng.normal(0, 200, 5000).astype(np.float32)
    d = a.astype(np.float64) - b.astype(np.float64)
    for w in (1, 3, 10):
        want = [min(max(int(np.floor(x / w)) + 32, 0), 63) for x in d.tolist()]
        assert MR.residual_bin(d, w).tolist() == want and min(want) == 0 and max(want) == 63


def _lib():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    lib.ieagan_last_error.restype = ctypes.c_char_p
    return _hip, lib


SYMBOLS = ("ieagan_pxd_match", "ieagan_pxd_match_scratch", "ieagan_pxd_match_stats")


def test_match_entry_points_are_declared_exported_and_bound():
    _hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTS and sym in _hip._SIGS, sym
    sig, stats = _hip._SIGS["ieagan_pxd_match"], _hip._SIGS["ieagan_pxd_match_stats"]
    assert len(sig) == 38 and len(stats) == 27 and len(_hip._SIGS["ieagan_pxd_match_scratch"]) == 4
    assert [k for k, t in enumerate(sig) if t is ctypes.c_int] == [21, 22, 23] and [k for k, t in enumerate(sig) if t is ctypes.c_long] == [24, 25]
    assert [k for k, t in enumerate(stats) if t is ctypes.c_int] == [17, 18, 19, 20, 23] and [k for k, t in enumerate(stats) if t is ctypes.c_long] == [21, 22]
    assert _hip.PXD_MATCH_BINS == MR.COLUMNS == 5 + 64 + 64 + 32 and _hip.PXD_MATCH_COUNTERS == MR.COUNTERS
    assert _hip.PXD_MATCH_COLUMNS == {"residual_u": (MR.RES_U, 64), "residual_v": (MR.RES_V, 64), "purity": (MR.PURITY, 32)}
    lib.ieagan_abi_version.restype = ctypes.c_int
    assert lib.ieagan_abi_version() == _hip.ABI_VERSION == 12       # new entry points only: no struct and no existing signature changed
    assert len(re.findall(r"^(?:int|long|const char\*) ieagan_\w+\(", header, re.M)) == len(_hip.EXPORTS)


MATCH_ARGS = ("s_index s_charge s_label s_digit_total s_size s_ccharge s_cluster_total s_cluster s_accepted_total s_u s_v m_index m_label "
              "m_digit_total m_size m_ccharge m_cluster_total m_cluster m_accepted_total m_u m_v N H W s_capacity m_capacity found lo hi "
              "signal_size signal_charge n_signal mixed_hit flags du dv scratch").split()
STATS_ARGS = ("s_cluster s_accepted_total s_first s_cluster_total s_digit_total s_u s_v m_ccharge m_cluster_total m_accepted_total "
              "m_digit_total m_u m_v lo signal_charge mixed_hit flags N H W n_sensors s_capacity m_capacity residual_bin table overflow").split()
SCALARS = dict(N=4, H=8, W=8, n_sensors=2, s_capacity=16, m_capacity=16, residual_bin=10)


def _refusals(lib, sigs, name, args, cases):
    fn = getattr(lib, name)
    fn.argtypes = sigs[name]
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.addressof(buf)
    good = {k: SCALARS.get(k, p) for k in args}
    for change, text in cases(p):
        rc = fn(*dict(good, **change).values(), None)
        msg = lib.ieagan_last_error().decode()
        assert rc != 0 and msg.startswith(name[len("ieagan_"):] + ": ") and text in msg, (change, msg)
    return good


def test_the_match_launcher_rejects_bad_arguments_before_any_launch():
    _hip, lib = _lib()

    def cases(p):
        out = [(dict(N=0), "outside 1 .. 65535"), (dict(N=65536), "outside 1 .. 65535"), (dict(H=0), "bad image size"), (dict(W=-1), "bad image size"),
               (dict(N=64, H=8192, W=8192), "does not fit the int32 flat index"), (dict(s_capacity=-1), "signal_capacity = -1 is negative"),
               (dict(m_capacity=-1), "mixed_capacity = -1 is negative"), (dict(s_charge=None), "s_charge / flags is NULL"),
               (dict(flags=None), "s_charge / flags is NULL"), (dict(scratch=None), "scratch"), (dict(scratch=p + 2), "scratch")]
        for k in MATCH_ARGS:
            side = "signal" if k.startswith("s_") or k in ("found", "lo", "hi", "mixed_hit", "du", "dv") else "mixed"
            if k.endswith("_total"):
                out += [({k: None}, f"a total of the {side} side is NULL or misaligned"), ({k: p + 2}, f"a total of the {side} side is NULL or misaligned")]
            elif k not in SCALARS and k not in ("s_charge", "flags", "scratch"):
                out += [({k: None}, f"an array of the {side} side is NULL"), ({k: p + 2}, f"array of the {side} side is not 4-byte aligned")]
        return out
    good = _refusals(lib, _hip._SIGS, "ieagan_pxd_match", MATCH_ARGS, cases)
    assert list(good) == MATCH_ARGS and len(good) + 1 == len(_hip._SIGS["ieagan_pxd_match"])


def test_the_statistics_launcher_rejects_bad_arguments_before_any_launch():
    _hip, lib = _lib()

    def cases(p):
        out = [(dict(N=0), "outside 1 .. 65535"), (dict(H=0), "bad image size"), (dict(N=64, H=8192, W=8192), "does not fit the int32 flat index"),
               (dict(n_sensors=0), "not a multiple of n_sensors"), (dict(n_sensors=3), "N = 4 is not a multiple of n_sensors = 3"),
               (dict(residual_bin=0), "residual_bin = 0 is not >= 1"), (dict(residual_bin=-5), "residual_bin = -5 is not >= 1"),
               (dict(s_capacity=-1), "signal_capacity = -1 is negative"), (dict(m_capacity=-1), "mixed_capacity = -1 is negative"),
               (dict(flags=None), "flags is NULL"), (dict(table=None), "table / overflow is NULL"), (dict(overflow=None), "table / overflow is NULL"),
               (dict(table=p + 4), "not 8-byte aligned"), (dict(overflow=p + 4), "not 8-byte aligned")]
        for k in STATS_ARGS:
            side = "signal" if k.startswith("s_") or k in ("lo", "mixed_hit") else "mixed"
            if k.endswith("_total"):
                out += [({k: None}, f"a total of the {side} side is NULL or misaligned"), ({k: p + 2}, f"a total of the {side} side is NULL or misaligned")]
            elif k not in SCALARS and k not in ("flags", "table", "overflow"):
                out += [({k: None}, f"an array of the {side} side is NULL"), ({k: p + 2}, f"array of the {side} side is not 4-byte aligned")]
        return out
    good = _refusals(lib, _hip._SIGS, "ieagan_pxd_match_stats", STATS_ARGS, cases)
    assert list(good) == STATS_ARGS and len(good) + 1 == len(_hip._SIGS["ieagan_pxd_match_stats"])


def test_the_scratch_size_is_non_negative_and_monotone():
    _hip, lib = _lib()
    scratch = lib.ieagan_pxd_match_scratch
    scratch.argtypes, scratch.restype = _hip._SIGS["ieagan_pxd_match_scratch"], ctypes.c_long
    caps = [0, 1, 255, 256, 4096, 10 ** 6, 2 ** 31 - 1, 2 ** 31, 2 ** 40]
    sizes = [scratch(40, 250, 768, c) for c in caps]
    assert sizes == [min(c, 2 ** 31 - 1) for c in caps]              # one word per mixed cluster
    assert scratch(0, 8, 8, 100) == 0 and scratch(4, 0, 8, 100) == 0 and scratch(4, 8, 8, -1) == 0


def _fake_hits(utils, **changes):
    h = utils.PXDHits.__new__(utils.PXDHits)
    geometry = changes.pop("geometry", None) or utils.PXDGeometry.uniform((8, 8), 100, 110, 2)
    vars(h).update(dict(shape=(4, 8, 8), n_sensors=2, threshold=7.0, seed_cut=0, charge_cut=0, head_tail=3, geometry=geometry,
                        header=types.SimpleNamespace(device=torch.device("cuda:0"))), **changes)
    return h


def test_host_side_refusals_come_before_any_device_call(monkeypatch):
    import _hip
    import utils

    def no_device(*a, **k):
        raise AssertionError("a device call before the host checks were done")
    monkeypatch.setattr(_hip, "require_gpu", no_device)
    monkeypatch.setattr(_hip, "call", no_device)
    a = _fake_hits(utils)
    cases = [(dict(shape=(4, 8, 9)), "differ in shape"), (dict(n_sensors=4), "differ in n_sensors"), (dict(threshold=0.0), "differ in threshold"),
             (dict(seed_cut=5), "differ in seed_cut"), (dict(charge_cut=5), "differ in charge_cut"), (dict(head_tail=0), "differ in head_tail"),
             (dict(geometry=utils.PXDGeometry.uniform((8, 8), 100, 120, 2)), "differ in geometry"),
             (dict(geometry=utils.PXDGeometry.uniform((8, 8), 100, 110, 2, unit_mm=1e-3)), "differ in geometry"),
             (dict(header=types.SimpleNamespace(device=torch.device("cuda:1"))), "differ in device")]
    for change, match in cases:
        for pair in ((a, _fake_hits(utils, **change)), (_fake_hits(utils, **change), a)):
            with pytest.raises(ValueError, match=match):
                utils.pxd_match(*pair)
            with pytest.raises(ValueError, match=match):
                utils.PXDMatchStatistics(n_sensors=2).update(*pair)
    for bad in (np.zeros(3), None, torch.zeros(4, 8, 8)):
        with pytest.raises(TypeError, match="must be the PXDHits"):
            utils.pxd_match(a, bad)
        with pytest.raises(TypeError, match="must be the PXDHits"):
            utils.pxd_match(bad, a)
    with pytest.raises(ValueError, match="residual_bin = 0"):
        utils.PXDMatchStatistics(residual_bin=0)
    with pytest.raises(RuntimeError, match="before any update"):
        utils.PXDMatchStatistics().result()
    # an equal geometry built twice is the same geometry
    b = _fake_hits(utils)
    assert a.geometry is not b.geometry
    with pytest.raises(AssertionError, match="a device call"):           # the checks pass; the next step is the device
        utils.pxd_match(a, b)
    for name in ("pxd_match", "PXDMatch", "PXDMatchStatistics", "pxd_match_distance", "PXD_MATCHED", "PXD_CHANGED", "PXD_SHARED"):
        assert hasattr(utils, name)
    assert (utils.PXD_MATCHED, utils.PXD_CHANGED, utils.PXD_SHARED) == (MR.MATCHED, MR.CHANGED, MR.SHARED)


def test_match_distance_of_two_result_tables():
    import utils
    S = 2

    def result(hits, matched, changed, shared, ru, rv, purity):
        r = dict(hits=np.array(hits), matched=np.array(matched), changed=np.array(changed), shared=np.array(shared), residual_bin=10, unit_mm=5e-4)
        for k, bins, n in (("residual_u", ru, 64), ("residual_v", rv, 64), ("purity", purity, 32)):
            r[k] = np.zeros((S, n), np.int64)
            for s, b, c in bins:
                r[k][s, b] = c
        return r
    real = result([10, 10], [8, 8], [4, 4], [2, 2], [(0, 32, 8)], [(1, 30, 8)], [(0, 31, 16)])
    fake = result([10, 10], [6, 8], [7, 0], [0, 7], [(0, 34, 4), (1, 34, 4)], [(0, 30, 8)], [(0, 31, 8), (1, 15, 8)])
    d = utils.pxd_match_distance(real, fake)
    assert d["efficiency_abs_err"] == pytest.approx(abs(14 / 20 - 16 / 20)) and d["changed_abs_err"] == pytest.approx(abs(7 / 14 - 8 / 16))
    assert d["shared_abs_err"] == pytest.approx(abs(7 / 14 - 4 / 16))
    assert d["residual_u_w1"] == pytest.approx(2 * 10 * 5e-4) and d["residual_v_w1"] == 0.0 and d["purity_w1"] == pytest.approx(0.5 * 16 / 32)
    same = utils.pxd_match_distance(real, real)
    assert all(v == 0.0 for v in same.values()) and set(same) == {"efficiency_abs_err", "changed_abs_err", "shared_abs_err", "residual_u_w1",
                                                                 "residual_v_w1", "purity_w1"}
    empty = result([0, 0], [0, 0], [0, 0], [0, 0], [], [], [])
    assert all(np.isnan(v) for v in utils.pxd_match_distance(real, empty).values())
    with pytest.raises(ValueError, match="residual_bin"):
        utils.pxd_match_distance(real, dict(fake, residual_bin=5))


def test_match_events_help_runs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "iea-gan_amd", "match_events.py"), "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and all(k in p.stdout for k in ("--signal", "--background", "--compare", "--residual_bin", "--batch"))
