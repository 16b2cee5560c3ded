"""Intra-event correlations, host side: the restatement (tests/pxd_corr_reference.py) against independent forms (``scipy.stats.rankdata``,
``np.corrcoef``, ``scipy.stats.spearmanr``) at the two shapes of the device tests; additivity of the Gram over updates; the sensitivity the
feature exists for; ``utils.pxd_correlation_distance`` on hand-made tables; the C ABI of the three entry points and the launchers'
refusals; the argument refusals of ``validate.py`` (no GPU needed).  The device side is tests/test_pxd_corr_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.stats

import pxd_corr_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES, case = CR.SHAPES, CR.case


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_restatement_against_independent_forms(name):
    E, S, H, W, regions = SHAPES[name]
    x, counts, res = case(name)
    R = S * regions[0] * regions[1]
    assert counts.shape == (E, R) and counts.dtype == np.int32 and counts.sum() == int((x >= 7).sum())
    assert np.array_equal(res["rank2"], 2 * scipy.stats.rankdata(counts, axis=0))                # exactly: twice a mid-rank is an integer
    # the planted constant column is the only one that never varies: its row and column are the NaN pattern, R - 1 pairs i < j and no more
    k = CR.constant_column(S, regions)
    assert [j for j in range(R) if (counts[:, j] == counts[0, j]).all()] == [k] and (counts[:, k] == 1).all()
    nan = np.zeros((R, R), bool)
    nan[k, :] = nan[:, k] = True
    for name_ in ("pearson", "spearman"):
        assert res[name_].dtype == np.float64 and np.array_equal(np.isnan(res[name_]), nan)
    assert int(np.triu(nan, 1).sum()) == R - 1
    # five float64 roundings of exact integers against the libraries' own mean subtraction
    with np.errstate(invalid="ignore", divide="ignore"):
        pearson = np.corrcoef(counts.T.astype(np.float64))
        spearman = scipy.stats.spearmanr(counts).statistic
    err_p, err_s = np.abs(pearson[~nan] - res["pearson"][~nan]).max(), np.abs(spearman[~nan] - res["spearman"][~nan]).max()
    print(f"{name}: pearson {err_p:.2e}, spearman {err_s:.2e} from numpy / scipy")
    assert err_p <= 1e-12 and err_s <= 1e-12
    assert np.array_equal(res["gram"], res["gram"].T) and np.array_equal(res["rank_gram"], res["rank_gram"].T)
    assert np.array_equal(res["gram"], counts.astype(np.int64).T @ counts.astype(np.int64)) and np.array_equal(res["sum"], counts.sum(0))
    # the fully lit sensor 1 of event 2: its counts are the region areas
    per = regions[0] * regions[1]
    areas = CR.region_areas(H, W, regions)
    assert np.array_equal(counts[2, per:2 * per], areas) and areas.sum() == H * W
    assert areas.tolist() == [np.sum((np.arange(H) * regions[0] // H == a)) * np.sum((np.arange(W) * regions[1] // W == b))
                              for a in range(regions[0]) for b in range(regions[1])]


def test_the_gram_of_seven_events_is_the_sum_over_updates_of_one_two_and_four():
    _, counts, res = case("A")
    parts = [CR.moments(counts[a:b]) for a, b in ((0, 1), (1, 3), (3, 7))]
    assert sum(p[0] for p in parts) == res["n_events"] == 7
    assert np.array_equal(sum(p[2] for p in parts).astype(np.int64), res["gram"])
    assert np.array_equal(sum(p[1] for p in parts).astype(np.int64), res["sum"])


def test_an_independent_generator_is_told_from_a_correlated_one():
    """The gap this feature closes.  The two sides draw every sensor image from the same single-sensor distribution (a gamma(2, 1)
    multiplicity, Poisson pixels, uniform charges), so every per-sensor statistic of the validation chain -- occupancy, charge and cluster
    spectra, position maps -- agrees in distribution; one side shares the multiplicity among the 40 sensors of an event, the other draws it
    per sensor.  Only the correlation tables tell them apart: 70 events of 40 x 8 x 24 on a 1 x 2 grid."""
    shared, again, independent = (case("B", s, seed)[2] for s, seed in ((True, 0), (True, 1), (False, 2)))
    same, other = CR.distance(shared, again), CR.distance(shared, independent)
    print(f"spearman_rms: shared / shared' {same['spearman_rms']:.3f}, shared / independent {other['spearman_rms']:.3f}; "
          f"strength_err {same['spearman_strength_err']:+.3f} and {other['spearman_strength_err']:+.3f}")
    assert other["spearman_rms"] >= 4 * same["spearman_rms"]
    assert other["spearman_strength_err"] < 0


def _tables(rho, regions=(1, 1), shape=(8, 8)):
    rho = np.asarray(rho, np.float64)
    return dict(pearson=rho, spearman=rho.copy(), regions=regions, shape=shape, n_events=5)


def test_distances_on_hand_made_tables():
    import pxd
    import utils
    nan = float("nan")
    real = _tables([[1, 0.5, nan], [0.5, 1, -0.25], [nan, -0.25, 1]])
    fake = _tables([[1, 0.1, 0.9], [0.1, 1, nan], [0.9, nan, 1]])
    keys = {"pearson_rms", "spearman_rms", "spearman_max_abs", "spearman_strength_err"}
    same = utils.pxd_correlation_distance(real, real)
    assert set(same) == keys and all(v == 0.0 for v in same.values())
    d = utils.pxd_correlation_distance(real, fake)
    # the pairs (0, 1) and (1, 2) count, (0, 2) has no real coefficient; the fake NaN counts as 0
    assert d["spearman_rms"] == pytest.approx(np.sqrt((0.4 ** 2 + 0.25 ** 2) / 2)) and d["pearson_rms"] == d["spearman_rms"]
    assert d["spearman_max_abs"] == pytest.approx(0.4) and d["spearman_strength_err"] == pytest.approx(0.05 - 0.375)
    assert d == CR.distance(real, fake)
    empty = _tables(np.full((3, 3), nan))
    assert all(np.isnan(v) for v in utils.pxd_correlation_distance(empty, fake).values())
    assert all(np.isnan(v) for v in CR.distance(empty, fake).values())
    # one event: no variance anywhere
    one = CR.result(np.array([[3, 1, 4]]), (1, 1), (8, 8))
    assert one["n_events"] == 1 and np.isnan(one["pearson"]).all() and np.isnan(one["spearman"]).all() and (one["rank2"] == 2).all()
    assert np.isnan(pxd._correlation(1, one["gram"], one["sum"])).all()
    assert all(np.isnan(v) for v in utils.pxd_correlation_distance(one, one).values())
    for change, what in ((dict(regions=(2, 1)), "regions"), (dict(shape=(8, 9)), "shape"), (dict(pearson=np.eye(4), spearman=np.eye(4)), "columns")):
        with pytest.raises(ValueError, match=what):
            utils.pxd_correlation_distance(real, dict(fake, **change))


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_host_recipe_gives_the_bits_of_the_restatement(name):
    import pxd
    res = case(name)[2]
    for coefficient, total, gram in (("pearson", "sum", "gram"), ("spearman", "rank_sum", "rank_gram")):
        got = pxd._correlation(res["n_events"], res[gram], res[total])
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), res[coefficient].view(np.uint64)), coefficient
    # moments past 2**63 / n: the product n * G is formed in Python integers
    big = np.array([[2 ** 62, 2 ** 61], [2 ** 61, 2 ** 62]], np.int64)
    rho = pxd._correlation(4, big, np.array([2 ** 31, 2 ** 31], np.int64))
    assert rho[0, 1] == float(4 * 2 ** 61 - 2 ** 62) / float(4 * 2 ** 62 - 2 ** 62) and rho[0, 0] == 1.0


def _lib():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    lib.ieagan_last_error.restype = ctypes.c_char_p
    return _hip, lib


SYMBOLS = ("ieagan_pxd_region_counts", "ieagan_pxd_gram", "ieagan_pxd_ranks")


def test_correlation_entry_points_are_declared_exported_and_bound():
    _hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTS and sym in _hip._SIGS, sym
    counts, gram, ranks = (_hip._SIGS[s] for s in SYMBOLS)
    assert len(counts) == 12 and len(gram) == 6 and len(ranks) == 5
    assert [k for k, t in enumerate(counts) if t is ctypes.c_int] == [2, 3, 4, 5, 6, 7] and [k for k, t in enumerate(counts) if t is ctypes.c_long] == [8]
    assert [k for k, t in enumerate(gram) if t is ctypes.c_int] == [1, 2] and [k for k, t in enumerate(ranks) if t is ctypes.c_int] == [1, 2]
    lib.ieagan_abi_version.restype = ctypes.c_int
    assert lib.ieagan_abi_version() == _hip.ABI_VERSION == 12       # new entry points only: no struct and no existing signature changed
    assert len(re.findall(r"^(?:int|long|const char\*) ieagan_\w+\(", header, re.M)) == len(_hip.EXPORTS) == 89 + 1          # and ieagan_last_error
    assert (_hip.PXD_CORR_MAX_COLUMNS, _hip.PXD_CORR_MAX_EVENTS) == (1024, 65535)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "89" in readme and "pxd_corr" in open(os.path.join(ROOT, "iea-gan_amd", "csrc", "build.sh")).read()


def _refusals(lib, sigs, name, args, scalars, cases):
    fn = getattr(lib, name)
    fn.argtypes = sigs[name]
    buf = (ctypes.c_longlong * 128)()
    p = ctypes.addressof(buf)
    good = {k: scalars.get(k, p + 64 * i) for i, k in enumerate(args)}           # distinct, 8-byte aligned addresses inside buf
    for change, text in cases(p):
        rc = fn(*dict(good, **change).values(), None)
        msg = lib.ieagan_last_error().decode()
        assert rc != 0 and msg.startswith(name[len("ieagan_"):] + ": ") and text in msg, (change, msg)
    return good


def test_the_counts_launcher_rejects_bad_arguments_before_any_launch():
    _hip, lib = _lib()
    args = "index digit_total N H W n_sensors RU RV capacity x overflow".split()
    scalars = dict(N=4, H=8, W=12, n_sensors=2, RU=2, RV=3, capacity=16)

    def cases(p):
        return [(dict(N=0), "outside 1 .. 65535"), (dict(N=65536), "outside 1 .. 65535"), (dict(H=0), "bad image size"), (dict(W=-1), "bad image size"),
                (dict(N=64, H=8192, W=8192), "does not fit the int32 flat index"), (dict(n_sensors=0), "not a multiple of n_sensors"),
                (dict(n_sensors=3), "N = 4 is not a multiple of n_sensors = 3"), (dict(RU=0), "regions 0 x 3 outside"),
                (dict(RU=9), "regions 9 x 3 outside 1 .. 8 x 1 .. 12"), (dict(RV=0), "regions 2 x 0 outside"), (dict(RV=13), "regions 2 x 13 outside"),
                (dict(RU=-1), "regions -1 x 3 outside"), (dict(N=1024, n_sensors=512, RU=1, RV=3), "columns exceed 1024"),
                (dict(N=40, n_sensors=40, H=250, W=768, RU=250, RV=768), "columns exceed 1024"), (dict(capacity=-1), "capacity = -1 is negative"),
                (dict(digit_total=None), "digit_total is NULL or misaligned"), (dict(digit_total=p + 2), "digit_total is NULL or misaligned"),
                (dict(index=None), "index is NULL with capacity 16"), (dict(index=p + 2), "not 4-byte aligned"),
                (dict(x=None), "x is NULL or not 4-byte aligned"), (dict(x=p + 1), "x is NULL or not 4-byte aligned"),
                (dict(overflow=None), "overflow is NULL or not 8-byte aligned"), (dict(overflow=p + 4), "overflow is NULL or not 8-byte aligned")]
    good = _refusals(lib, _hip._SIGS, SYMBOLS[0], args, scalars, cases)
    assert list(good) == args and len(good) + 1 == len(_hip._SIGS[SYMBOLS[0]])


def test_the_gram_and_rank_launchers_reject_bad_arguments_before_any_launch():
    _hip, lib = _lib()
    table = lambda p: [(dict(E=0), "E = 0 outside 1 .. 65535"), (dict(E=65536), "E = 65536 outside 1 .. 65535"), (dict(E=-3), "outside 1 .. 65535"),
                       (dict(R=0), "R = 0 outside 1 .. 1024"), (dict(R=1025), "R = 1025 outside 1 .. 1024"), (dict(x=None), "x is NULL or not 4-byte"),
                       (dict(x=p + 2), "x is NULL or not 4-byte")]
    gram = lambda p: table(p) + [(dict(gram=None), "gram / sum is NULL"), (dict(sum=None), "gram / sum is NULL"), (dict(gram=p + 4), "not 8-byte aligned"),
                                 (dict(sum=p + 4), "not 8-byte aligned")]
    good = _refusals(lib, _hip._SIGS, SYMBOLS[1], "x E R gram sum".split(), dict(E=7, R=18), gram)
    assert len(good) + 1 == len(_hip._SIGS[SYMBOLS[1]])
    ranks = lambda p: table(p) + [(dict(rank2=None), "rank2 is NULL or not 4-byte"), (dict(rank2=p + 2), "rank2 is NULL or not 4-byte"),
                                  (dict(rank2=p), "rank2 must not be x")]
    good = _refusals(lib, _hip._SIGS, SYMBOLS[2], "x E R rank2".split(), dict(E=7, R=18), ranks)
    assert len(good) + 1 == len(_hip._SIGS[SYMBOLS[2]])


def test_host_side_refusals_come_before_any_device_call(monkeypatch):
    import _hip
    import pxd
    import utils

    def no_device(*a, **k):
        raise AssertionError("a device call before the host checks were done")
    monkeypatch.setattr(_hip, "call", no_device)
    for regions, what in (((0, 1), "at least 1 x 1"), ((1, -2), "at least 1 x 1"), ((2, 13), "more than 1024 columns"), (5, "a pair"), ((1, 2, 3), "a pair")):
        with pytest.raises(ValueError, match=what):
            utils.PXDCorrelations(regions=regions)
        with pytest.raises(ValueError, match=what):
            utils.PXDValidation(correlations=regions if isinstance(regions, tuple) else [regions])
    acc = utils.PXDCorrelations(n_sensors=2, regions=(2, 4))
    assert acc.regions == (2, 4) and acc.tables is None and acc.counts == []
    with pytest.raises(RuntimeError, match="PXDCorrelations.result.. before any update"):
        acc.result()
    assert utils.PXDValidation().correlations is None and utils.PXDValidation(correlations=True).correlations.regions == (1, 1)
    assert utils.PXDValidation(correlations=(2, 4)).correlations.regions == (2, 4)
    for name in ("pxd_region_counts", "PXDCorrelations", "pxd_correlation_distance"):
        assert hasattr(utils, name)
    assert [p[0] for p in pxd._PARTS] == ["stats", "clusters", "maps", "correlations"]


def test_validation_tables_name_the_counts_of_the_correlations():
    import utils
    res = {k: v for k, v in case("A")[2].items() if k != "rank2"}
    side = dict(stats=dict(n_events=7, hits=np.zeros((7, 3))), correlations=res)
    tables = utils.pxd_validation_tables(real=side, fake=side)
    want = {"gram", "sum", "rank_gram", "rank_sum", "region_counts", "pearson", "spearman"}
    assert set(tables) == {f"{s}_{k}" for s in ("real", "fake") for k in want | {"n_events", "hits"}}
    assert np.array_equal(tables["fake_region_counts"], res["counts"])
    assert set(utils.pxd_validation_distance(dict(correlations=res), dict(correlations=res))) == {"pearson_rms", "spearman_rms", "spearman_max_abs",
                                                                                                    "spearman_strength_err"}


def test_validate_refuses_bad_region_arguments():
    import validate
    base = ["--compare", "somewhere", "--synthetic", "2", "--resolution", "64", "--H_base", "1"]
    for extra, what in ((["--regions", "2", "4"], "--regions needs --correlations"), (["--correlations", "--regions", "0", "4"], "must be positive"),
                        (["--correlations", "--regions", "2", "-1"], "must be positive")):
        with pytest.raises(SystemExit, match=what):
            validate.run(base + extra)
    with pytest.raises(SystemExit):                         # argparse: two values
        validate.run(base + ["--correlations", "--regions", "2"])
