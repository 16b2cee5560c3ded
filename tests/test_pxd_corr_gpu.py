"""Intra-event correlations on the device (MI355X): ``utils.pxd_region_counts``, ``utils.PXDCorrelations``, the part of ``utils.PXDValidation``
and ``validate.py --correlations`` against the NumPy restatement (tests/pxd_corr_reference.py) at its two shapes -- A: 7 events of
3 x 13 x 37 on a 2 x 3 grid (R = 18: every offset unaligned, the runs of a wave's step cross region, row, image and event boundaries); B: 70
events of 40 x 8 x 24 on a 1 x 2 grid (R = 80: E > 64 and R > 64, neither a multiple of 64, every edge tile of the rank and Gram kernels).

Every comparison is ``np.array_equal``: the device numbers are integers, and the float64 coefficients come from the same host recipe on
equal integers, so they are compared as bit patterns; no tolerance appears anywhere.  The comparand is always the restatement, except
where two runs must give the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pxd_corr_reference as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
THRESHOLD = CR.THRESHOLD
INT_TABLES = ("gram", "sum", "rank_gram", "rank_sum", "counts")
KEYS = {"gram", "sum", "rank_gram", "rank_sum", "counts", "n_events", "regions", "shape", "pearson", "spearman"}


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _check(res, want, what):
    """A ``PXDCorrelations.result()`` against the restatement's."""
    assert set(res) == KEYS, what
    for k in INT_TABLES:
        assert res[k].dtype == want[k].dtype and np.array_equal(res[k], want[k]), (what, k)
    assert res["n_events"] == want["n_events"] and tuple(res["regions"]) == want["regions"] and tuple(res["shape"]) == want["shape"], what
    assert np.array_equal(res["gram"], res["gram"].T) and np.array_equal(res["rank_gram"], res["rank_gram"].T), what
    for k in ("pearson", "spearman"):
        assert res[k].dtype == np.float64 and np.array_equal(_bits(res[k]), _bits(want[k])), (what, k)


def _same_bytes(a, b, what):
    for k in INT_TABLES + ("pearson", "spearman"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("name", list(CR.SHAPES))
def test_region_counts_against_the_restatement_and_two_calls(name):
    import _hip as H
    import utils
    E, S, Hh, Ww, regions = CR.SHAPES[name]
    x, counts, _ = CR.case(name)
    want = _dev(counts)
    u8, f32 = _dev(x), _dev(CR.as_f32(x))
    digits = utils.pxd_digits(u8, THRESHOLD, x.size, S)
    for what, given in (("uint8", u8), ("fp32", f32), ("PXDDigits", digits)):
        got = utils.pxd_region_counts(given, regions, THRESHOLD, x.size, S)
        assert got.dtype == torch.int32 and got.shape == counts.shape and got.device == u8.device and torch.equal(got, want), (name, what)
        assert torch.equal(utils.pxd_region_counts(given, regions, THRESHOLD, x.size, S), got), (name, what)          # two calls, the same bytes
    # images that start one element past a 16-byte boundary
    for base in (u8, f32):
        buf = torch.empty(base.numel() + 17, dtype=base.dtype, device=DEV)
        view = buf[17:].view(base.shape)
        view.copy_(base)
        assert view.data_ptr() % 16 == base.element_size()
        assert torch.equal(utils.pxd_region_counts(view, regions, THRESHOLD, x.size, S), want), (name, base.dtype)
    # the digit list and the table themselves one element past a 16-byte boundary, through the C ABI
    total = int(digits.total.item())
    index = torch.empty(total + 5, dtype=torch.int32, device=DEV)[5:]
    index.copy_(digits.index[:total])
    out = torch.full((counts.size + 5,), -1, dtype=torch.int32, device=DEV)
    overflow = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert index.data_ptr() % 16 == 4 and out[5:].data_ptr() % 16 == 4
    H.call("ieagan_pxd_region_counts", index.data_ptr(), digits.total.data_ptr(), E * S, Hh, Ww, S, *regions, total, out[5:].data_ptr(),
           overflow.data_ptr(), H.stream())
    assert torch.equal(out[5:].view(counts.shape), want) and (out[:5] == -1).all() and int(overflow.item()) == 0
    # whole sensors: the grid 1 x 1 sums the regions of a sensor
    per = regions[0] * regions[1]
    whole = utils.pxd_region_counts(digits, (1, 1))
    assert whole.shape == (E, S) and torch.equal(whole, want.view(E, S, per).sum(2).to(torch.int32))
    for bad, what in (((Hh + 1, 1), "finer than"), ((1, Ww + 1), "finer than"), ((0, 1), "at least 1 x 1"), ((32, 32), "more than 1024 columns")):
        with pytest.raises(ValueError, match=what):
            utils.pxd_region_counts(digits, bad)


@pytest.mark.parametrize("name,cuts", [("A", (1, 2, 4)), ("B", (8,) * 8 + (6,))])
def test_correlations_in_updates_against_the_restatement(name, cuts):
    import utils
    E, S, Hh, Ww, regions = CR.SHAPES[name]
    x, counts, want = CR.case(name)
    assert sum(cuts) == E
    u8 = _dev(x)
    kw = dict(n_sensors=S, threshold=THRESHOLD, regions=regions, capacity=x.size, device=DEV)
    acc = utils.PXDCorrelations(**kw)
    e0 = 0
    for i, n in enumerate(cuts):
        batch = u8[e0 * S:(e0 + n) * S]
        given = (batch, utils.pxd_digits(batch, THRESHOLD, x.size, S), utils.pxd_clusters(batch, THRESHOLD, x.size, S))[i % 3]
        got = acc.update(given)
        assert torch.equal(got, _dev(counts[e0:e0 + n])), (name, i)
        e0 += n
    assert acc.tables.shape == (want["gram"].size + want["sum"].size + 1,) and acc.tables.dtype == torch.int64
    res = acc.result()
    _check(res, want, name)
    print(f"{name}: {res['n_events']} events, R = {res['sum'].size}, {int(res['sum'].sum())} digits, "
          f"{int(np.isnan(res['spearman']).sum())} undefined coefficients, largest rank_gram {int(res['rank_gram'].max())}")
    assert np.array_equal(res["rank_sum"], np.full(res["sum"].size, E * (E + 1)))           # twice the sum of the ranks 1 .. E, ties or not
    _same_bytes(acc.result(), res, f"{name} result() twice")
    one = utils.PXDCorrelations(**kw)
    one.update(u8)
    _same_bytes(one.result(), res, f"{name} one update")
    d = utils.pxd_correlation_distance(res, one.result())
    assert all(v == 0.0 for v in d.values()) and len(d) == 4
    with pytest.raises(ValueError, match="image size"):
        acc.update(torch.zeros(S, Hh + 1, Ww, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="threshold"):
        acc.update(utils.pxd_digits(u8, 0.0, x.size, S))


def test_an_empty_an_all_lit_and_an_all_equal_batch():
    import utils
    E, S, Hh, Ww, regions = 5, 3, 13, 37, (2, 3)
    R = S * regions[0] * regions[1]
    areas = np.tile(CR.region_areas(Hh, Ww, regions), S)
    kw = dict(n_sensors=S, threshold=THRESHOLD, regions=regions, capacity=E * S * Hh * Ww, device=DEV)
    for what, value, row in (("empty", 0, np.zeros(R, np.int32)), ("all lit", 200, areas)):
        acc = utils.PXDCorrelations(**kw)
        x = torch.full((E * S, Hh, Ww), value, dtype=torch.uint8, device=DEV)
        assert torch.equal(acc.update(x), _dev(np.tile(row, (E, 1)))), what
        res = acc.result()
        want = CR.result(np.tile(row, (E, 1)), regions, (Hh, Ww))
        _check(res, want, what)
        # every column tied: rank2 = E + 1 everywhere, no coefficient is defined
        assert np.array_equal(res["rank_sum"], np.full(R, E * (E + 1))) and np.array_equal(res["rank_gram"], np.full((R, R), E * (E + 1) ** 2))
        assert np.isnan(res["pearson"]).all() and np.isnan(res["spearman"]).all()
        assert all(np.isnan(v) for v in utils.pxd_correlation_distance(res, res).values())
    # equal events of a planted one
    ev = CR.case("A")[0][:S]
    acc = utils.PXDCorrelations(**kw)
    acc.update(_dev(np.tile(ev, (E, 1, 1))))
    res = acc.result()
    _check(res, CR.result(np.tile(CR.case("A")[1][:1], (E, 1)), regions, (Hh, Ww)), "all equal")
    assert np.isnan(res["spearman"]).all() and (res["rank_sum"] == E * (E + 1)).all() and res["sum"].sum() > 0
    # a single event
    acc = utils.PXDCorrelations(**kw)
    acc.update(_dev(ev))
    res = acc.result()
    _check(res, CR.result(CR.case("A")[1][:1], regions, (Hh, Ww)), "one event")
    assert res["n_events"] == 1 and np.isnan(res["pearson"]).all() and (res["rank_sum"] == 2).all()


def test_a_capacity_below_the_digit_total_raises_in_result():
    import utils
    E, S, Hh, Ww, regions = CR.SHAPES["A"]
    x, counts, _ = CR.case("A")
    u8 = _dev(x)
    total = int(counts.sum())
    kw = dict(n_sensors=S, threshold=THRESHOLD, device=DEV)
    acc = utils.PXDCorrelations(regions=regions, capacity=total - 1, **kw)
    got = acc.update(u8)
    assert int(got.sum().item()) == total - 1                    # the first capacity digits are counted
    acc.update(utils.pxd_digits(u8, THRESHOLD, total, S))           # this one fits
    with pytest.raises(RuntimeError, match=r"PXDCorrelations: 1 update\(s\) held more digits than the capacity of %d" % (total - 1)):
        acc.result()
    acc.reset()
    assert acc.tables is None and acc.counts == [] and acc.rank_tables == []
    with pytest.raises(RuntimeError, match="before any update"):
        acc.result()
    # the other accumulators say what they said
    cs = utils.PXDClusterStatistics(capacity=64, **kw)
    cs.update(u8)
    with pytest.raises(RuntimeError, match=r"PXDClusterStatistics: 1 update\(s\) held more digits than the capacity of 64, their clusters are "
                                           r"truncated: pass a larger capacity= to PXDClusterStatistics"):
        cs.result()
    bundle = utils.PXDValidation(capacity=64, correlations=regions, **kw)
    bundle.update(u8)
    assert bundle.stats.result()["n_events"] == E
    with pytest.raises(RuntimeError, match="PXDCorrelations: 1 update.s. held more digits"):
        bundle.result()


def test_an_update_is_captured_into_a_graph_and_replays_on_changed_input():
    """One ``update`` with a fixed capacity inside a capture on a single stream -- a synchronising call or a copy across PCIe inside a capture
    raises -- replayed on three batches in the captured buffer; the moments equal those of three eager updates."""
    import utils
    E, S, Hh, Ww, regions = CR.SHAPES["A"]
    x, counts, _ = CR.case("A")
    batches = [x[:2 * S], x[2 * S:4 * S], x[4 * S:6 * S]]
    cap = 2 * S * Hh * Ww
    kw = dict(n_sensors=S, threshold=THRESHOLD, regions=regions, capacity=cap, device=DEV)
    eager = utils.PXDCorrelations(**kw)
    for b in batches:
        eager.update(_dev(b))
    buf = _dev(batches[0])
    acc = utils.PXDCorrelations(**kw)
    acc.update(buf)                      # eager: loads the library, allocates the tables
    acc.tables.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = acc.update(buf)
    for k in (0, 1, 2):
        buf.copy_(_dev(batches[k]))
        g.replay()
        assert torch.equal(captured, _dev(counts[2 * k:2 * k + 2])), k
    assert torch.equal(acc.tables, eager.tables)
    want = CR.moments(counts[:6])
    R = counts.shape[1]
    assert np.array_equal(acc.tables[:R * R].cpu().numpy().reshape(R, R), want[2].astype(np.int64)) and int(acc.tables[-1].item()) == 0
    del g


def test_the_bundle_equals_the_four_parts_fed_separately_and_is_unchanged_when_off(monkeypatch):
    import _hip
    import utils
    S, Hh, Ww, cuts, regions = 4, 64, 96, (20, 30), (2, 3)
    rng = np.random.Generator(np.random.PCG64(18))
    evs = [_dev(np.where(rng.random((S, Hh, Ww)) < 0.04, rng.integers(1, 256, (S, Hh, Ww)), 0).astype(np.uint8)) for _ in range(3)]
    batches = [torch.cat(evs[:2]), evs[2]]
    kw = dict(n_sensors=S, threshold=THRESHOLD, device=DEV)
    parts = dict(stats=utils.PXDStatistics(**kw), clusters=utils.PXDClusterStatistics(**kw),
                 maps=utils.PXDClusterMaps(seed_cut=cuts[0], charge_cut=cuts[1], **kw), correlations=utils.PXDCorrelations(regions=regions, **kw))
    calls = []
    call = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), call(name, *a))[1])
    new = {"ieagan_pxd_region_counts", "ieagan_pxd_gram", "ieagan_pxd_ranks"}
    for x in batches:
        for acc in parts.values():
            acc.update(x)
    want = {k: acc.result() for k, acc in parts.items()}
    del calls[:]
    acc = utils.PXDValidation(True, cuts, correlations=regions, **kw)
    for x in batches:
        acc.update(x)
    assert calls.count("ieagan_pxd_digits") == 2 and calls.count("ieagan_pxd_region_counts") == 2 and calls.count("ieagan_pxd_gram") == 2
    got = acc.result()
    assert tuple(got) == ("stats", "clusters", "maps", "correlations") and calls.count("ieagan_pxd_ranks") == 1
    for part in got:
        assert set(got[part]) == set(want[part]), part
        for k, v in want[part].items():
            a, b = np.asarray(got[part][k]), np.asarray(v)
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=b.dtype.kind == "f"), (part, k)
    dense = torch.cat(batches).cpu().numpy()
    _check(got["correlations"], CR.result(CR.region_counts(dense, regions, S, THRESHOLD), regions, (Hh, Ww)), "bundle")
    dist = utils.pxd_validation_distance(got, want)
    assert len(dist) == 15 and {"pearson_rms", "spearman_rms", "spearman_max_abs", "spearman_strength_err"} <= set(dist)
    tables = utils.pxd_validation_tables(real=got, fake=want)
    assert {"real_region_counts", "fake_spearman", "real_rank_gram", "fake_sum"} <= set(tables) and "real_regions" not in tables and "real_counts" not in tables
    # the chain off: the correlations run pxd_digits alone
    del calls[:]
    only = utils.PXDValidation(correlations=True, **kw)
    only.update(batches[0])
    assert calls == ["ieagan_pxd_stats", "ieagan_pxd_digits", "ieagan_pxd_region_counts", "ieagan_pxd_gram"]
    assert tuple(only.result()) == ("stats", "correlations") and only.correlations.regions == (1, 1)
    # correlations off: the launches and the keys of before
    del calls[:]
    off = utils.PXDValidation(True, cuts, **kw)
    for x in batches:
        off.update(x)
    res = off.result()
    assert off.correlations is None and not new & set(calls) and set(res) == {"stats", "clusters", "maps"}
    assert calls == ["ieagan_pxd_stats", "ieagan_pxd_digits", "ieagan_pxd_clusters", "ieagan_pxd_cluster_stats", "ieagan_pxd_cluster_positions",
                     "ieagan_pxd_cluster_maps"] * 2


KEYS_TODAY = {"which", "n_events_real", "n_events", "occ_rel_err", "charge_rel_err", "spectrum_w1"}
KEYS_CORR = {"pearson_rms", "spearman_rms", "spearman_max_abs", "spearman_strength_err", "regions"}
TABLES_CORR = ("gram", "sum", "rank_gram", "rank_sum", "region_counts", "pearson", "spearman")


def test_validate_tool_with_and_without_correlations(tmp_path):
    import train
    import utils
    tool = os.path.join(ROOT, "iea-gan_amd", "validate.py")
    geom = ["--resolution", "64", "--H_base", "1"]
    cfg = train.parse(geom)
    d = os.path.join(str(tmp_path), "events")
    os.makedirs(d)
    fake_events = [train.synthetic_event(40, 58, 64, 500 + i) for i in range(3)]
    for i, ev in enumerate(fake_events):
        np.save(os.path.join(d, f"event_{i}.npy"), ev)
    real_events = [train.synthetic_event(40, 58, 64, cfg["seed"] + i) for i in range(3)]
    sides = []
    for events in (real_events, fake_events):
        acc = utils.PXDCorrelations(n_sensors=40, threshold=cfg["val_threshold"], regions=(2, 4), device=DEV)
        for ev in events:
            acc.update(torch.from_numpy(ev))
        sides.append(acc.result())
        _check(sides[-1], CR.result(CR.region_counts(np.concatenate(events), (2, 4), 40, cfg["val_threshold"]), (2, 4), (58, 64)), "validate")
    want = utils.pxd_correlation_distance(*sides)
    assert sides[0]["sum"].size == 320 and all(np.isfinite(v) for v in want.values()) and want["spearman_rms"] > 0
    recs, tables = {}, {}
    for flag in ([], ["--correlations", "--regions", "2", "4"]):
        out = os.path.join(str(tmp_path), f"tables{len(flag)}.npz")
        p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, tool, "--synthetic", "3", "--compare", d, "--events", "3", "--out", out]
                           + flag + geom, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        recs[len(flag)] = json.loads(p.stdout.strip().splitlines()[-1])
        tables[len(flag)] = dict(np.load(out))
    print(recs)
    assert set(recs[0]) == KEYS_TODAY and set(recs[4]) == KEYS_TODAY | KEYS_CORR
    assert all(recs[4][k] == recs[0][k] for k in KEYS_TODAY)
    assert all(recs[4][k] == want[k] for k in KEYS_CORR - {"regions"}) and recs[4]["regions"] == [2, 4]
    new_tables = {f"{side}_{k}" for side in ("real", "fake") for k in TABLES_CORR}
    assert not new_tables & set(tables[0]) and set(tables[4]) - set(tables[0]) == new_tables
    for side, t in zip(("real", "fake"), sides):
        for k in TABLES_CORR:
            assert np.array_equal(tables[4][f"{side}_{k}"], t["counts" if k == "region_counts" else k], equal_nan=True), (side, k)
    for k in tables[0]:
        assert np.array_equal(tables[0][k], tables[4][k], equal_nan=True), k
