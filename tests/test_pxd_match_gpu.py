"""Signal-hit matching on the device (MI355X): ``utils.pxd_match`` and ``utils.PXDMatchStatistics`` against the NumPy restatement
(tests/pxd_match_reference.py) on the planted overlay pairs, at 7 x 13 x 37 (every offset unaligned) and 2 x 40 x 259 (one full image: a
10 360-digit cluster that spans many waves and workgroups, so the run reduction and the atomics across steps are exercised).

Every comparison is ``np.array_equal``: the columns are integers, and ``du`` / ``dv`` are compared as bit patterns; no tolerance appears
anywhere.  The comparands (the restatement; ``pxd_hits``, ``PXDEventStore`` and ``pxd_overlay``, which predate the kernel) are never the
kernel itself, except where two runs must give the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pxd_events_reference as ER
import pxd_hits_reference as HR
import pxd_match_reference as MR
import pxd_overlay_reference as OR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPES = {"7x13x37": (7, 13, 37), "2x40x259": (2, 40, 259)}
CUTS = (20, 30)                     # seed and cluster-charge cut of the unrelated pairs: a match need not be a hit
INT_COLUMNS = ("cluster", "sensor", "event", "mixed_hit", "flags", "found", "size", "charge", "match", "hi", "mixed_charge", "signal_charge",
               "signal_size", "n_signal", "counts")
_GEOMETRY = {}


def _geometry(S, H, W):
    import utils
    if (S, H, W) not in _GEOMETRY:
        _GEOMETRY[S, H, W] = HR.two_type_geometry((H, W), W // 3, S, utils)
    return _GEOMETRY[S, H, W]


def _hits(images, S, H, W, capacity=None, seed_cut=0, charge_cut=0, threshold=0.0):
    import utils
    x = images if isinstance(images, torch.Tensor) else torch.from_numpy(images).to(DEV)
    # a capacity of one digit a pixel: the planted events are far denser than the default capacity expects
    return utils.pxd_hits(x, _geometry(S, H, W), 3, threshold, seed_cut, charge_cut, x.numel() if capacity is None else capacity, S)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _check(host, want, unit_mm, what):
    """``PXDMatch.cpu()`` against the ``per_hit`` dict of the restatement."""
    for k in INT_COLUMNS:
        assert host[k].dtype == want[k].dtype and np.array_equal(host[k], want[k]), (what, k)
    for k in ("du", "dv"):
        assert host[k].dtype == np.float32 and np.array_equal(_bits(host[k]), _bits(want[k])), (what, k)
        assert host[k + "_mm"].dtype == np.float64 and np.array_equal(host[k + "_mm"], want[k].astype(np.float64) * unit_mm), (what, k)


def _check_tables(mt, ref, what):
    """The per-cluster arrays on the device, trimmed to the true totals."""
    pc, Ts, Tm = ref["clusters"], ref["cs"]["total"], ref["cm"]["total"]
    for k in MR.PER_CLUSTER:
        T = Ts if k in ("found", "lo", "hi") else Tm
        assert np.array_equal(getattr(mt, k)[:T].cpu().numpy(), pc[k]), (what, k)


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_true_overlay_against_the_restatement_and_two_calls(name):
    import utils
    S, H, W = SHAPES[name]
    signal, _, mixed = MR.planted_case(S, H, W)
    ref = MR.cached_match("planted", S, H, W)
    hs, hm = _hits(signal, S, H, W), _hits(mixed, S, H, W)
    mt = utils.pxd_match(hs, hm)
    assert mt.signal is hs and mt.mixed is hm and mt.found.shape == (hs.capacity,) and mt.n_signal.shape == (hm.capacity,)
    assert mt.flags.dtype == torch.uint8 and mt.du.dtype == torch.float32 and mt.mixed_hit.dtype == torch.int32
    host = mt.cpu()
    want = ref["hits"]
    print(f"{name}: {ref['cs']['index'].size} signal digits in {ref['cs']['total']} clusters, {ref['cm']['index'].size} mixed digits in "
          f"{ref['cm']['total']} clusters, largest signal cluster {ref['cs']['size'].max()}; {want['cluster'].size} hits, "
          f"{int(want['changed'].sum())} changed, {int(want['shared'].sum())} shared")
    _check(host, want, hs.geometry.unit_mm, name)
    _check_tables(mt, ref, name)
    assert (host["flags"] & utils.PXD_MATCHED).all() and (host["flags"] & utils.PXD_CHANGED).any() and (host["flags"] & utils.PXD_SHARED).any()
    same = host["flags"] == utils.PXD_MATCHED
    assert same.any() and not host["du"][same].any() and not host["dv"][same].any()          # unchanged: exactly 0
    if name == "2x40x259":
        assert ref["cs"]["size"].max() == H * W                  # the full image is one cluster of 10 360 digits
    # two calls give the same bytes
    again = utils.pxd_match(hs, hm)
    n = want["cluster"].size
    for k, T in [(k, ref["cs"]["total"]) for k in ("found", "lo", "hi")] + [(k, ref["cm"]["total"]) for k in ("signal_size", "signal_charge", "n_signal")] + \
            [(k, n) for k in ("mixed_hit", "flags", "du", "dv")]:
        assert torch.equal(getattr(again, k)[:T].view(torch.uint8), getattr(mt, k)[:T].view(torch.uint8)), (name, k)


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_unrelated_batches_with_cuts_lose_hits(name):
    import utils
    S, H, W = SHAPES[name]
    signal, background, _ = MR.planted_case(S, H, W)
    ref = MR.cached_match("planted", S, H, W, 0.0, *CUTS, unrelated=True)
    hs, hm = _hits(signal, S, H, W, None, *CUTS), _hits(background, S, H, W, None, *CUTS)
    mt = utils.pxd_match(hs, hm)
    host, want = mt.cpu(), ref["hits"]
    _check(host, want, hs.geometry.unit_mm, name)
    _check_tables(mt, ref, name)
    lost = (host["flags"] & utils.PXD_MATCHED) == 0
    assert lost.any() and (~lost).any() and (host["found"] < host["size"]).any() and (host["match"] < host["hi"]).any()
    assert ((host["match"] >= 0) & (host["mixed_hit"] < 0)).any()          # a match that did not pass the cuts
    assert not host["du"][lost].any() and not host["dv"][lost].any()


def test_the_chain_is_captured_into_a_graph_and_replays_on_changed_inputs():
    """Both reconstructions and ``pxd_match`` with fixed capacities inside one capture -- a synchronising call or a copy across PCIe inside
    a capture raises -- replayed on three pairs of batches in the captured buffers."""
    import utils
    S, H, W = SHAPES["7x13x37"]
    signal, background, mixed = MR.planted_case(S, H, W)
    geometry = HR.two_type_geometry((H, W), W // 3, S)
    sets = [(signal, mixed, MR.cached_match("planted", S, H, W)["hits"]), (signal, background, MR.cached_match("planted", S, H, W, unrelated=True)["hits"]),
            (background, mixed, MR.match(background, mixed, geometry)["hits"])]
    xs, xm = torch.from_numpy(signal).to(DEV), torch.from_numpy(mixed).to(DEV)
    cap = signal.size + 5
    utils.pxd_match(_hits(xs, S, H, W, cap), _hits(xm, S, H, W, cap))       # eager: loads the library, uploads the tables
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mt = utils.pxd_match(_hits(xs, S, H, W, cap), _hits(xm, S, H, W, cap))
    for k in (0, 1, 2, 0):
        s, m, want = sets[k]
        xs.copy_(torch.from_numpy(s))
        xm.copy_(torch.from_numpy(m))
        g.replay()
        _check(mt.cpu(), want, mt.geometry.unit_mm, f"replay {k}")
    assert sets[0][2]["cluster"].size != sets[2][2]["cluster"].size
    del g


def test_statistics_over_two_updates_and_with_a_product_passed_in(monkeypatch):
    import _hip
    import utils
    S, H, W = SHAPES["7x13x37"]
    signal, background, mixed = MR.planted_case(S, H, W)
    refs = [MR.cached_match("planted", S, H, W, 0.0, *CUTS), MR.cached_match("planted", S, H, W, 0.0, *CUTS, unrelated=True)]
    hs, hm, hb = (_hits(x, S, H, W, None, *CUTS) for x in (signal, mixed, background))
    calls = []
    call = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), call(name, *a))[1])
    for w in (10, 3):
        acc = utils.PXDMatchStatistics(n_sensors=S, residual_bin=w, device=DEV)
        del calls[:]
        first = acc.update(hs, hm)
        assert isinstance(first, utils.PXDMatch) and calls == ["ieagan_pxd_match", "ieagan_pxd_match_stats"]
        del calls[:]
        product = utils.pxd_match(hs, hb)
        assert acc.update(product) is product and calls == ["ieagan_pxd_match", "ieagan_pxd_match_stats"]       # the second: the statistics alone
        res = acc.result()
        want = MR.tables(refs[0]["hits"], S, w) + MR.tables(refs[1]["hits"], S, w)
        for i, k in enumerate(MR.COUNTERS):
            assert res[k].dtype == np.int64 and np.array_equal(res[k], want[:, i]), (w, k)
        assert np.array_equal(res["residual_u"], want[:, MR.RES_U:MR.RES_V]) and np.array_equal(res["residual_v"], want[:, MR.RES_V:MR.PURITY])
        assert np.array_equal(res["purity"], want[:, MR.PURITY:]) and res["residual_bin"] == w and res["unit_mm"] == hs.geometry.unit_mm
        assert np.array_equal(res["hits"], res["matched"] + res["lost"]) and res["lost"].sum() > 0 and res["changed"].sum() > 0
        assert res["residual_u"].sum() == res["residual_v"].sum() == res["changed"].sum() and res["purity"].sum() == res["matched"].sum()
        assert res["n_events"] == 2 * len(signal) // S
        assert np.array_equal(res["hits_per_image"], np.concatenate([r["hits"]["counts"] for r in refs]).reshape(-1, S))
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.array_equal(res["efficiency"], res["matched"] / res["hits"], equal_nan=True)
            assert np.array_equal(res["changed_fraction"], res["changed"] / res["matched"], equal_nan=True)
            assert np.array_equal(res["shared_fraction"], res["shared"] / res["matched"], equal_nan=True)
        print(f"w = {w}: " + ", ".join(f"{k} {int(res[k].sum())}" for k in MR.COUNTERS))
    d = utils.pxd_match_distance(res, res)
    assert all(v == 0.0 for v in d.values())
    with pytest.raises(TypeError, match="mixed= must be left out"):
        acc.update(product, hm)


def test_a_capacity_below_the_digit_total_raises_in_result_and_reruns_in_cpu():
    import utils
    S, H, W = SHAPES["7x13x37"]
    signal, _, mixed = MR.planted_case(S, H, W)
    ref = MR.cached_match("planted", S, H, W)
    ds, dm = ref["cs"]["index"].size, ref["cm"]["index"].size
    for cap_s, cap_m in ((signal.size, dm - 1), (ds // 2, mixed.size), (ds - 1, dm // 3)):
        hs, hm = _hits(signal, S, H, W, cap_s), _hits(mixed, S, H, W, cap_m)
        acc = utils.PXDMatchStatistics(n_sensors=S, device=DEV)
        mt = acc.update(hs, hm)
        with pytest.raises(RuntimeError, match="1 update.s. held more digits than the capacity"):
            acc.result()
        host = mt.cpu()                                             # grows the side that overflowed and runs the match again
        _check(host, ref["hits"], hs.geometry.unit_mm, (cap_s, cap_m))
        assert hs.capacity == max(cap_s, ds) and hm.capacity == max(cap_m, dm) and mt.found.numel() == hs.capacity
        _check_tables(mt, ref, (cap_s, cap_m))
        acc.reset()
        acc.update(mt)
        assert np.array_equal(acc.result()["hits"], MR.tables(ref["hits"], S)[:, 0])


def test_match_events_as_a_child_process(tmp_path):
    import utils
    sys.path.insert(0, os.path.join(ROOT, "iea-gan_amd"))
    import match_events
    S, H, W = SHAPES["7x13x37"]
    ea, eb, _ = OR.planted(S, H, W, seed=S)
    A, B = ER.columns(ea, S), ER.columns(eb, S)
    sig, bg, out = (os.path.join(str(tmp_path), f) for f in ("signal.npz", "background.npz", "match.npz"))
    utils.write_digits(sig, *A)
    utils.write_digits(bg, *B)
    n, opts = 11, dict(head_tail=3, threshold=7.0, seed_cut=20, charge_cut=30, residual_bin=4, batch=4)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "iea-gan_amd", "match_events.py"), "--signal", sig,
                        "--background", bg, "--compare", sig, "--out", out, "--events", str(n), "--seed", "5", "--shape", str(H), str(W), "--n_sensors",
                        str(S), "--uniform_pitch", "50", "55.5", "--threshold", "7", "--seed_cut", "20", "--cluster_cut", "30", "--residual_bin", "4",
                        "--batch", "4"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    print(rec)
    assert rec == json.load(open(out + ".json"))
    # the in-process path
    geometry = utils.PXDGeometry.uniform((H, W), 100, 111, S)
    a = utils.PXDEventStore.from_arrays(*A, shape=(H, W), n_sensors=S, device=DEV)
    results = []
    for cols in (B, A):
        b = utils.PXDEventStore.from_arrays(*cols, shape=(H, W), n_sensors=S, device=DEV)
        ids_s, ids_b = match_events.pairs(len(a), len(b), n, 5)
        results.append(match_events.match_stores(utils, a, b, ids_s, ids_b, geometry, **opts))
    want = dict(match_events.record(results[0]), compare=match_events.record(results[1]), distance=utils.pxd_match_distance(*results))
    assert json.loads(json.dumps(want)) == rec or str(json.loads(json.dumps(want))) == str(rec)          # NaN != NaN: compare the text then
    with np.load(out) as t:
        for k in match_events.TABLES:
            assert np.array_equal(t[k], results[0][k], equal_nan=True) and np.array_equal(t["compare_" + k], results[1][k], equal_nan=True), k
    # and the restatement of the first background: the same pairs as dense images
    ids_s, ids_b = match_events.pairs(len(ea), len(eb), n, 5)
    signal = ER.dense(A, ids_s, (H, W), S)
    mixed = OR.dense_sum(A, ids_s, B, ids_b, (H, W), S)
    tables = (np.full((1, H), 100), np.full((1, W), 111), np.zeros(S, np.int64))
    ref = MR.match(signal, mixed, tables, 3, 7.0, 20, 30)["hits"]
    t = MR.tables(ref, S, 4)
    assert [rec[k] for k in MR.COUNTERS] == t[:, :5].sum(0).tolist() and rec["events"] == n and rec["hits"] > 0 and rec["changed"] > 0
    assert rec["residual_u_sum"] == rec["changed"] and rec["purity_sum"] == rec["matched"] and rec["residual_bin"] == 4 and rec["unit_mm"] == 5e-4
    assert np.array_equal(results[0]["residual_v"], t[:, MR.RES_V:MR.PURITY]) and np.array_equal(results[0]["purity"], t[:, MR.PURITY:])
