"""Cluster-level validation on the device (MI355X): the cluster kernels against the union-find checker (tests/pxd_clusters_reference.py,
itself pinned against ``scipy.ndimage.label`` in tests/test_pxd_clusters.py), the capacity protocol, ``utils.PXDClusterStatistics`` and
``validate.py --clusters``.

Every comparison is exact (``array_equal``): labels, positions, sizes, charges and counters are integers and the numbering -- by the first
digit of a cluster -- is part of the contract.  There are no tolerances."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pxd_clusters_reference as CR
import pxd_digits_reference as DR
import pxd_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TABLE = ("first", "size", "charge", "seed", "size_u", "size_v")


def _synthetic(kind, *a, **k):
    return (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(*a, **k)


def _all_hit(kind):
    ev = np.random.Generator(np.random.PCG64(2)).integers(8, 255, (1, 250, 768))
    ev[0, 100, 300] = 255
    return ev.astype(np.uint8 if kind == "u8" else np.float32)


def _pattern(kind, rule, side=64):
    r, c = np.mgrid[0:side, 0:side]
    ev = np.where(rule(r, c), 8 + (r * side + c) % 200, 0)[None]
    return ev.astype(np.uint8 if kind == "u8" else np.float32)


CASES = {
    "7x13x37": lambda kind: _synthetic(kind, 7, 13, 37, seed=32, p_hit=0.3),
    "4x64x96_structured": lambda kind: CR.cached_structured(4, 64, 96, 21, kind)[0],
    "one_all_hit": _all_hit,
    "checkerboard": lambda kind: _pattern(kind, lambda r, c: (r + c) % 2 == 0),
    "every_second_column": lambda kind: _pattern(kind, lambda r, c: c % 2 == 0),
    "all_zero": lambda kind: np.zeros((40, 58, 64), np.uint8 if kind == "u8" else np.float32),
    "40x250x768_structured": lambda kind: CR.cached_structured(40, 250, 768, 22, kind)[0],
    # capacity 2^20 = 1024 blocks of the cluster launches, the most there are: the scan's one tile is full, its last thread owns real slots
    "1x1024x1024_isolated": lambda kind: _pattern(kind, lambda r, c: (r % 3 == 1) & (c % 3 == 0), side=1024),
}


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    return CASES[case](kind)


@functools.lru_cache(maxsize=None)
def _reference(case, kind, threshold):
    """The checker's result of a case: computed once, shared by the tests, never written."""
    return CR.clusters(_case(case, kind), threshold)


def _check(c, ref, tag):
    """A ``PXDClusters`` against the checker's dict; prints the figures before it asserts."""
    M, T = ref["label"].size, ref["total"]
    got_m, got_t = int(c.digits.total.cpu()), int(c.total.cpu())
    print(f"{tag}: digits {got_m} (checker {M}) clusters {got_t} (checker {T}) capacity {c.capacity} "
          f"largest {int(ref['size'].max()) if T else 0}")
    assert c.label.dtype == torch.int32 and c.seed.dtype == torch.uint8 and c.counts.dtype == torch.int32 and c.total.shape == (1,)
    assert all(getattr(c, k).dtype == torch.int32 for k in TABLE if k != "seed")
    assert got_m == M and got_t == T, tag
    assert M <= c.capacity, (tag, "the test's capacity is too small")
    assert np.array_equal(c.counts.cpu().numpy(), ref["counts"]), tag
    assert np.array_equal(c.digits.index[:M].cpu().numpy(), ref["index"]), tag
    assert np.array_equal(c.label[:M].cpu().numpy(), ref["label"]), tag
    for k in TABLE:
        assert np.array_equal(getattr(c, k)[:T].cpu().numpy(), ref[k]), (tag, k)


@pytest.mark.parametrize("threshold", [0.0, 7.0])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_against_checker(case, kind, threshold):
    import utils
    ev = _case(case, kind)
    ref = _reference(case, kind, threshold)
    n, h, w = ev.shape
    at = lambda cl, flat: int(cl["label"][np.searchsorted(cl["index"], flat)])
    # first, on the CPU: the case really holds what it is there for
    if case.endswith("structured"):
        plants = CR.cached_structured(n, h, w, 21 if n == 4 else 22, kind)[1]
        for name in ("snake", "spiral", "u") + tuple(f"corner{k}_3" for k in range(4)):
            assert ref["size"][at(ref, plants[name][0])] == plants[name][1], name
        assert plants["snake"][1] > 4 * 256 and plants["u"][1] >= 6 * h           # a snake across many waves' parts, two big arms
        for pair in ("wrap", "image", "column"):
            assert at(ref, plants[pair + "_a"][0]) != at(ref, plants[pair + "_b"][0]), pair
        L = plants["diagonal"][1]
        whole, cut = _reference(case, kind, 0.0), _reference(case, kind, 7.0)
        assert whole["size"][at(whole, plants["diagonal"][0])] == L == whole["size_u"][at(whole, plants["diagonal"][0])]
        assert cut["size"][at(cut, plants["diagonal"][0])] == L // 2                # the value in [6.78, 7) splits the chain at the cut
    elif case == "7x13x37":
        assert ref["size"].max() >= 15 and ref["total"] > 50
    elif case == "one_all_hit":
        assert ref["total"] == 1 and ref["size"][0] == 192000 and ref["seed"][0] == 255 and CR.size_bin(ref["size"])[0] == 63
        assert ref["size_u"][0] == 250 and ref["size_v"][0] == 768
    elif case == "checkerboard":
        assert ref["total"] == 1 and ref["size"][0] == 2048 and ref["size_u"][0] == ref["size_v"][0] == 64
    elif case == "every_second_column":
        assert ref["total"] == 32 and (ref["size"] == 64).all() and (ref["size_v"] == 1).all() and (ref["size_u"] == 64).all()
    elif case == "all_zero":
        assert ref["total"] == 0 and ref["label"].size == 0
    elif case == "1x1024x1024_isolated":
        assert ref["total"] == ref["label"].size == 341 * 342 == 116622 and (ref["size"] == 1).all() and ev.size == 1024 * 1024
    cap = ev.size if ev.size < 2 * 10 ** 6 else None
    c = utils.pxd_clusters(torch.from_numpy(ev).to(DEV), threshold=threshold, capacity=cap, n_sensors=n)
    assert c.label.is_cuda and c.capacity == (ev.size if ev.size < 2 * 10 ** 6 else max(1024, ev.size // 16)) == c.digits.capacity
    _check(c, ref, f"{case} {kind} cut {threshold}")
    host = c.cpu()
    for k in ("index", "digit_charge", "label", "counts") + TABLE:
        assert np.array_equal(host[k], ref[k]) and host[k].dtype == ref[k].dtype, k
    image = ref["first"].astype(np.int64) // (h * w)
    assert np.array_equal(host["sensor"], image % n) and np.array_equal(host["event"], image // n)
    # the same through an existing PXDDigits
    d = utils.pxd_digits(torch.from_numpy(ev).to(DEV), threshold=threshold, capacity=cap, n_sensors=n)
    c2 = utils.pxd_clusters(d)
    assert c2.digits is d
    _check(c2, ref, f"{case} {kind} cut {threshold}, from digits")


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_all_zero_writes_nothing(kind):
    """Straight through the C ABI on sentinel-filled outputs: an event without digits leaves label and table untouched."""
    import _hip as H
    import utils
    n, h, w, cap = 40, 58, 64, 4096
    d = utils.pxd_digits(torch.zeros(n, h, w, dtype=torch.uint8 if kind == "u8" else torch.float32, device=DEV), capacity=cap)
    out = {k: torch.full((cap,), -77, dtype=torch.int32, device=DEV) for k in ("label",) + TABLE if k != "seed"}
    out["seed"] = torch.full((cap,), 0xAB, dtype=torch.uint8, device=DEV)
    hdr = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.empty(H.lib().ieagan_pxd_clusters_scratch(n, h, w, cap), dtype=torch.int32, device=DEV)
    H.call("ieagan_pxd_clusters", d.index.data_ptr(), d.charge.data_ptr(), d.total.data_ptr(), n, h, w, cap, out["label"].data_ptr(),
           out["first"].data_ptr(), out["size"].data_ptr(), out["charge"].data_ptr(), out["seed"].data_ptr(), out["size_u"].data_ptr(),
           out["size_v"].data_ptr(), hdr.data_ptr(), hdr.data_ptr() + 4 * n, scratch.data_ptr(), H.stream())
    torch.cuda.synchronize()
    assert bool((hdr == 0).all())                       # counts and total are always written
    for k, t in out.items():
        assert bool((t == (0xAB if k == "seed" else -77)).all()), k


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_view_one_element_past_a_16_byte_boundary(kind):
    import utils
    ev = _synthetic(kind, 6, 21, 53, seed=3, p_hit=0.2)
    t = torch.from_numpy(ev).to(DEV)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:].copy_(t.reshape(-1))
    view = buf[1:].view(6, 21, 53)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    for thr in (0.0, 7.0):
        c = utils.pxd_clusters(view, threshold=thr, capacity=ev.size, n_sensors=3)
        assert c.digits.images.data_ptr() == view.data_ptr()
        _check(c, CR.clusters(ev, thr), f"{kind} offset view, cut {thr}")


@pytest.mark.parametrize("case", ["7x13x37", "4x64x96_structured"])
def test_label_is_consistent_with_the_table(case):
    import utils
    ev = _case(case, "f32")
    c = utils.pxd_clusters(torch.from_numpy(ev).to(DEV), capacity=ev.size, n_sensors=ev.shape[0])
    M, T = int(c.digits.total.cpu()), int(c.total.cpu())
    assert M > T > 0
    label, index = c.label[:M].cpu().numpy(), c.digits.index[:M].cpu().numpy()
    first, size = c.first[:T].cpu().numpy(), c.size[:T].cpu().numpy()
    assert label.min() == 0 and label.max() == T - 1
    assert np.array_equal(np.bincount(label, minlength=T), size)
    assert (first[label] <= index).all()
    at_root = first[label] == index
    assert at_root.sum() == T and np.array_equal(index[at_root], first) and (np.diff(first) > 0).all()
    assert np.array_equal(np.bincount(label, weights=c.digits.charge[:M].cpu().numpy(), minlength=T).astype(np.int64), c.charge[:T].cpu().numpy())


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_capacity_below_the_digit_total_touches_nothing_beyond(kind):
    """Straight through the C ABI on buffers 64 elements longer than the capacity, pre-filled with a sentinel: the first ``capacity``
    digits are clustered, nothing is written behind them; then the Python surface, which reruns instead of truncating."""
    import _hip as H
    import utils
    ev = _case("4x64x96_structured", kind)
    n, h, w = ev.shape
    x = torch.from_numpy(ev).to(DEV)
    d = utils.pxd_digits(x, capacity=ev.size, n_sensors=n)
    index, charge, _, total = DR.digits(ev, 0.0)
    assert int(d.total.cpu()) == total > 3000
    for cap in (total // 3, 1, 0, total - 1):
        ref = CR.clusters_of_digits(index[:cap].numpy(), charge[:cap].numpy(), ev.shape)
        out = {k: torch.full((cap + 64,), -77, dtype=torch.int32, device=DEV) for k in ("label",) + TABLE if k != "seed"}
        out["seed"] = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        hdr = torch.full((n + 1 + 64,), -1, dtype=torch.int32, device=DEV)
        scratch = torch.empty(H.lib().ieagan_pxd_clusters_scratch(n, h, w, cap), dtype=torch.int32, device=DEV)
        H.call("ieagan_pxd_clusters", d.index.data_ptr(), d.charge.data_ptr(), d.total.data_ptr(), n, h, w, cap, out["label"].data_ptr(),
               out["first"].data_ptr(), out["size"].data_ptr(), out["charge"].data_ptr(), out["seed"].data_ptr(), out["size_u"].data_ptr(),
               out["size_v"].data_ptr(), hdr.data_ptr(), hdr.data_ptr() + 4 * n, scratch.data_ptr(), H.stream())
        torch.cuda.synchronize()
        T = ref["total"]
        print(f"{kind}: capacity {cap} of {total} digits, clusters {int(hdr[n])} (checker on the first {cap} digits: {T})")
        assert int(hdr[n]) == T and np.array_equal(hdr[:n].cpu().numpy(), ref["counts"]) and bool((hdr[n + 1:] == -1).all())
        assert np.array_equal(out["label"][:cap].cpu().numpy(), ref["label"]) and bool((out["label"][cap:] == -77).all())
        for k in TABLE:
            assert np.array_equal(out[k][:T].cpu().numpy(), ref[k]), k
            assert bool((out[k][T:] == (0xAB if k == "seed" else -77)).all()), k
    # the Python surface never hands back a truncated event
    full = CR.clusters(ev, 0.0)
    c = utils.pxd_clusters(x, capacity=total // 3, n_sensors=n)
    assert c.capacity == total // 3 and int(c.digits.total.cpu()) == total
    host = c.cpu()
    assert c.capacity == total and host["label"].size == total
    for k in ("index", "digit_charge", "label", "counts") + TABLE:
        assert np.array_equal(host[k], full[k]), k


def test_statistics_refuse_an_overflowed_update():
    import utils
    ev = _case("4x64x96_structured", "u8")
    x = torch.from_numpy(ev).to(DEV)
    acc = utils.PXDClusterStatistics(n_sensors=4, threshold=0.0, capacity=1000, device=DEV)
    acc.update(x)
    with pytest.raises(RuntimeError, match="capacity="):
        acc.result()
    acc = utils.PXDClusterStatistics(n_sensors=4, threshold=0.0, capacity=ev.size, device=DEV)
    acc.update(x)
    res = acc.result()
    want = CR.spectra(_reference("4x64x96_structured", "u8", 0.0), ev.shape, 4)
    for k, v in want.items():
        assert np.array_equal(res[k], v), k


def test_two_runs_are_bit_identical():
    import utils
    ev = _case("40x250x768_structured", "f32")
    x = torch.from_numpy(ev).to(DEV)
    runs = []
    for _ in range(2):
        c = utils.pxd_clusters(x)
        acc = utils.PXDClusterStatistics(n_sensors=40, threshold=0.0, device=DEV)
        acc.update(x)
        runs.append((c, acc))
    (a, sa), (b, sb) = runs
    M, T = int(a.digits.total.cpu()), int(a.total.cpu())
    assert M > 40 * 1500 and T > 40 * 1000
    assert torch.equal(a.header, b.header) and torch.equal(a.digits.header, b.digits.header)
    assert torch.equal(a.label[:M], b.label[:M]) and torch.equal(a.digits.index[:M], b.digits.index[:M])
    for k in TABLE:
        assert torch.equal(getattr(a, k)[:T], getattr(b, k)[:T]), k
    assert torch.equal(sa.tables, sb.tables) and torch.equal(sa.clusters[0], sb.clusters[0]) and int(sa.tables.sum()) == 5 * T


def test_calls_neither_synchronise_nor_copy_and_replay_from_a_graph():
    """``pxd_clusters`` and ``PXDClusterStatistics.update`` are captured into a HIP graph: a synchronising call or a device-to-host copy
    inside a capture raises.  The replay then runs on new input in the captured buffer."""
    import utils
    evs = [R.synthetic_u8(40, 58, 64, seed=s, p_hit=0.05) for s in (9, 10)]
    refs = [CR.clusters(ev, 7.0) for ev in evs]
    sps = [CR.spectra(ref, (40, 58, 64), 40) for ref in refs]
    x = torch.from_numpy(evs[0]).to(DEV)
    acc = utils.PXDClusterStatistics(n_sensors=40, threshold=7.0, capacity=16384, device=DEV)
    utils.pxd_clusters(x, threshold=7.0, capacity=16384)       # eager: loads the library
    acc.update(x)                                              # eager: allocates the tables
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = utils.pxd_clusters(x, threshold=7.0, capacity=16384)
        acc.update(x)
    for i in (0, 1, 0):
        x.copy_(torch.from_numpy(evs[i]))
        g.replay()
        _check(c, refs[i], "graph replay")
    assert refs[0]["total"] != refs[1]["total"]
    res = acc.result()
    for k in ("size_spectrum", "charge_spectrum", "seed_spectrum", "size_u_spectrum", "size_v_spectrum"):
        assert np.array_equal(res[k], 3 * sps[0][k] + sps[1][k]), k
    assert np.array_equal(res["clusters"], np.concatenate([sps[0]["clusters"], sps[0]["clusters"]]))
    del g


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_statistics_over_three_events_against_the_checker(kind):
    import utils
    evs = [_synthetic(kind, 40, 58, 64, seed=50 + i, p_hit=0.04) for i in range(3)]
    acc = utils.PXDClusterStatistics(n_sensors=40, threshold=7.0, device=DEV)
    acc.update(torch.from_numpy(np.concatenate(evs[:2])).to(DEV))          # two events in one batch, then one
    c = acc.update(torch.from_numpy(evs[2]).to(DEV))
    assert isinstance(c, utils.PXDClusters) and c.capacity == max(1024, 40 * 58 * 64 // 16)
    res = acc.result()
    want = [CR.spectra(CR.clusters(ev, 7.0), ev.shape, 40) for ev in evs]
    assert res["n_events"] == 3 and res["clusters"].shape == (3, 40) and res["clusters"].dtype == np.int32
    assert np.array_equal(res["clusters"], np.concatenate([t["clusters"] for t in want]))
    for k in ("size_spectrum", "charge_spectrum", "seed_spectrum", "size_u_spectrum", "size_v_spectrum"):
        assert res[k].dtype == np.int64 and np.array_equal(res[k], sum(t[k] for t in want)), k
        assert res[k].sum() == res["clusters"].sum()
    assert (res["size_spectrum"][:, 1:].sum() > 0) and res["clusters"].min() > 0
    d = utils.pxd_cluster_distance(res, res)
    assert d == dict(cluster_rate_rel_err=0.0, size_w1=0.0, cluster_charge_w1=0.0, seed_w1=0.0)
    with pytest.raises(ValueError):
        acc.update(torch.from_numpy(evs[0][:, :30]).to(DEV))


KEYS_TODAY = {"which", "n_events_real", "n_events", "occ_rel_err", "charge_rel_err", "spectrum_w1"}
KEYS_CLUSTERS = {"cluster_rate_rel_err", "size_w1", "cluster_charge_w1", "seed_w1"}


def test_validate_tool_with_and_without_clusters(tmp_path):
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
        acc = utils.PXDClusterStatistics(n_sensors=40, threshold=cfg["val_threshold"], device=DEV)
        for ev in events:
            acc.update(torch.from_numpy(ev))
        sides.append(acc.result())
    want = utils.pxd_cluster_distance(*sides)
    assert all(np.isfinite(v) for v in want.values()) and want["cluster_rate_rel_err"] > 0
    recs, tables = {}, {}
    for flag in ([], ["--clusters"]):
        out = os.path.join(str(tmp_path), f"tables{len(flag)}.npz")
        p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, tool, "--synthetic", "3", "--compare", d, "--events", "3", "--out", out]
                           + flag + geom, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        recs[len(flag)] = json.loads(p.stdout.strip().splitlines()[-1])
        tables[len(flag)] = dict(np.load(out))
    print(recs)
    assert set(recs[0]) == KEYS_TODAY and set(recs[1]) == KEYS_TODAY | KEYS_CLUSTERS
    assert all(recs[1][k] == recs[0][k] for k in KEYS_TODAY)
    assert all(recs[1][k] == want[k] for k in KEYS_CLUSTERS)
    new_tables = {f"{side}_{k}" for side in ("real", "fake") for k in sides[0] if k != "n_events"}
    assert not new_tables & set(tables[0]) and set(tables[1]) - set(tables[0]) == new_tables
    for side, t in zip(("real", "fake"), sides):
        for k, v in t.items():
            if k != "n_events":
                assert np.array_equal(tables[1][f"{side}_{k}"], v), (side, k)
    for k in tables[0]:
        assert np.array_equal(tables[0][k], tables[1][k], equal_nan=True), k
