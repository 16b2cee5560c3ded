"""Cluster reconstruction on the device (MI355X): the reconstruction kernels against the NumPy checker (tests/pxd_reco_reference.py, itself
pinned against ``scipy.ndimage.center_of_mass`` in tests/test_pxd_reco.py), the capacity protocol, ``utils.PXDClusterMaps`` and
``validate.py --maps``.

Every comparison is exact (``array_equal`` / ``torch.equal``; positions are compared as bit patterns): moments, ranks and map counters are
integers and a position is one IEEE division of two exact integers.  There are no tolerances."""
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
import pxd_reco_reference as RR
import pxd_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GATHERED = ("size", "charge", "seed", "size_u", "size_v")


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
    "all_zero": lambda kind: np.zeros((40, 58, 64), np.uint8 if kind == "u8" else np.float32),
    # capacity 2^20 = 1024 blocks, the most there are: the compaction ranks cross every block
    "1x1024x1024_isolated": lambda kind: _pattern(kind, lambda r, c: (r % 3 == 1) & (c % 3 == 0), side=1024),
}
CUTS = {case: [(0, 0), (100, 150)] for case in CASES}
CUTS["1x1024x1024_isolated"] = [(0, 0), (108, 0)]


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    return CASES[case](kind)


@functools.lru_cache(maxsize=None)
def _clusters(case, kind, threshold):
    """The cluster checker's result of a case: computed once, shared by the tests, never written."""
    return CR.clusters(_case(case, kind), threshold)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(p, cl, pos, tag):
    """A ``PXDClusterPositions`` against the checkers' dicts; prints the figures before it asserts."""
    T, A = cl["total"], pos["total"]
    got_t, got_a = int(p.clusters.total.cpu()), int(p.total.cpu())
    print(f"{tag}: clusters {got_t} (checker {T}) accepted {got_a} (checker {A}) capacity {p.capacity} "
          f"largest mu {int(pos['mu'].max()) if T else 0} mv {int(pos['mv'].max()) if T else 0}")
    assert p.cluster.dtype == torch.int32 and p.u.dtype == p.v.dtype == torch.float32 and p.mu.dtype == p.mv.dtype == torch.int64
    assert p.counts.dtype == torch.int32 and p.total.shape == (1,)
    assert got_t == T and got_a == A, tag
    assert np.array_equal(p.counts.cpu().numpy(), pos["counts"]), tag
    assert np.array_equal(p.mu[:T].cpu().numpy(), pos["mu"]) and np.array_equal(p.mv[:T].cpu().numpy(), pos["mv"]), tag
    assert np.array_equal(p.cluster[:A].cpu().numpy(), pos["cluster"]), tag
    assert np.array_equal(_bits(p.u[:A].cpu().numpy()), _bits(pos["u"])), tag            # bit for bit
    assert np.array_equal(_bits(p.v[:A].cpu().numpy()), _bits(pos["v"])), tag


def _check_host(host, cl, pos, shape, n_sensors, tag):
    h, w = shape[1:]
    j = pos["cluster"]
    assert set(host) == {"cluster", "u", "v", "mu", "mv", "sensor", "event", "counts"} | set(GATHERED), tag
    assert np.array_equal(host["cluster"], j) and host["cluster"].dtype == np.int32 and host["u"].dtype == host["v"].dtype == np.float32
    assert np.array_equal(_bits(host["u"]), _bits(pos["u"])) and np.array_equal(_bits(host["v"]), _bits(pos["v"])), tag
    assert np.array_equal(host["mu"], pos["mu"][j]) and np.array_equal(host["mv"], pos["mv"][j]) and host["mu"].dtype == np.int64, tag
    assert np.array_equal(host["counts"], pos["counts"]), tag
    for k in GATHERED:
        assert np.array_equal(host[k], cl[k][j]) and host[k].dtype == cl[k].dtype, (tag, k)
    image = cl["first"][j].astype(np.int64) // (h * w)
    assert np.array_equal(host["sensor"], image % n_sensors) and np.array_equal(host["event"], image // n_sensors), tag
    # the host recipe of the contract on what came back
    assert np.array_equal(_bits(host["u"]), _bits(RR.float_recipe(host["mu"], host["charge"]))), tag
    assert np.array_equal(_bits(host["v"]), _bits(RR.float_recipe(host["mv"], host["charge"]))), tag


@pytest.mark.parametrize("threshold", [0.0, 7.0])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_against_checker(case, kind, threshold):
    import utils
    ev = _case(case, kind)
    cl = _clusters(case, kind, threshold)
    n, h, w = ev.shape
    cap = ev.size
    x = torch.from_numpy(ev).to(DEV)
    c = utils.pxd_clusters(x, threshold=threshold, capacity=cap, n_sensors=n)
    for seed_cut, charge_cut in CUTS[case]:
        pos = RR.positions(cl, ev.shape, seed_cut, charge_cut)
        tag = f"{case} {kind} threshold {threshold} cuts ({seed_cut}, {charge_cut})"
        # first, on the CPU: the case really holds what it is there for
        if case == "one_all_hit":
            assert cl["total"] == 1 and pos["mu"][0] == 3138994938 > 2 ** 31 and pos["mv"][0] == 9666396989 > 2 ** 32
        elif case == "4x64x96_structured":
            assert cl["size"].max() > 4 * 256               # the snake: one cluster's moments come from many waves and workgroups
        elif case == "checkerboard":
            assert cl["total"] == 1 and cl["size"][0] == 2048
        elif case == "all_zero":
            assert cl["total"] == 0 and pos["total"] == 0
        elif case == "1x1024x1024_isolated":
            assert cl["total"] == 116622
            if seed_cut:
                share = pos["total"] / cl["total"]
                print(f"{tag}: accepted share {share:.4f}")
                assert 0.4 <= share <= 0.6 and 0 < (np.diff(pos["cluster"]) > 1).sum() > 1000      # interleaved, not one block
        if (seed_cut, charge_cut) != (0, 0) and case not in ("all_zero", "one_all_hit", "checkerboard"):
            assert 0 < pos["total"] < cl["total"], tag       # a real cut
        p = utils.pxd_cluster_positions(c, seed_cut=seed_cut, charge_cut=charge_cut)
        assert p.clusters is c and p.capacity == cap and p.u.is_cuda
        _check(p, cl, pos, tag)
        _check_host(p.cpu(), cl, pos, ev.shape, n, tag)
    # the same from the images
    seed_cut, charge_cut = CUTS[case][1]
    p = utils.pxd_cluster_positions(x, threshold=threshold, seed_cut=seed_cut, charge_cut=charge_cut, capacity=cap, n_sensors=n)
    _check(p, cl, RR.positions(cl, ev.shape, seed_cut, charge_cut), f"{case} {kind} threshold {threshold}, from images")


def _raw_positions(c, seed_cut, charge_cut, pad=64):
    """Straight through the C ABI on buffers ``pad`` elements longer than the capacity, pre-filled with sentinels."""
    import _hip as H
    n, h, w = c.shape
    cap, d = c.capacity, c.digits
    out = dict(mu=torch.full((cap + pad,), -77, dtype=torch.int64, device=DEV), mv=torch.full((cap + pad,), -77, dtype=torch.int64, device=DEV),
               cluster=torch.full((cap + pad,), -77, dtype=torch.int32, device=DEV), u=torch.full((cap + pad,), -77.0, dtype=torch.float32, device=DEV),
               v=torch.full((cap + pad,), -77.0, dtype=torch.float32, device=DEV))
    hdr = torch.full((n + 1 + pad,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.empty(H.lib().ieagan_pxd_cluster_positions_scratch(n, h, w, cap), dtype=torch.int32, device=DEV)
    ptr = lambda t: t.data_ptr() if cap else None
    H.call("ieagan_pxd_cluster_positions", ptr(d.index), ptr(d.charge), ptr(c.label), d.total.data_ptr(), ptr(c.first), ptr(c.charge), ptr(c.seed),
           c.total.data_ptr(), n, h, w, cap, seed_cut, charge_cut, out["mu"].data_ptr(), out["mv"].data_ptr(), out["cluster"].data_ptr(),
           out["u"].data_ptr(), out["v"].data_ptr(), hdr.data_ptr(), hdr.data_ptr() + 4 * n, scratch.data_ptr(), H.stream())
    torch.cuda.synchronize()
    return out, hdr


def _untouched(out, hdr, n, T, A):
    assert bool((hdr[n + 1:] == -1).all())
    for k in ("mu", "mv"):
        assert bool((out[k][T:] == -77).all()), k
    for k in ("cluster", "u", "v"):
        assert bool((out[k][A:] == -77).all()), k


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_a_cut_that_rejects_everything_and_a_batch_without_digits_write_nothing(kind):
    import utils
    ev = _case("4x64x96_structured", kind)
    n = ev.shape[0]
    cl = _clusters("4x64x96_structured", kind, 0.0)
    c = utils.pxd_clusters(torch.from_numpy(ev).to(DEV), capacity=ev.size, n_sensors=n)
    out, hdr = _raw_positions(c, 256, 0)                  # a uint8 seed never reaches 256
    assert int(hdr[n]) == 0 and bool((hdr[:n] == 0).all())
    _untouched(out, hdr, n, cl["total"], 0)
    assert np.array_equal(out["mu"][:cl["total"]].cpu().numpy(), RR.moments(cl, ev.shape)[0])       # the moments do not depend on the cut
    p = utils.pxd_cluster_positions(c, seed_cut=256)
    host = p.cpu()
    assert all(host[k].size == 0 for k in host if k != "counts") and (host["counts"] == 0).all()
    # an event without digits: counts and total only
    zero = torch.zeros(40, 58, 64, dtype=torch.uint8 if kind == "u8" else torch.float32, device=DEV)
    c = utils.pxd_clusters(zero, capacity=4096)
    out, hdr = _raw_positions(c, 0, 0)
    assert bool((hdr[:41] == 0).all())
    _untouched(out, hdr, 40, 0, 0)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_capacity_below_the_digit_total_touches_nothing_beyond(kind):
    """The first ``capacity`` digits are clustered and reconstructed, nothing is written behind the arrays; the Python surface reruns
    instead of truncating and the accumulator refuses the update."""
    import utils
    ev = _case("4x64x96_structured", kind)
    n, h, w = ev.shape
    x = torch.from_numpy(ev).to(DEV)
    index, charge, _, total = DR.digits(ev, 0.0)
    assert total > 3000
    for cap in (total // 3, 1, 0, total - 1):
        cl = CR.clusters_of_digits(index[:cap].numpy(), charge[:cap].numpy(), ev.shape)
        pos = RR.positions(cl, ev.shape, 60, 0)
        c = utils.pxd_clusters(x, capacity=cap, n_sensors=n)
        out, hdr = _raw_positions(c, 60, 0)
        T, A = cl["total"], pos["total"]
        print(f"{kind}: capacity {cap} of {total} digits, clusters {T}, accepted {int(hdr[n])} (checker {A})")
        assert int(c.digits.total.cpu()) == total and int(c.total.cpu()) == T
        assert int(hdr[n]) == A and np.array_equal(hdr[:n].cpu().numpy(), pos["counts"])
        _untouched(out, hdr, n, T, A)
        assert np.array_equal(out["mu"][:T].cpu().numpy(), pos["mu"]) and np.array_equal(out["mv"][:T].cpu().numpy(), pos["mv"])
        assert np.array_equal(out["cluster"][:A].cpu().numpy(), pos["cluster"])
        assert np.array_equal(_bits(out["u"][:A].cpu().numpy()), _bits(pos["u"])) and np.array_equal(_bits(out["v"][:A].cpu().numpy()), _bits(pos["v"]))
    # the Python surface never hands back a truncated event
    cl = _clusters("4x64x96_structured", kind, 0.0)
    pos = RR.positions(cl, ev.shape, 60, 0)
    p = utils.pxd_cluster_positions(x, seed_cut=60, capacity=total // 3, n_sensors=n)
    assert p.capacity == total // 3
    host = p.cpu()
    assert p.capacity == total == p.clusters.capacity
    _check_host(host, cl, pos, ev.shape, n, f"{kind} rerun")
    _check(p, cl, pos, f"{kind} rerun")
    acc = utils.PXDClusterMaps(n_sensors=n, threshold=0.0, seed_cut=60, capacity=1000, device=DEV)
    acc.update(x)
    with pytest.raises(RuntimeError, match="capacity="):
        acc.result()
    acc = utils.PXDClusterMaps(n_sensors=n, threshold=0.0, seed_cut=60, capacity=ev.size, device=DEV)
    acc.update(x)
    res = acc.result()
    for k, v in RR.maps(cl, pos, ev.shape, n).items():
        assert np.array_equal(res[k], v), k


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
        p = utils.pxd_cluster_positions(view, threshold=thr, seed_cut=50, charge_cut=60, capacity=ev.size, n_sensors=3)
        assert p.clusters.digits.images.data_ptr() == view.data_ptr()
        cl, pos = RR.reco(ev, thr, 50, 60)
        assert 0 < pos["total"] < cl["total"]
        _check(p, cl, pos, f"{kind} offset view, threshold {thr}")


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_two_runs_are_bit_identical(kind):
    import utils
    x = torch.from_numpy(_synthetic(kind, 40, 250, 768, seed=31)).to(DEV)
    runs = []
    for _ in range(2):
        p = utils.pxd_cluster_positions(x, threshold=7.0, seed_cut=30, charge_cut=40)
        acc = utils.PXDClusterMaps(n_sensors=40, threshold=7.0, seed_cut=30, charge_cut=40, device=DEV)
        acc.update(x)
        runs.append((p, acc))
    (a, ma), (b, mb) = runs
    T, A = int(a.clusters.total.cpu()), int(a.total.cpu())
    assert T > 40 * 1000 and 0 < A < T
    assert torch.equal(a.header, b.header) and torch.equal(a.clusters.header, b.clusters.header)
    assert torch.equal(a.mu[:T], b.mu[:T]) and torch.equal(a.mv[:T], b.mv[:T]) and torch.equal(a.cluster[:A], b.cluster[:A])
    assert torch.equal(a.u[:A].view(torch.int32), b.u[:A].view(torch.int32)) and torch.equal(a.v[:A].view(torch.int32), b.v[:A].view(torch.int32))
    assert torch.equal(ma.tables, mb.tables) and torch.equal(ma.clusters[0], mb.clusters[0])
    assert int(ma.tables[:40 * 25 * 48].sum()) == A and int(ma.tables[-1]) == 0


def test_calls_neither_synchronise_nor_copy_and_replay_from_a_graph():
    """``pxd_cluster_positions`` and ``PXDClusterMaps.update`` are captured into a HIP graph: a synchronising call or a device-to-host copy
    inside a capture raises.  The replay then runs on new input in the captured buffer."""
    import utils
    shape = (40, 58, 64)
    evs = [R.synthetic_u8(*shape, seed=s, p_hit=0.05) for s in (9, 10)]
    recos = [RR.reco(ev, 7.0, 40, 50) for ev in evs]
    tabs = [RR.maps(cl, pos, shape, 40) for cl, pos in recos]
    x = torch.from_numpy(evs[0]).to(DEV)
    acc = utils.PXDClusterMaps(n_sensors=40, threshold=7.0, seed_cut=40, charge_cut=50, capacity=16384, device=DEV)
    utils.pxd_cluster_positions(x, threshold=7.0, seed_cut=40, charge_cut=50, capacity=16384)       # eager: loads the library
    acc.update(x)                                                                                   # eager: allocates the tables
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p = utils.pxd_cluster_positions(x, threshold=7.0, seed_cut=40, charge_cut=50, capacity=16384)
        acc.update(x)
    for i in (0, 1, 0):
        x.copy_(torch.from_numpy(evs[i]))
        g.replay()
        _check(p, *recos[i], "graph replay")
    assert recos[0][1]["total"] != recos[1][1]["total"] and 0 < recos[0][1]["total"] < recos[0][0]["total"]
    res = acc.result()
    for k in ("count_map", "charge_map", "u_profile", "v_profile"):
        assert np.array_equal(res[k], 3 * tabs[0][k] + tabs[1][k]), k
    assert np.array_equal(res["clusters"], np.concatenate([tabs[0]["clusters"], tabs[0]["clusters"]]))
    del g


def _planted(kind, seed):
    """4 x 64 x 96 with a two-pixel cluster in image 1 whose centroid (12.8, 20.0) sits exactly on the edge between the u bins 4 and 5
    (12.8 / 64 * 25 = 5) and between the v bins 9 and 10 (20 / 96 * 48 = 10)."""
    ev = _synthetic(kind, 4, 64, 96, seed=seed, p_hit=0.04).copy()
    ev[1, 11:15, 19:22] = 0
    ev[1, 12, 20], ev[1, 13, 20] = 10, 40
    return ev


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_maps_over_three_events_against_the_checker(kind):
    import utils
    evs = [_planted(kind, 70 + i) for i in range(3)]
    acc = utils.PXDClusterMaps(n_sensors=4, threshold=7.0, seed_cut=20, charge_cut=30, device=DEV)
    acc.update(torch.from_numpy(np.concatenate(evs[:2])).to(DEV))          # two events in one batch, then one
    p = acc.update(torch.from_numpy(evs[2]).to(DEV))
    assert isinstance(p, utils.PXDClusterPositions) and p.capacity == max(1024, 4 * 64 * 96 // 16)
    res = acc.result()
    want = []
    for ev in evs:
        cl, pos = RR.reco(ev, 7.0, 20, 30)
        hit = np.nonzero((cl["first"][pos["cluster"]] == 64 * 96 + 12 * 96 + 20) & (cl["size"][pos["cluster"]] == 2))[0]
        assert hit.size == 1 and pos["u"][hit[0]] == np.float32(12.8) and pos["v"][hit[0]] == 20.0          # the planted cluster, accepted
        j = pos["cluster"][hit[0]]
        bu, bv = RR.bins(pos["mu"][j], pos["mv"][j], cl["charge"][j], 64, 96)
        assert (bu, bv) == (5, 10) and pos["mu"][j] * 25 == 5 * 50 * 64 and pos["mv"][j] * 48 == 10 * 50 * 96       # exactly on both edges
        assert 0 < pos["total"] < cl["total"]
        want.append(RR.maps(cl, pos, ev.shape, 4))
    assert res["n_events"] == 3 and res["clusters"].shape == (3, 4) and res["clusters"].dtype == np.int32 and res["shape"] == (64, 96)
    assert np.array_equal(res["clusters"], np.concatenate([t["clusters"] for t in want]))
    for k in ("count_map", "charge_map", "u_profile", "v_profile"):
        assert res[k].dtype == np.int64 and np.array_equal(res[k], sum(t[k] for t in want)), k
    assert res["count_map"].shape == (4, 25, 48) and res["u_profile"].shape == (4, 25) and res["v_profile"].shape == (4, 48)
    assert res["count_map"].sum() == res["clusters"].sum() and res["count_map"][1, 5, 10] >= 3 and res["clusters"].min() > 0
    d = utils.pxd_map_distance(res, res)
    assert d == dict(accepted_rate_rel_err=0.0, u_profile_w1=0.0, v_profile_w1=0.0, map_tv=0.0)
    with pytest.raises(ValueError):
        acc.update(torch.from_numpy(evs[0][:, :30]).to(DEV))


KEYS_TODAY = {"which", "n_events_real", "n_events", "occ_rel_err", "charge_rel_err", "spectrum_w1"}
KEYS_MAPS = {"accepted_rate_rel_err", "u_profile_w1", "v_profile_w1", "map_tv"}
TABLES_MAPS = ("count_map", "charge_map", "u_profile", "v_profile", "accepted_clusters")


def test_validate_tool_with_and_without_maps(tmp_path):
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
        acc = utils.PXDClusterMaps(n_sensors=40, threshold=cfg["val_threshold"], seed_cut=30, charge_cut=40, device=DEV)
        for ev in events:
            acc.update(torch.from_numpy(ev))
        sides.append(acc.result())
    want = utils.pxd_map_distance(*sides)
    assert all(np.isfinite(v) for v in want.values()) and want["map_tv"] > 0
    recs, tables = {}, {}
    for flag in ([], ["--maps", "--seed_cut", "30", "--cluster_cut", "40"]):
        out = os.path.join(str(tmp_path), f"tables{len(flag)}.npz")
        p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, tool, "--synthetic", "3", "--compare", d, "--events", "3", "--out", out]
                           + flag + geom, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        recs[len(flag)] = json.loads(p.stdout.strip().splitlines()[-1])
        tables[len(flag)] = dict(np.load(out))
    print(recs)
    assert set(recs[0]) == KEYS_TODAY and set(recs[5]) == KEYS_TODAY | KEYS_MAPS | {"seed_cut", "cluster_cut"}
    assert all(recs[5][k] == recs[0][k] for k in KEYS_TODAY)
    assert all(recs[5][k] == want[k] for k in KEYS_MAPS) and recs[5]["seed_cut"] == 30 and recs[5]["cluster_cut"] == 40
    new_tables = {f"{side}_{k}" for side in ("real", "fake") for k in TABLES_MAPS}
    assert not new_tables & set(tables[0]) and set(tables[5]) - set(tables[0]) == new_tables
    for side, t in zip(("real", "fake"), sides):
        for k in TABLES_MAPS:
            assert np.array_equal(tables[5][f"{side}_{k}"], t["clusters" if k == "accepted_clusters" else k]), (side, k)
    for k in tables[0]:
        assert np.array_equal(tables[0][k], tables[5][k], equal_nan=True), k
