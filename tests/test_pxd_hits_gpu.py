"""PXD hits on the device (MI355X): ``utils.pxd_hits`` / ``ieagan_pxd_hits`` against the NumPy checker (tests/pxd_hits_reference.py, itself
pinned against a brute force in exact rationals in tests/test_pxd_hits.py), the capacity protocol, graph capture and ``produce.py --hits``.

Every comparison is exact (``array_equal``; positions are compared as bit patterns): moments, edge charges and extents are integers and a
position is one IEEE division of two exact integers.  There are no tolerances."""
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
import pxd_hits_reference as HR
import pxd_reco_reference as RR
import pxd_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
PER_CLUSTER = ("pu", "pv", "v_start", "qh_u", "qt_u", "qh_v", "qt_v")
HOST_KEYS = {"cluster", "sensor", "event", "u", "v", "u_mm", "v_mm", "charge", "seed", "size", "size_u", "size_v", "u_start", "v_start", "flags",
             "counts"}


def _synthetic(kind, *a, **k):
    return (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(*a, **k)


def _pattern(kind, rule, side=64):
    r, c = np.mgrid[0:side, 0:side]
    ev = np.where(rule(r, c), 8 + (r * side + c) % 200, 0)[None]
    return ev.astype(np.uint8 if kind == "u8" else np.float32)


# case -> (images, column at which the v pitch of the two-type test geometry changes)
CASES = {
    "7x13x37": (lambda kind: _synthetic(kind, 7, 13, 37, seed=32, p_hit=0.3), 18),
    "4x64x96_structured": (lambda kind: CR.cached_structured(4, 64, 96, 21, kind)[0], 40),
    "checkerboard": (lambda kind: _pattern(kind, lambda r, c: (r + c) % 2 == 0), 24),
    "isolated": (lambda kind: _pattern(kind, lambda r, c: (r % 3 == 1) & (c % 3 == 0)), 24),
    "all_zero": (lambda kind: np.zeros((40, 58, 64), np.uint8 if kind == "u8" else np.float32), 24),
}
CUTS = [(0, 0), (100, 150)]


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    return CASES[case][0](kind)


@functools.lru_cache(maxsize=None)
def _clusters(case, kind, threshold):
    """The cluster checker's result of a case: computed once, shared by the tests, never written."""
    return CR.clusters(_case(case, kind), threshold)


def _geometry(case):
    import utils
    n, h, w = _case(case, "u8").shape
    return HR.two_type_geometry((h, w), CASES[case][1], n), HR.two_type_geometry((h, w), CASES[case][1], n, utils)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_arrays(got, T, A, want, tag):
    """Device arrays (a ``PXDHits`` or a dict of raw buffers) against the checker's dict; the invariant on what the device wrote."""
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    for k in PER_CLUSTER:
        assert np.array_equal(get(k)[:T].cpu().numpy(), want[k]), (tag, k)
    u, v = get("u")[:A].cpu().numpy(), get("v")[:A].cpu().numpy()
    assert np.array_equal(_bits(u), _bits(want["u"])) and np.array_equal(_bits(v), _bits(want["v"])), tag              # bit for bit
    assert np.array_equal(get("flags")[:A].cpu().numpy(), want["flags"]), tag
    # every hit lies inside [x2[lo] - p[lo], x2[hi] + p[hi]] / 2 of its own cluster (fp32 -> float64 and the doubling are exact)
    for x, axis in ((u, "u"), (v, "v")):
        assert (2 * x.astype(np.float64) >= want["lower_" + axis]).all() and (2 * x.astype(np.float64) <= want["upper_" + axis]).all(), (tag, axis)


def _check(h, cl, pos, want, tag):
    T, A = cl["total"], pos["total"]
    got_t, got_a = int(h.positions.clusters.total.cpu()), int(h.total.cpu())
    print(f"{tag}: clusters {got_t} (checker {T}) hits {got_a} (checker {A}) capacity {h.capacity} head-tail u {int(want['ht_u'].sum())} "
          f"v {int(want['ht_v'].sum())} clamped u {int(want['clamp_u'].sum())} v {int(want['clamp_v'].sum())} straddling {int(want['straddle'].sum())} "
          f"(head-tail {int((want['straddle'] & want['ht_v']).sum())})")
    assert h.pu.dtype == h.pv.dtype == torch.int64 and h.u.dtype == h.v.dtype == torch.float32 and h.flags.dtype == torch.uint8
    assert all(getattr(h, k).dtype == torch.int32 for k in PER_CLUSTER[2:]) and h.header is h.positions.header
    assert got_t == T and got_a == A == want["total"], tag
    assert np.array_equal(h.counts.cpu().numpy(), pos["counts"]), tag
    _check_arrays(h, T, A, want, tag)


def _check_host(host, cl, pos, want, shape, n_sensors, unit_mm, tag):
    h, w = shape[1:]
    j = pos["cluster"]
    assert set(host) == HOST_KEYS, tag
    assert np.array_equal(host["cluster"], j) and host["u"].dtype == host["v"].dtype == np.float32 and host["flags"].dtype == np.uint8
    assert np.array_equal(_bits(host["u"]), _bits(want["u"])) and np.array_equal(_bits(host["v"]), _bits(want["v"])), tag
    assert host["u_mm"].dtype == host["v_mm"].dtype == np.float64
    assert np.array_equal(host["u_mm"], want["u"].astype(np.float64) * unit_mm) and np.array_equal(host["v_mm"], want["v"].astype(np.float64) * unit_mm)
    assert np.array_equal(host["flags"], want["flags"]) and np.array_equal(host["counts"], pos["counts"]), tag
    assert np.array_equal(host["u_start"], want["u_start"][j]) and np.array_equal(host["v_start"], want["v_start"][j]), tag
    for k in ("charge", "seed", "size", "size_u", "size_v"):
        assert np.array_equal(host[k], cl[k][j]) and host[k].dtype == cl[k].dtype, (tag, k)
    image = cl["first"][j].astype(np.int64) // (h * w)
    assert np.array_equal(host["sensor"], image % n_sensors) and np.array_equal(host["event"], image // n_sensors), tag


@pytest.mark.parametrize("threshold", [0.0, 7.0])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_against_checker(case, kind, threshold):
    import utils
    ev = _case(case, kind)
    cl = _clusters(case, kind, threshold)
    tables, geometry = _geometry(case)
    n, h, w = ev.shape
    cap = ev.size
    x = torch.from_numpy(ev).to(DEV)
    c = utils.pxd_clusters(x, threshold=threshold, capacity=cap, n_sensors=n)
    for seed_cut, charge_cut in CUTS:
        pos = RR.positions(cl, ev.shape, seed_cut, charge_cut)
        want = HR.hits(cl, pos, ev.shape, tables)
        tag = f"{case} {kind} threshold {threshold} cuts ({seed_cut}, {charge_cut})"
        # first, on the CPU: the case really holds what it is there for
        if (seed_cut, charge_cut) == (0, 0):
            if case in ("7x13x37", "4x64x96_structured"):
                assert want["ht_u"].sum() > 0 and want["ht_v"].sum() > 0 and (~want["ht_v"]).sum() > 0, tag
                assert want["straddle"].sum() > 0 and len(set(want["type"].tolist())) == 2, tag
            if case == "7x13x37":
                assert (want["straddle"] & want["ht_v"]).sum() > 0, tag
            if case == "7x13x37" and kind == "u8" and threshold == 0.0:
                assert cl["total"] == 208 and want["ht_u"].sum() == want["ht_v"].sum() == 70 and want["straddle"].sum() == 12
                assert (want["straddle"] & want["ht_v"]).sum() == 10 and want["clamp_u"].sum() > 0 and want["clamp_v"].sum() > 0
            if case == "4x64x96_structured":
                assert cl["size"].max() > 4 * 256           # the snake: one cluster's edge charges and first column come from many waves
            if case == "checkerboard":
                assert cl["total"] == 1 and want["flags"][0] & 3 == 3 and cl["charge"][0] - want["qh_u"][0] - want["qt_u"][0] > 100000
            if case == "isolated":
                assert cl["total"] > 400 and (cl["size"] == 1).all() and (want["flags"] == 0).all()
        if case == "all_zero":
            assert cl["total"] == 0 and want["total"] == 0
        p = utils.pxd_cluster_positions(c, seed_cut=seed_cut, charge_cut=charge_cut)
        hits = utils.pxd_hits(p, geometry)
        assert hits.positions is p and hits.capacity == cap and hits.u.is_cuda and hits.head_tail == 3 and hits.geometry is geometry
        _check(hits, cl, pos, want, tag)
        _check_host(hits.cpu(), cl, pos, want, ev.shape, n, geometry.unit_mm, tag)
    # centre of gravity only, and head-tail from four cells on
    pos = RR.positions(cl, ev.shape, 0, 0)
    p = utils.pxd_cluster_positions(c)
    for head_tail in (0, 4):
        _check(utils.pxd_hits(p, geometry, head_tail), cl, pos, HR.hits(cl, pos, ev.shape, tables, head_tail), f"{case} {kind} head_tail {head_tail}")


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_from_images_clusters_and_positions_the_same_bytes(kind):
    import utils
    case = "7x13x37"
    ev = _case(case, kind)
    _, geometry = _geometry(case)
    n = ev.shape[0]
    x = torch.from_numpy(ev).to(DEV)
    kw = dict(threshold=7.0, seed_cut=100, charge_cut=150, capacity=ev.size, n_sensors=n)
    c = utils.pxd_clusters(x, threshold=7.0, capacity=ev.size, n_sensors=n)
    runs = [utils.pxd_hits(x, geometry, **kw), utils.pxd_hits(c, geometry, seed_cut=100, charge_cut=150),
            utils.pxd_hits(utils.pxd_cluster_positions(c, seed_cut=100, charge_cut=150), geometry)]
    assert runs[1].positions.clusters is c and runs[0].seed_cut == runs[1].seed_cut == runs[2].seed_cut == 100
    T, A = int(c.total.cpu()), int(runs[0].total.cpu())
    assert 0 < A < T
    for other in runs[1:]:
        assert torch.equal(runs[0].header, other.header)
        for k in PER_CLUSTER:
            assert torch.equal(getattr(runs[0], k)[:T], getattr(other, k)[:T]), k
        for k in ("u", "v"):
            assert torch.equal(getattr(runs[0], k)[:A].view(torch.int32), getattr(other, k)[:A].view(torch.int32)), k
        assert torch.equal(runs[0].flags[:A], other.flags[:A])
    with pytest.raises(ValueError, match="the geometry has"):
        utils.pxd_hits(c, utils.PXDGeometry.uniform((13, 36), 100, 110, n_sensors=n))
    with pytest.raises(ValueError, match="the geometry has"):
        utils.pxd_hits(c, utils.PXDGeometry.uniform((13, 37), 100, 110, n_sensors=n + 1))
    with pytest.raises(ValueError, match="head_tail = 2"):
        utils.pxd_hits(c, geometry, head_tail=2)


def _raw_hits(p, geometry, head_tail=3, pad=64):
    """Straight through the C ABI on buffers ``pad`` elements longer than the capacity, pre-filled with sentinels."""
    import _hip as H
    c, d = p.clusters, p.clusters.digits
    n, h, w = p.shape
    cap = p.capacity
    full = lambda dtype: torch.full((cap + pad,), -77, dtype=dtype, device=DEV)
    out = dict(pu=full(torch.int64), pv=full(torch.int64), **{k: full(torch.int32) for k in PER_CLUSTER[2:]}, u=full(torch.float32),
               v=full(torch.float32), flags=torch.full((cap + pad,), 177, dtype=torch.uint8, device=DEV))
    t = geometry.tables(torch.device(DEV))
    ptr = lambda x: x.data_ptr() if cap else None
    H.call("ieagan_pxd_hits", ptr(d.index), ptr(d.charge), ptr(c.label), d.total.data_ptr(), ptr(c.first), ptr(c.charge), ptr(c.size_u),
           ptr(c.size_v), c.total.data_ptr(), ptr(p.cluster), p.total.data_ptr(), *(t[k].data_ptr() for k in geometry.TABLES), n, h, w, p.n_sensors,
           geometry.K, cap, head_tail, *(out[k].data_ptr() for k in PER_CLUSTER + ("u", "v", "flags")), None, H.stream())
    torch.cuda.synchronize()
    return out


def _untouched(out, T, A):
    for k in PER_CLUSTER:
        assert bool((out[k][T:] == -77).all()), k
    assert bool((out["u"][A:] == -77).all()) and bool((out["v"][A:] == -77).all()) and bool((out["flags"][A:] == 177).all())


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_a_cut_that_rejects_everything_and_a_batch_without_digits_write_nothing(kind):
    import utils
    case = "4x64x96_structured"
    ev = _case(case, kind)
    tables, geometry = _geometry(case)
    n = ev.shape[0]
    cl = _clusters(case, kind, 0.0)
    c = utils.pxd_clusters(torch.from_numpy(ev).to(DEV), capacity=ev.size, n_sensors=n)
    p = utils.pxd_cluster_positions(c, seed_cut=256)                # a uint8 seed never reaches 256
    out = _raw_hits(p, geometry)
    assert int(p.total.cpu()) == 0
    _untouched(out, cl["total"], 0)
    want = HR.per_cluster(cl, ev.shape, *tables)                   # the per-cluster tables do not depend on the cut
    for k in PER_CLUSTER:
        assert np.array_equal(out[k][:cl["total"]].cpu().numpy(), want[k]), k
    host = utils.pxd_hits(p, geometry).cpu()
    assert set(host) == HOST_KEYS and all(host[k].size == 0 for k in host if k != "counts") and (host["counts"] == 0).all()
    # an event without digits: nothing at all
    zero = torch.zeros(40, 58, 64, dtype=torch.uint8 if kind == "u8" else torch.float32, device=DEV)
    p = utils.pxd_cluster_positions(zero, capacity=4096)
    _untouched(_raw_hits(p, _geometry("all_zero")[1]), 0, 0)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_capacity_below_the_digit_total_touches_nothing_beyond(kind):
    """The first ``capacity`` digits are clustered and reconstructed, nothing is written behind the arrays; ``cpu()`` reruns instead of
    truncating."""
    import utils
    case = "4x64x96_structured"
    ev = _case(case, kind)
    tables, geometry = _geometry(case)
    n, h, w = ev.shape
    x = torch.from_numpy(ev).to(DEV)
    index, charge, _, total = DR.digits(ev, 0.0)
    assert total > 3000
    for cap in (total // 3, 1, 0, total - 1):
        cl = CR.clusters_of_digits(index[:cap].numpy(), charge[:cap].numpy(), ev.shape)
        pos = RR.positions(cl, ev.shape, 60, 0)
        want = HR.hits(cl, pos, ev.shape, tables)
        p = utils.pxd_cluster_positions(x, seed_cut=60, capacity=cap, n_sensors=n)
        out = _raw_hits(p, geometry)
        T, A = cl["total"], pos["total"]
        print(f"{kind}: capacity {cap} of {total} digits, clusters {T}, hits {int(p.total.cpu())} (checker {A}), head-tail v {int(want['ht_v'].sum())}")
        assert int(p.clusters.digits.total.cpu()) == total and int(p.clusters.total.cpu()) == T and int(p.total.cpu()) == A
        _untouched(out, T, A)
        _check_arrays(out, T, A, want, f"{kind} capacity {cap}")
    # the Python surface never hands back a truncated event
    cl = _clusters(case, kind, 0.0)
    pos = RR.positions(cl, ev.shape, 60, 0)
    want = HR.hits(cl, pos, ev.shape, tables)
    hits = utils.pxd_hits(x, geometry, seed_cut=60, capacity=total // 3, n_sensors=n)
    assert hits.capacity == total // 3
    host = hits.cpu()
    assert hits.capacity == total == hits.positions.capacity == hits.positions.clusters.capacity and hits.geometry is geometry
    _check_host(host, cl, pos, want, ev.shape, n, geometry.unit_mm, f"{kind} rerun")
    _check(hits, cl, pos, want, f"{kind} rerun")


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_view_one_element_past_a_16_byte_boundary(kind):
    import utils
    ev = _synthetic(kind, 6, 21, 53, seed=3, p_hit=0.2)
    tables = HR.two_type_geometry((21, 53), 30, 3)
    geometry = utils.PXDGeometry(*tables)
    t = torch.from_numpy(ev).to(DEV)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:].copy_(t.reshape(-1))
    view = buf[1:].view(6, 21, 53)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    for thr in (0.0, 7.0):
        hits = utils.pxd_hits(view, geometry, threshold=thr, seed_cut=50, charge_cut=60, capacity=ev.size, n_sensors=3)
        assert hits.images.data_ptr() == view.data_ptr()
        cl, pos, want = HR.reco_hits(ev, tables, 3, thr, 50, 60)
        assert 0 < pos["total"] < cl["total"] and want["ht_v"].sum() > 0
        _check(hits, cl, pos, want, f"{kind} offset view, threshold {thr}")


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_two_runs_are_bit_identical_and_every_hit_lies_inside_its_cluster(kind):
    import utils
    ev = _synthetic(kind, 40, 58, 64, seed=9, p_hit=0.05)
    tables = HR.two_type_geometry((58, 64), 24, 40)
    geometry = utils.PXDGeometry(*tables)
    x = torch.from_numpy(ev).to(DEV)
    a, b = (utils.pxd_hits(x, geometry, threshold=7.0, seed_cut=30, charge_cut=40) for _ in range(2))
    T, A = int(a.positions.clusters.total.cpu()), int(a.total.cpu())
    assert T > 1000 and 0 < A < T
    assert torch.equal(a.header, b.header)
    for k in PER_CLUSTER:
        assert torch.equal(getattr(a, k)[:T], getattr(b, k)[:T]), k
    assert torch.equal(a.u[:A].view(torch.int32), b.u[:A].view(torch.int32)) and torch.equal(a.v[:A].view(torch.int32), b.v[:A].view(torch.int32))
    assert torch.equal(a.flags[:A], b.flags[:A])
    cl, pos, want = HR.reco_hits(ev, tables, 3, 7.0, 30, 40)
    _check(a, cl, pos, want, f"{kind} 40x58x64")           # holds the invariant on the device's own positions
    host = a.cpu()
    length = np.stack([geometry.u_length, geometry.v_length])[:, geometry.kind[host["sensor"]]] * geometry.unit_mm
    assert (np.abs(host["u_mm"]) <= length[0] / 2).all() and (np.abs(host["v_mm"]) <= length[1] / 2).all()       # inside the sensor


def test_capture_into_a_graph_and_replay_on_new_input():
    """``pxd_hits`` is captured into a HIP graph -- a synchronising call or a device-to-host copy inside a capture raises -- and the replay
    runs on new input in the captured buffer."""
    import utils
    shape = (40, 58, 64)
    tables = HR.two_type_geometry(shape[1:], 24, 40)
    geometry = utils.PXDGeometry(*tables)
    evs = [R.synthetic_u8(*shape, seed=s, p_hit=0.05) for s in (9, 10)]
    wants = [HR.reco_hits(ev, tables, 3, 7.0, 40, 50) for ev in evs]
    x = torch.from_numpy(evs[0]).to(DEV)
    kw = dict(threshold=7.0, seed_cut=40, charge_cut=50, capacity=16384)
    utils.pxd_hits(x, geometry, **kw)                       # eager: loads the library, uploads the tables
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hits = utils.pxd_hits(x, geometry, **kw)
    for i in (0, 1, 0):
        x.copy_(torch.from_numpy(evs[i]))
        g.replay()
        _check(hits, *wants[i], "graph replay")
    assert wants[0][1]["total"] != wants[1][1]["total"] and 0 < wants[0][1]["total"] < wants[0][0]["total"]
    del g


def test_produce_tool_with_and_without_hits(tmp_path):
    """``produce.py --hits`` as a child process: the hit file equals ``pxd_hits`` on the dense export of the same events, the digit file's
    columns are byte for byte those of a run without ``--hits`` (the ``.npz`` container stamps the time of writing) and ``host_waits`` is
    unchanged."""
    import produce
    import train
    import utils
    tool = os.path.join(ROOT, "iea-gan_amd", "produce.py")
    geom = ["--resolution", "64", "--H_base", "1"]
    recs, files = {}, {}
    for name, flags in (("plain", []), ("hits", ["--hits", os.path.join(str(tmp_path), "hit_file.npz"), "--seed_cut", "9", "--cluster_cut", "12",
                                                 "--uniform_pitch", "50", "55"])):
        out = os.path.join(str(tmp_path), f"{name}.npz")
        p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, tool, "--synthetic-weights", "--events", "3", "--events_per_batch", "2",
                            "--seed", "11", "--out", out] + flags + geom, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        recs[name] = json.loads(p.stdout.strip().splitlines()[-1])
        files[name] = dict(np.load(out))
    print(recs)
    assert set(recs["hits"]) == set(recs["plain"]) | {"hits", "hit_waits"} and recs["hits"]["hit_waits"] == 2
    assert recs["hits"]["host_waits"] == recs["plain"]["host_waits"] == 2 and recs["hits"]["digits"] == recs["plain"]["digits"] > 0
    assert set(files["hits"]) == set(files["plain"]) == set(utils.EVENT_COLUMNS)
    for k, v in files["plain"].items():
        assert files["hits"][k].dtype == v.dtype and files["hits"][k].tobytes() == v.tobytes(), k
    assert "hits" not in json.load(open(os.path.join(str(tmp_path), "plain.npz.json")))
    assert json.load(open(os.path.join(str(tmp_path), "hits.npz.json")))["seed_cut"] == 9
    # the same events, dense, in this process
    cfg = train.parse(geom)
    G, _ = produce.load_generator(cfg, None, synthetic=True, seed=11)
    dense = torch.cat(list(produce.event_batches(G, cfg, 3, 2, 11)))
    assert dense.shape == (120, 58, 64)
    geometry = utils.PXDGeometry.uniform((58, 64), 100, 110)
    host = utils.pxd_hits(dense, geometry, seed_cut=9, charge_cut=12).cpu()
    got = utils.read_hits(os.path.join(str(tmp_path), "hit_file.npz"))
    assert got["unit_mm"] == geometry.unit_mm and got["event_offsets"].tolist() == [0] + np.cumsum(host["counts"].reshape(3, 40).sum(1)).tolist()
    assert recs["hits"]["hits"] == got["event_offsets"][-1] == host["u"].size > 0
    for k in list(utils.HIT_COLUMNS)[1:]:
        assert got[k].dtype == utils.HIT_COLUMNS[k] and np.array_equal(got[k], host[k].astype(utils.HIT_COLUMNS[k])), k
    assert np.array_equal(_bits(got["u_mm"]), _bits((host["u"].astype(np.float64) * 5e-4).astype(np.float32)))
    # the nominal geometry is known for 250 x 768 x 40 only
    with pytest.raises(SystemExit, match="--uniform_pitch"):
        produce.hit_geometry(cfg)
    with pytest.raises(SystemExit, match="0.5 um"):
        produce.hit_geometry(cfg, (50.0, 55.3))
