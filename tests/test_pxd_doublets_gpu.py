"""PXD space points and doublets on the device (MI355X): ``utils.pxd_space_points`` / ``utils.pxd_doublets`` /
``utils.PXDDoubletStatistics`` against the NumPy checker (tests/pxd_doublets_reference.py, itself pinned against a brute force in Python
integers in tests/test_pxd_doublets.py), at the seams of csrc/pxd_doublets.hip, the two capacity protocols, graph capture and the command
lines.

Every comparison is exact (``array_equal``): after ``rintf`` there is no float on the device.  There are no tolerances."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pxd_doublets_reference as DR
import pxd_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TILE = DR.TILE          # the rows of a workgroup and the records of an LDS tile that the edge cases below assume


def _objects(g, p):
    import utils
    geometry = utils.PXDGeometry(g.u_pitch, g.v_pitch, g.kind, g.unit_mm)
    return geometry, utils.PXDPlacement(p.origin, p.u_axis, p.v_axis, p.layer, p.pairs, p.unit_mm, geometry)


def _device(ev, g, p, win, threshold=0.0, capacity=None, doublet_capacity=None):
    import pxd
    import utils
    geometry, placement = _objects(g, p)
    S = len(g.kind)
    h = utils.pxd_hits(torch.from_numpy(ev).to(DEV), geometry, threshold=threshold, capacity=ev.size if capacity is None else capacity, n_sensors=S)
    pts = utils.pxd_space_points(h, placement)
    return pts, pxd._doublets(pts, *win, doublet_capacity)


def _check(pts, d, pt, db, tag, listed=None):
    """Device products against the checker's dicts; ``listed``: the doublets the device list must hold (default: all of them)."""
    A = pt["total"]
    assert int(pts.total.cpu()) == A, tag
    for k in ("x", "y", "z", "r", "sensor", "role"):
        assert np.array_equal(getattr(pts, k)[:A].cpu().numpy(), pt[k]), (tag, k)
    assert pts.role.dtype == torch.int8 and pts.x.dtype == torch.int32 and np.array_equal(pts.offsets.cpu().numpy(), pt["offsets"]), tag
    n = db["total"] if listed is None else listed
    inside = "both" if 0 < db["total"] < int((pt["role"] == 0).sum()) * int((pt["role"] == 1).sum()) else "one"
    print(f"{tag}: hits {A} (inner {int((pt['role'] == 0).sum())}, outer {int((pt['role'] == 1).sum())}) doublets {db['total']} listed {n} "
          f"outcomes {inside} windows {(d.tan_q12, d.z0_sub)}")
    assert int(d.total.cpu()) == db["total"], tag
    assert np.array_equal(d.partners[:A].cpu().numpy(), db["partners"]) and np.array_equal(d.event_doublets.cpu().numpy(), db["event_doublets"]), tag
    S = d.n_sensors
    assert np.array_equal(d.pair_doublets.cpu().numpy(), np.bincount(pt["sensor"][db["inner"]] * S + pt["sensor"][db["outer"]], minlength=S * S).reshape(S, S)), tag
    assert np.array_equal(d.inner[:n].cpu().numpy(), db["inner"][:n]) and np.array_equal(d.outer[:n].cpu().numpy(), db["outer"][:n]), tag
    order = db["inner"] * (A + 1) + db["outer"]
    assert (np.diff(order) > 0).all(), tag                  # ascending (inner, outer)


@pytest.mark.parametrize("threshold", [0.0, 7.0])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_default_shape_against_checker(kind, threshold):
    import utils
    ev, g, p, win, (_, _, _, pt, db) = DR.default_case(kind, threshold)
    pts, d = _device(ev, g, p, win, threshold)
    _check(pts, d, pt, db, f"default {kind} threshold {threshold}")
    assert 0 < db["total"] < int((pt["role"] == 0).sum()) * int((pt["role"] == 1).sum())             # both outcomes occur
    # the public entry point turns the windows into the same integers, and the barrel of the checker is the barrel of the package
    geometry, placement = _objects(g, p)
    assert placement.same_as(utils.PXDPlacement.barrel(geometry, DR.DEFAULT["radii"], DR.DEFAULT["ladders"], 1))
    d2 = utils.pxd_doublets(pts, dphi=DR.DEFAULT["dphi"], z0_mm=DR.DEFAULT["z0_mm"])
    assert (d2.tan_q12, d2.z0_sub) == win and torch.equal(d2.inner[:db["total"]], d.inner[:db["total"]])
    host = pts.cpu()
    assert np.array_equal(host["x_mm"], pt["x"].astype(np.float64) * g.unit_mm / 16) and host["x_mm"].dtype == np.float64
    assert np.array_equal(host["event"], (np.searchsorted(pt["offsets"], np.arange(pt["total"]), side="right") - 1) // 4)
    host = d.cpu()
    assert np.array_equal(host["inner"], db["inner"]) and np.array_equal(host["outer"], db["outer"]) and host["total"] == db["total"]


def test_events_without_an_inner_or_an_outer_hit_and_an_empty_batch():
    ev, g, p, win, _ = DR.default_case()
    ev = ev.copy()
    ev[4:6] = 0                 # event 1: sensors 0, 1 (inner) empty
    ev[10:12] = 0               # event 2: sensors 2, 3 (outer) empty
    _, _, _, pt, db = DR.chain(ev, g, p, *win)
    assert db["event_doublets"][0] > 0 and db["event_doublets"][1] == db["event_doublets"][2] == 0
    pts, d = _device(ev, g, p, win)
    _check(pts, d, pt, db, "no inner / no outer")
    zero = np.zeros((40, 58, 64), np.uint8)
    g40 = DR.uniform_geometry((58, 64), 100, 120, 40)
    p40 = DR.barrel(g40, (14.0, 22.0), (8, 12), 2)
    _, _, _, pt, db = DR.chain(zero, g40, p40, *win)
    pts, d = _device(zero, g40, p40, win)
    _check(pts, d, pt, db, "all zero")
    assert pt["total"] == 0 and db["total"] == 0 and d.cpu()["inner"].size == 0


@functools.lru_cache(maxsize=None)
def _isolated():
    """One event of 2 inner + 6 outer sensors of 64 x 64 with a hit on every third row and column: 462 hits a sensor."""
    r, c = np.mgrid[0:64, 0:64]
    one = np.where((r % 3 == 1) & (c % 3 == 0), 8 + (r * 64 + c) % 200, 0).astype(np.uint8)
    ev = np.repeat(one[None], 8, 0)
    g = DR.uniform_geometry((64, 64), 100, 120, 8)
    p = DR.barrel(g, (14.0, 22.0), (2, 6))
    win = DR.windows(1.2, 2.0)
    return ev, g, p, win, DR.chain(ev, g, p, *win)


def test_more_outer_hits_than_a_tile_and_more_inner_hits_than_a_workgroup():
    ev, g, p, win, (_, _, _, pt, db) = _isolated()
    n_in, n_out = int((pt["role"] == 0).sum()), int((pt["role"] == 1).sum())
    assert n_in == 2 * 462 > 3 * TILE and n_out == 6 * 462 > 10 * TILE and n_in % 64 and n_out % 64 and (n_in + n_out) % TILE
    assert 0 < db["total"] < n_in * n_out
    pts, d = _device(ev, g, p, win, doublet_capacity=db["total"])
    _check(pts, d, pt, db, "isolated 2 + 6 sensors")


def test_pairs_with_an_inner_sensor_and_one_entry_masked_off():
    ev, g, _, win, _ = DR.default_case()
    p = DR.barrel(g, DR.DEFAULT["radii"], (1, 1), 2)            # one ladder a layer, two sensors each: every (inner, outer) pair can occur
    full = DR.chain(ev, g, p, *win)[4]
    pairs = p.pairs.copy()
    pairs[0, :] = 0
    pairs[1, 3] = 0
    q = DR.Tables(**dict(vars(p), pairs=pairs))
    _, _, _, pt, db = DR.chain(ev, g, q, *win)
    by_pair = lambda d: np.bincount(pt["sensor"][d["inner"]] * 4 + pt["sensor"][d["outer"]], minlength=16).reshape(4, 4)
    assert (by_pair(full)[:2, 2:] > 0).all() and np.array_equal(by_pair(db), by_pair(full) * pairs)
    assert 0 < db["total"] < full["total"] and not db["partners"][pt["sensor"] == 0].any()
    pts, d = _device(ev, g, q, win)
    _check(pts, d, pt, db, "pairs masked")
    # entries outside inner x outer are zeroed by the constructor, whatever is passed
    _, placement = _objects(g, DR.Tables(**dict(vars(p), pairs=np.ones((4, 4), np.uint8))))
    assert np.array_equal(placement.pairs, p.pairs)


def test_an_ignored_sensor_between_the_others():
    ev, g, p, win, _ = DR.default_case()
    layer = np.array([0, -1, 1, 1])
    q = DR.Tables(**dict(vars(p), layer=layer, pairs=((layer[:, None] == 0) & (layer[None, :] == 1)).astype(np.uint8)))
    _, _, _, pt, db = DR.chain(ev, g, q, *win)
    assert (pt["role"] == -1).any() and db["total"] > 0 and not db["partners"][pt["role"] != 0].any()
    pts, d = _device(ev, g, q, win)
    _check(pts, d, pt, db, "layer -1")


@pytest.mark.parametrize("win", [(1, 0), (32768, 0), (1, 2 ** 23 - 1), (32768, 2 ** 23 - 1)])
def test_windows_at_their_extremes_on_a_placement_that_reaches_two_to_the_22(win):
    ev, g, _, _, _ = DR.default_case()
    p = DR.barrel(g, (70.0, 131.2), DR.DEFAULT["ladders"])
    assert np.abs(p.origin).max() >= 2 ** 22
    _, _, _, pt, db = DR.chain(ev, g, p, *win)
    assert max(np.abs(pt[k]).max() for k in "xyz") >= 2 ** 22
    pts, d = _device(ev, g, p, win, doublet_capacity=max(db["total"], 1))
    _check(pts, d, pt, db, f"extreme windows {win}")


def test_a_doublet_capacity_below_the_total_keeps_the_first_of_the_order_and_cpu_returns_all():
    ev, g, p, win, (_, _, _, pt, db) = DR.default_case()
    cap = db["total"] // 2
    pts, d = _device(ev, g, p, win, doublet_capacity=cap)
    guard = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    _check(pts, d, pt, db, "doublet capacity", listed=cap)
    assert d.inner.numel() == cap and (guard == -7).all()
    host = d.cpu()
    assert host["total"] == db["total"] and np.array_equal(host["inner"], db["inner"]) and np.array_equal(host["outer"], db["outer"])
    assert np.array_equal(host["partners"], db["partners"]) and d.doublet_capacity == db["total"]
    pts0, d0 = _device(ev, g, p, win, doublet_capacity=0)
    _check(pts0, d0, pt, db, "doublet capacity 0", listed=0)


def test_a_hit_capacity_below_the_digit_total_is_grown_by_cpu():
    ev, g, p, win, (cl, _, _, pt, db) = DR.default_case()
    digits = int(cl["index"].size)
    pts, d = _device(ev, g, p, win, capacity=digits // 2)
    assert int(pts.hits.positions.clusters.digits.total.cpu()) == digits > pts.capacity
    host = d.cpu()
    assert host["total"] == db["total"] and np.array_equal(host["inner"], db["inner"]) and np.array_equal(host["outer"], db["outer"])
    assert np.array_equal(host["partners"], db["partners"]) and np.array_equal(host["event_doublets"], db["event_doublets"])
    host = pts.cpu()
    assert np.array_equal(host["x"], pt["x"]) and np.array_equal(host["r"], pt["r"]) and np.array_equal(host["offsets"], pt["offsets"])


def test_two_calls_write_the_same_bytes():
    ev, g, p, win, (_, _, _, pt, db) = _isolated()
    a_pts, a = _device(ev, g, p, win, doublet_capacity=db["total"])
    b_pts, b = _device(ev, g, p, win, doublet_capacity=db["total"])
    for k in ("x", "y", "z", "r", "sensor", "role"):
        assert torch.equal(getattr(a_pts, k)[:pt["total"]], getattr(b_pts, k)[:pt["total"]]), k
    for k in ("partners", "event_doublets", "pair_doublets", "total", "inner", "outer"):
        n = pt["total"] if k == "partners" else None
        assert torch.equal(getattr(a, k)[:n], getattr(b, k)[:n]), k


def _statistics(g, p, **kw):
    import utils
    geometry, placement = _objects(g, p)
    return utils.PXDDoubletStatistics(placement, geometry, n_sensors=len(g.kind), threshold=0.0, dphi=DR.DEFAULT["dphi"], z0_mm=DR.DEFAULT["z0_mm"],
                                      device=DEV, **dict(dict(capacity=8192), **kw))


def test_the_accumulator_fed_in_updates_of_one_and_two_events_equals_one_update_of_three():
    import utils
    ev, g, p, win, (_, _, _, pt, db) = DR.default_case()
    want = DR.tables(pt, db, p.layer, 4)
    one, parts = _statistics(g, p), _statistics(g, p)
    one.update(torch.from_numpy(ev).to(DEV))
    parts.update(torch.from_numpy(ev[:4]).to(DEV))
    parts.update(torch.from_numpy(ev[4:]).to(DEV))
    assert torch.equal(one.tables, parts.tables)
    assert np.array_equal(one.tables[:-1].cpu().numpy(), want) and int(one.tables[-1]) == 0
    r1, r2 = one.result(), parts.result()
    assert (r1["events"], r1["inner_hits"], r1["outer_hits"], r1["doublets"], r1["candidates"]) == tuple(int(v) for v in want[:5])
    assert r1["n_events"] == 3 and np.array_equal(r1["hits"].reshape(-1), np.diff(pt["offsets"]))
    assert r1["acceptance"] == want[3] / want[4] and r1["sensor_pairs"].sum() == want[3] and r1["partners_spectrum"].sum() == want[1]
    assert all(v == 0.0 for v in utils.pxd_doublet_distance(r1, r2).values())
    assert utils.pxd_doublet_distance(r1, r2) == DR.distance(DR.result(want, 4), DR.result(want, 4))
    # a product of the chain goes in as it is; the statistics do not read the list, so its capacity does not matter; a truncated digit
    # list is refused in result()
    pts, d = _device(ev, g, p, win)
    again = _statistics(g, p)
    assert again.update(d) is d and torch.equal(again.tables, one.tables)
    small = _statistics(g, p, doublet_capacity=db["total"] // 2)
    assert small.update(pts).doublet_capacity == db["total"] // 2 and torch.equal(small.tables, one.tables)
    short = _statistics(g, p, capacity=1024)
    short.update(torch.from_numpy(ev).to(DEV))
    with pytest.raises(RuntimeError, match="PXDDoubletStatistics: 1 update.s. held more digits than the capacity of 1024"):
        short.result()
    with pytest.raises(ValueError, match="windows"):
        _statistics(g, p).update(__import__("pxd")._doublets(pts, 5, 5))


def test_doublets_and_an_update_are_captured_into_a_graph_and_replay_on_a_second_input():
    import utils
    ev, g, p, win, (_, _, _, pt, db) = DR.default_case()
    ev2 = ev[::-1].copy()                       # the same images in another order: another batch of whole events
    _, _, _, pt2, db2 = DR.chain(ev2, g, p, *win)
    geometry, placement = _objects(g, p)
    cap = ev.size
    buf = torch.from_numpy(ev).to(DEV)
    acc = _statistics(g, p, capacity=cap, doublet_capacity=cap)
    chain = lambda: utils.pxd_doublets(utils.pxd_hits(buf, geometry, capacity=cap, n_sensors=4), placement, DR.DEFAULT["dphi"], DR.DEFAULT["z0_mm"], cap)
    chain()                                     # eager: loads the library, uploads the tables
    acc.update(buf)
    acc.tables.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d = chain()
        acc.update(d)
    for images, (wpt, wdb) in ((ev, (pt, db)), (ev2, (pt2, db2))):
        buf.copy_(torch.from_numpy(images).to(DEV))
        graph.replay()
        _check(d.points, d, wpt, wdb, "captured")
    want = DR.tables(pt, db, p.layer, 4) + DR.tables(pt2, db2, p.layer, 4)
    assert np.array_equal(acc.tables[:-1].cpu().numpy(), want) and int(acc.tables[-1]) == 0
    del graph


def test_the_command_lines_against_the_checker(tmp_path):
    """``validate.py --doublets`` on two tiny synthetic directories and ``produce.py --hits --space_points`` with a fresh generator, each in a
    fresh child process."""
    n, h, w, pitch = 40, 58, 64, (50.0, 60.0)
    g = DR.uniform_geometry((h, w), 100, 120, n)
    p = DR.barrel(g, (14.0, 22.0), (8, 12), 2)
    win = DR.windows(0.3, 10.0)
    sides = {}
    for side, seed in (("real", 3), ("fake", 4)):
        os.makedirs(tmp_path / side)
        total = np.zeros(DR.COUNTERS + n * n + DR.PARTNER_BINS + DR.EVENT_BINS, np.int64)
        for k in range(2):
            ev = R.synthetic_u8(n, h, w, seed=10 * seed + k, p_hit=0.004)
            np.save(tmp_path / side / f"event_{k}.npy", ev)
            _, _, _, pt, db = DR.chain(ev, g, p, *win, threshold=7.0)
            total += DR.tables(pt, db, p.layer, n)
        sides[side] = total
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "iea-gan_amd"))
    common = ["--resolution", "64", "--H_base", "1"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "iea-gan_amd", "validate.py"), "--dataroot", str(tmp_path / "real"), "--compare",
                          str(tmp_path / "fake"), "--events", "2", "--doublets", "--uniform_pitch", *map(str, pitch), "--out", str(tmp_path / "v.npz")]
                         + common, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    want = DR.distance(DR.result(sides["real"], n), DR.result(sides["fake"], n))
    assert (rec["tan_q12"], rec["z0_sub"]) == win and sides["real"][3] > 0 and sides["fake"][3] > 0
    for k, v in want.items():
        assert rec[k] == v or (math.isnan(rec[k]) and math.isnan(v)), k
    with np.load(tmp_path / "v.npz") as t:
        for side, table in sides.items():
            assert np.array_equal(t[f"{side}_doublet_sensor_pairs"].reshape(-1), table[DR.COUNTERS:DR.COUNTERS + n * n]), side
            assert int(t[f"{side}_doublet_doublets"]) == table[3] and int(t[f"{side}_doublet_candidates"]) == table[4], side
    out = subprocess.run([sys.executable, os.path.join(ROOT, "iea-gan_amd", "produce.py"), "--synthetic-weights", "--events", "2", "--out",
                          str(tmp_path / "e.npz"), "--hits", str(tmp_path / "h.npz"), "--uniform_pitch", *map(str, pitch), "--space_points"] + common,
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import pxd_hits_reference as HR
    import utils
    hits = utils.read_hits(str(tmp_path / "h.npz"))
    with np.load(str(tmp_path / "h.npz") + ".points.npz") as t:
        points = {k: t[k] for k in t.files}
    assert np.array_equal(points["event_offsets"], hits["event_offsets"]) and hits["sensor"].size == points["x_mm"].size > 0
    # the events the child wrote, dense again, through the checker: the points of the hits in the hit file's order
    with np.load(tmp_path / "e.npz") as t:
        off, sensor, ucell, vcell, charge = (t[k] for k in utils.EVENT_COLUMNS)
    dense = np.zeros((2 * n, h, w), np.uint8)
    dense[np.repeat(np.arange(2), np.diff(off)) * n + sensor, ucell, vcell] = charge
    cl, pos, hit = HR.reco_hits(dense, (g.u_pitch, g.v_pitch, g.kind))
    pt = DR.space_points(cl["first"][pos["cluster"]].astype(np.int64) // (h * w) % n, hit["u"], hit["v"], pos["counts"], p)
    for k in "xyz":
        assert points[k + "_mm"].dtype == np.float32 and np.array_equal(points[k + "_mm"], (pt[k].astype(np.float64) * g.unit_mm / 16).astype(np.float32)), k
