#!/usr/bin/env python3
"""Measurement of the PXD space points and doublets on one MI355X: prints one JSON record, the content of
profiles/pxd_doublets.json.

    python tools/doublets_bench.py [--iters 30] [--warmup 5] [--out FILE]

One production-sized event, 40 x 250 x 768, synthetic at about 1 % occupancy (the sample of section 15), hits at 7 ADU with the default
capacity, ``PXDGeometry.belle2`` / ``PXDPlacement.belle2``, the default windows.
``hits``          the chain step that produces the operand and predates this work: ``utils.pxd_hits`` on the ready positions -- the yardstick;
``space_points``  ``utils.pxd_space_points`` on the ready hits: one thread per hit over the same rows, and the scan of the counts;
``doublets``      ``utils.pxd_doublets`` on the ready points with the default list capacity (count pass, scan, fill pass);
``doublets_full`` the same with a list capacity of the doublet total: the fill pass writes every doublet;
``update``        ``PXDDoubletStatistics.update`` on the ready doublets.
A device event is recorded on the stream in front of each call and one behind it.  The legs alternate call by call in one process; after
``--warmup`` rounds the median, minimum and maximum of ``--iters`` calls of each are reported; every leg includes the host work of its
call where the device waits for it.  ``launches_us``: the launches alone, through the library's own event profiler (``pxd_doublets count``
is the zeroing, the count pass and the scan, ``pxd_doublets fill`` the fill pass).  Condition, on the linear part only: the median of
``space_points`` does not exceed the median of ``hits`` plus that leg's own max - min.

The pair passes have no predecessor; their time is recorded beside an instruction bound: the pairs a pass tests (every thread of a workgroup
that holds an inner row tests every record of every tile of its event that is not skipped) times the vector instructions per pair of the
disassembly, over the 256 CUs x 4 SIMDs x 32 lanes a cycle at 2.4 GHz of section 18.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "iea-gan_amd"), os.path.join(ROOT, "tests")]
import _hip as H              # noqa: E402
import pxd                    # noqa: E402
import utils                  # noqa: E402
import pxd_reference as R     # noqa: E402

TILE = 256
VALU_PER_PAIR = {"count": 163 / 4, "fill": 224 / 4}      # vector instructions of the pair loop, unrolled four times, per pair (disassembly)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(legs, warmup, iters):
    ms = {name: [] for name in legs}
    for k in range(warmup + iters):
        for name, fn in legs.items():
            t = _timed(fn)
            if k >= warmup:
                ms[name].append(t)
    torch.cuda.synchronize()
    return {name: dict(median=1e3 * statistics.median(v), min=1e3 * min(v), max=1e3 * max(v)) for name, v in ms.items()}


def _profiled(fn, iters):
    """Mean microseconds per call of every launcher ``fn`` goes through, by the library's event profiler."""
    torch.cuda.synchronize()
    H.prof_enable(1)
    H.call("ieagan_prof_reset")
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    out = {p["name"]: 1e3 * p["ms"] / p["launches"] for p in H.prof_collect()}
    H.prof_enable(0)
    return out


def _pairs_tested(points, placement):
    """Thread x record tests of one pass, from the rows on the host: per event, the workgroups that hold an inner row times the records of
    the tiles that hold an outer row some inner sensor pairs with (all of them with the default ``pairs``)."""
    host = points.cpu()
    S, off, role = points.n_sensors, host["offsets"], host["role"]
    tested = 0
    for e in range((off.size - 1) // S):
        lo, hi = int(off[e * S]), int(off[(e + 1) * S])
        rows = np.arange(lo, hi)
        groups = np.unique((rows[role[lo:hi] == 0] - lo) // TILE).size
        tiles = np.unique((rows[role[lo:hi] == 1] - lo) // TILE)
        records = sum(min(TILE, hi - lo - int(t) * TILE) for t in tiles)
        tested += groups * TILE * records
    return tested


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    S, Hh, Ww = 40, 250, 768
    x = torch.from_numpy(R.synthetic_u8(S, Hh, Ww, seed=41, p_hit=0.01)).to(dev)
    geometry = utils.PXDGeometry.belle2()
    placement = utils.PXDPlacement.belle2(geometry)
    positions = utils.pxd_cluster_positions(x, threshold=7.0, n_sensors=S)         # the default capacity, one digit per 16 pixels
    hits = utils.pxd_hits(positions, geometry)
    points = utils.pxd_space_points(hits, placement)
    doublets = utils.pxd_doublets(points)
    total, n_hits = int(doublets.total[0]), int(hits.total[0])
    assert int(positions.clusters.digits.total[0]) <= hits.capacity
    full = utils.pxd_doublets(points, capacity=total)
    acc = utils.PXDDoubletStatistics(placement, geometry, n_sensors=S, threshold=7.0, device=dev)
    legs = dict(hits=lambda: utils.pxd_hits(positions, geometry), space_points=lambda: utils.pxd_space_points(hits, placement),
                doublets=lambda: utils.pxd_doublets(points), doublets_full=lambda: utils.pxd_doublets(points, capacity=total),
                update=lambda: acc.update(doublets))
    host = points.cpu()
    rec = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, geometry=[S, Hh, Ww], hits=n_hits,
               inner_hits=int((host["role"] == 0).sum()), outer_hits=int((host["role"] == 1).sum()), capacity=hits.capacity, doublets=total,
               windows=dict(tan_q12=doublets.tan_q12, z0_sub=doublets.z0_sub), method="device events around each call; the legs alternate call by call in one process")
    rec["call_us"] = _alternate(legs, args.warmup, args.iters)
    rec["launches_us"] = {name: _profiled(fn, args.iters) for name, fn in legs.items()}
    h = rec["call_us"]["hits"]
    rec["condition"] = "median of space_points <= median of hits + (max - min) of hits"
    rec["condition_bound_us"] = h["median"] + h["max"] - h["min"]
    rec["condition_met"] = bool(rec["call_us"]["space_points"]["median"] <= rec["condition_bound_us"])
    tested = _pairs_tested(points, placement)
    lanes_per_s = 256 * 4 * 32 * 2.4e9
    rec["pairs_tested_per_pass"] = tested
    rec["candidate_pairs"] = rec["inner_hits"] * rec["outer_hits"]
    rec["bound"] = {}
    for name, leg, key in (("count", "doublets", "pxd_doublets count"), ("fill", "doublets", "pxd_doublets fill"), ("fill_full", "doublets_full", "pxd_doublets fill")):
        valu = VALU_PER_PAIR["count" if name == "count" else "fill"]
        us = rec["launches_us"][leg][key]
        bound = 1e6 * tested * valu / lanes_per_s
        rec["bound"][name] = dict(valu_per_pair=valu, launch_us=us, bound_us=bound, ratio=us / bound)
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
