#!/usr/bin/env python3
"""Measurement of the cluster-reconstruction path on one MI355X: prints one JSON record, the content of
profiles/pxd_reco.json.

    python tools/reco_bench.py [--iters 200] [--out FILE]

``PXDClusterMaps.update`` (digits -> clusters -> positions -> maps) and, in the same session, ``PXDClusterStatistics.update`` (digits ->
clusters -> spectra) at 40x250x768 fp32 and uint8 (synthetic events, ~1 % occupancy plus planted edge values, cut at 7 ADU), without cuts
and with a seed / cluster-charge cut: every entry point through the library's own event profiler (``ieagan_prof_enable(1)``: device
events around the launches of an entry point), and the host clock around ``--iters`` calls ended by one device synchronise: what a
caller pays per event, enqueue cost included.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "iea-gan_amd"), os.path.join(ROOT, "tests")]
import _hip as H                        # noqa: E402
import utils                            # noqa: E402
import pxd_reference as R               # noqa: E402

THRESHOLD = 7.0
CUTS = ((0, 0), (30, 40))


def profiled(update, iters):
    """Per entry point: calls and microseconds per call over ``iters`` calls of ``update``; and the host clock per call."""
    for _ in range(10):                     # warm-up: code objects, allocator
        last = update()
    torch.cuda.synchronize()
    H.prof_enable(1)
    H.call("ieagan_prof_reset")
    for _ in range(iters):
        last = update()
    torch.cuda.synchronize()
    recs = {r["name"]: dict(calls=r["launches"], us_per_call=1e3 * r["ms"] / r["launches"]) for r in H.prof_collect() if r["launches"]}
    H.prof_enable(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        update()
    torch.cuda.synchronize()
    recs["update_call"] = dict(calls=iters, us_per_call_host_clock=1e6 * (time.perf_counter() - t0) / iters)
    return recs, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H.require_gpu()
    rec = dict(device=torch.cuda.get_device_name(0), geometry=[40, 250, 768], threshold=THRESHOLD, iters=args.iters)
    for kind, gen in (("f32", R.synthetic_f32), ("u8", R.synthetic_u8)):
        x = torch.from_numpy(gen(40, 250, 768, seed=31)).cuda()
        out = {}
        stats = utils.PXDClusterStatistics(n_sensors=40, threshold=THRESHOLD)
        out["cluster_statistics_update"], c = profiled(lambda: stats.update(x), args.iters)
        out.update(digits=int(c.digits.total.cpu()), clusters=int(c.total.cpu()), capacity=c.capacity)
        for seed_cut, charge_cut in CUTS:
            maps = utils.PXDClusterMaps(n_sensors=40, threshold=THRESHOLD, seed_cut=seed_cut, charge_cut=charge_cut)
            r, p = profiled(lambda: maps.update(x), args.iters)
            r["accepted"] = int(p.total.cpu())
            out[f"cluster_maps_update_cuts_{seed_cut}_{charge_cut}"] = r
        rec[kind] = out
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
