#!/usr/bin/env python3
"""Measurement of ``utils.pxd_hits`` on one MI355X: prints one JSON record, the content of profiles/pxd_hits.json.

    python tools/hits_bench.py [--rounds 3] [--iters 300] [--produce_events 4 --produce_threshold T] [--out FILE]

``pxd_hits`` on a ``PXDClusterPositions`` against ``pxd_cluster_positions`` on the ``PXDClusters`` of the same input (it reads the same digit
list once where ``pxd_hits`` reads it twice: the natural yardstick), at 40x250x768 fp32 and uint8 (synthetic events, ~1 % occupancy plus
planted edge values, cut at 7 ADU), in the nominal geometry ``PXDGeometry.belle2``.  Each figure comes from a process of its own (``--leg``),
the two legs alternate, ``--rounds`` times; the record holds every sample, the median and the spread.  Per process: the library's own event
profiler (``ieagan_prof_enable(1)``: device events around the launches of an entry point) over ``--iters`` calls, then, with the profiler
off, the host clock around ``--iters`` calls ended by one device synchronise -- what a caller pays per call, enqueue cost included.

``--produce_events N`` (0: skip) also times ``produce.produce`` -- the region ``produce.py`` itself times for its ``events_per_s`` -- with a
freshly initialised generator at the default geometry, alternately without and with the hits, a process each.  An untrained generator
lights 91 % of the pixels and its bright regions are connected: even at ``--produce_threshold 255`` (2 % of the pixels) a sensor holds a
cluster of more digits than the hit file's uint16 ``size`` column takes, so ``produce.py --hits`` itself ends in ``write_hits``' refusal
and the rate is taken one call below it.  The record holds the largest cluster; the rates are those of the machinery on such blobs, capacity
reruns included, not of a trained generator at ~1 % occupancy.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLD = 7.0
LEGS = {"positions": "pxd_cluster_positions", "hits": "pxd_hits"}


def leg(name, kind, iters):
    """One process, one entry point: ``{device_us, host_us, digits, clusters, accepted}``."""
    sys.path[:0] = [os.path.join(ROOT, "iea-gan_amd"), os.path.join(ROOT, "tests")]
    import torch
    import _hip as H
    import utils
    import pxd_reference as R
    H.require_gpu()
    x = torch.from_numpy((R.synthetic_f32 if kind == "f32" else R.synthetic_u8)(40, 250, 768, seed=31)).cuda()
    c = utils.pxd_clusters(x, threshold=THRESHOLD)
    p = utils.pxd_cluster_positions(c)
    geometry = utils.PXDGeometry.belle2()
    call = (lambda: utils.pxd_cluster_positions(c)) if name == "positions" else (lambda: utils.pxd_hits(p, geometry))
    for _ in range(20):                     # warm-up: code objects, allocator, the geometry's upload
        call()
    torch.cuda.synchronize()
    H.prof_enable(1)
    H.call("ieagan_prof_reset")
    for _ in range(iters):
        call()
    torch.cuda.synchronize()
    device = {r["name"]: 1e3 * r["ms"] / r["launches"] for r in H.prof_collect() if r["launches"]}[LEGS[name]]
    H.prof_enable(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        call()
    torch.cuda.synchronize()
    host = 1e6 * (time.perf_counter() - t0) / iters
    return dict(device_us=device, host_us=host, digits=int(c.digits.total.cpu()), clusters=int(c.total.cpu()), accepted=int(p.total.cpu()),
                capacity=c.capacity)


def produce_leg(with_hits, events, threshold):
    """One process: the record of ``produce.produce`` with its ``events_per_s`` as ``produce.run`` computes it."""
    sys.path.insert(0, os.path.join(ROOT, "iea-gan_amd"))
    import produce
    import train
    import utils
    cfg = train.parse([])
    G, _ = produce.load_generator(cfg, None, synthetic=True, seed=0)
    hits = dict(geometry=utils.PXDGeometry.belle2(), seed_cut=0, charge_cut=0, head_tail=3) if with_hits else None
    t0 = time.perf_counter()
    out = produce.produce(G, cfg, events, 1, 0, threshold, hits)
    rec = out[5]
    rec["events_per_s"] = events / (time.perf_counter() - t0)
    if with_hits:
        rec["largest_cluster"] = int(out[6]["size"].max()) if out[6]["size"].size else 0
    return rec


def child(*argv, seconds=900):
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, *argv], capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"{argv} ended with {p.returncode}: {p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def summary(samples):
    return dict(samples=samples, median=statistics.median(samples), min=min(samples), max=max(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--produce_events", type=int, default=4)
    ap.add_argument("--produce_threshold", type=float, default=0.0, help="digit cut of the produce.py runs (ADU)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=list(LEGS) + ["produce_plain", "produce_hits"], default=None,
                    help="one measurement in this process (used by the driver)")
    ap.add_argument("--kind", choices=["f32", "u8"], default="u8")
    args = ap.parse_args()
    if args.leg:
        if args.leg.startswith("produce_"):
            print(json.dumps(produce_leg(args.leg == "produce_hits", args.produce_events, args.produce_threshold)))
        else:
            print(json.dumps(leg(args.leg, args.kind, args.iters)))
        return
    rec = dict(geometry=[40, 250, 768], threshold=THRESHOLD, iters=args.iters, rounds=args.rounds)
    for kind in ("u8", "f32"):
        runs = {name: [] for name in LEGS}
        for _ in range(args.rounds):
            for name in LEGS:               # alternated: positions, hits, positions, hits, ...
                runs[name].append(child(os.path.abspath(__file__), "--leg", name, "--kind", kind, "--iters", str(args.iters)))
        out = {k: runs["hits"][0][k] for k in ("digits", "clusters", "accepted", "capacity")}
        for name in LEGS:
            out[LEGS[name]] = dict(device_us_per_call=summary([r["device_us"] for r in runs[name]]),
                                   host_clock_us_per_call=summary([r["host_us"] for r in runs[name]]))
        out["hits_over_positions_device"] = out["pxd_hits"]["device_us_per_call"]["median"] / out["pxd_cluster_positions"]["device_us_per_call"]["median"]
        rec[kind] = out
    if args.produce_events > 0:
        rates, last = dict(plain=[], hits=[]), {}
        for _ in range(args.rounds):
            for name in rates:
                last[name] = child(os.path.abspath(__file__), "--leg", "produce_" + name, "--produce_events", str(args.produce_events),
                                   "--produce_threshold", str(args.produce_threshold))
                rates[name].append(last[name]["events_per_s"])
        rec["produce"] = dict(events=args.produce_events, weights="freshly initialised", threshold=args.produce_threshold,
                              occupancy=last["hits"]["digits"] / (args.produce_events * 40 * 250 * 768),
                              hits_per_event=last["hits"]["hits"] / args.produce_events, largest_cluster=last["hits"]["largest_cluster"],
                              host_waits=last["plain"]["host_waits"], hit_waits=last["hits"]["hit_waits"],
                              events_per_s=summary(rates["plain"]), events_per_s_with_hits=summary(rates["hits"]))
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
