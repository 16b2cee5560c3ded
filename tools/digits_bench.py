#!/usr/bin/env python3
"""Measurement of the event-production path on one MI355X: prints one JSON record, the content of
profiles/pxd_digits.json.

    python tools/digits_bench.py [--events 200] [--events_per_batch 1] [--repeats 3] [--out FILE]

kernel      ``ieagan_pxd_digits`` at 40x250x768 fp32 and uint8 (synthetic events, ~1 % occupancy plus planted edge values) through the
            library's own event profiler (``ieagan_prof_enable(1)``: device events around the three launches), and ``ieagan_pxd_stats``
            on the same input beside it; bytes from the launcher's ProfScope (two reads of the input).
production  events/s at 256x768 with freshly initialised weights (output bias bisected to ~1 % occupancy) for three data paths in this process, alternated ``--repeats`` times:
            ``sparse``  produce.produce (device compaction, header + digits into pinned buffers, double-buffered);
            ``dense``   the parent commit's path: Generator(export=True) -> .cpu() -> .to(uint8) -> nonzero() -> gather, which is
                        create_g1.generate with this package's generator;
            ``none``    generation alone, no read-back, one synchronise at the end.
            Host clock around work that ends in a device synchronise; the best and the median of the repeats are reported.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "iea-gan_amd"), os.path.join(ROOT, "tests")]
import _hip as H              # noqa: E402
import produce                # noqa: E402
import train                  # noqa: E402
import utils                  # noqa: E402
import pxd_reference as R     # noqa: E402

COPY_RATE = 4.9e12            # bytes/s, the device copy rate DESIGN section 3 quotes


def kernel_times(iters=200):
    out = {}
    for kind, gen in (("f32", R.synthetic_f32), ("u8", R.synthetic_u8)):
        x = torch.from_numpy(gen(40, 250, 768, seed=31)).cuda()
        acc = utils.PXDStatistics(n_sensors=40, threshold=7.0)
        for _ in range(10):                     # warm-up: code objects, allocator
            d = utils.pxd_digits(x)
            acc.update(x)
        torch.cuda.synchronize()
        H.prof_enable(1)
        H.call("ieagan_prof_reset")
        for _ in range(iters):
            d = utils.pxd_digits(x)
            acc.update(x)
        torch.cuda.synchronize()
        recs = {r["name"]: r for r in H.prof_collect()}
        H.prof_enable(0)
        for name in (f"pxd_digits_{kind}", f"pxd_stats_{kind}"):
            r = recs[name]
            ms = r["ms"] / r["launches"]
            by = r["bytes"] / r["launches"]
            out[name] = dict(calls=r["launches"], us_per_call=1e3 * ms, bytes_per_call=by, gbytes_per_s=by / ms / 1e6,
                             share_of_copy_rate=by / (ms * 1e-3) / COPY_RATE)
        out[f"pxd_digits_{kind}"]["digits"] = int(d.total.cpu())
    return out


def calibrate_occupancy(G, cfg, target=0.01):
    """A freshly initialised generator fires on more than half of the pixels; PXD background sits near 1 %, and the cost of every read-back
    path depends on it.  Bisect the (single) bias of G's output convolution until one event has about ``target`` occupancy."""
    lo, hi, occ = -30.0, 30.0, None
    for _ in range(16):
        mid = 0.5 * (lo + hi)
        with torch.no_grad():
            G.output_layer[2].bias.fill_(mid)
        x = next(iter(produce.event_batches(G, cfg, 1, 1, 0)))
        occ = int(utils.pxd_digits(x, capacity=0).total.cpu()) / x.numel()
        lo, hi = (lo, mid) if occ > target else (mid, hi)
    return occ


def dense_path(G, cfg, n_events, seed):
    """create_g1.generate's host side on the dense export: 30.7 MB per event over PCIe, then uint8 / nonzero / gather on the host."""
    digits = 0
    for x in produce.event_batches(G, cfg, n_events, 1, seed):
        imgs = x.cpu().to(torch.uint8)
        nonzeros = imgs.nonzero(as_tuple=True)
        charges = imgs[nonzeros]
        digits += charges.numel()
    return digits


def none_path(G, cfg, n_events, per_batch, seed):
    for x in produce.event_batches(G, cfg, n_events, per_batch, seed):
        pass
    torch.cuda.synchronize()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=200)
    ap.add_argument("--events_per_batch", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H.require_gpu()
    rec = dict(device=torch.cuda.get_device_name(0), kernel=kernel_times())
    cfg = train.parse([])
    with contextlib.redirect_stdout(io.StringIO()):
        G, _ = produce.load_generator(cfg, None, synthetic=True, seed=0)
    occupancy = calibrate_occupancy(G, cfg)
    n, h, w = cfg["n_classes"], cfg["resolution"] - 6, cfg["resolution"] * cfg["H_base"]
    paths = {"sparse": lambda: produce.produce(G, cfg, args.events, args.events_per_batch, 0)[5],
             "dense": lambda: dense_path(G, cfg, args.events, 0),
             "none": lambda: none_path(G, cfg, args.events, args.events_per_batch, 0)}
    for f in paths.values():                    # warm-up of every path (plans, code objects, pinned buffers of the allocator)
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    info = {}
    for _ in range(args.repeats):               # alternate the paths: other work shares the host
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info[k] = f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    prod = dict(events=args.events, events_per_batch=args.events_per_batch, geometry=[n, h, w], weights="freshly initialised (seed 0), output bias set for the occupancy below", occupancy=occupancy)
    for k, ts in times.items():
        prod[k] = dict(events_per_s_best=args.events / min(ts), events_per_s_median=args.events / statistics.median(ts),
                       seconds=[round(t, 4) for t in ts])
    prod["sparse"].update(digits=info["sparse"]["digits"], bytes_copied_per_event=info["sparse"]["bytes_copied_per_event"],
                          host_waits=info["sparse"]["host_waits"], extra_copies=info["sparse"]["extra_copies"])
    prod["dense"].update(digits=info["dense"], bytes_copied_per_event=4 * n * h * w)
    prod["none"].update(bytes_copied_per_event=0)
    rec["production"] = prod
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
