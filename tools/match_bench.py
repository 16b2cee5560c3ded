#!/usr/bin/env python3
"""Measurement of the signal-hit matching on one MI355X: prints one JSON record, the content of
profiles/pxd_match.json.

    python tools/match_bench.py [--iters 50] [--warmup 10] [--out FILE]

One production-sized event, 40 x 250 x 768: a synthetic signal at about 1 % occupancy and the same signal with an independent synthetic
background of about 1 % laid over it (``PXDEventStore.overlay``), both reconstructed at 7 ADU in the nominal geometry.  Two legs:
``match``      the new call, ``utils.pxd_match`` on the two ready ``PXDHits`` (csrc/pxd_match.hip: four launches over the digit lists and
               the cluster tables);
``mixed_hits`` the chain that produces its mixed operand: ``utils.pxd_hits`` from the dense mixed images (digits -> clusters -> positions
               -> hits, kernels that predate the match).
A device event is recorded on the stream in front of each call and one behind it.  The legs alternate call by call in one process; after
``--warmup`` pairs the median, minimum and maximum of ``--iters`` calls of each are reported; both legs include the host work of their
calls (allocations, launches) where the device waits for it.  ``match_launches_us``: the four launches of the new call alone, through the
library's own event profiler.  ``ideal_us``: the bytes read and written over the device copy rate DESIGN section 3 quotes, plus the
dependent loads of one search -- ceil(log2(mixed digits)) rounds at the L2 hit latency -- which no schedule of this algorithm avoids.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "iea-gan_amd"), os.path.join(ROOT, "tests")]
import _hip as H              # noqa: E402
import utils                  # noqa: E402
import pxd_reference as R     # noqa: E402

COPY_RATE = 4.9e12            # bytes/s, the device copy rate DESIGN section 3 quotes
L2_HIT_US = 200 / 2.4e3       # about 200 cycles at 2.4 GHz for one dependent load that hits L2


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H.require_gpu()
    S, Hh, Ww = 40, 250, 768
    geometry = utils.PXDGeometry.belle2()
    a = utils.PXDEventStore.from_dense([R.synthetic_u8(S, Hh, Ww, seed=41, p_hit=0.01)])
    b = utils.PXDEventStore.from_dense([R.synthetic_u8(S, Hh, Ww, seed=43, p_hit=0.01)])
    x_signal, x_mixed = a.dense([0]), a.overlay([0], b).dense([0])
    kw = dict(head_tail=3, threshold=7.0, n_sensors=S)            # the default capacity, one digit per 16 pixels
    signal = utils.pxd_hits(x_signal, geometry, **kw)

    def mixed_hits():
        return utils.pxd_hits(x_mixed, geometry, **kw)

    mixed = mixed_hits()

    def match():
        return utils.pxd_match(signal, mixed)

    host = match().cpu()
    flags = host["flags"]
    ds, dm = (int(h.positions.clusters.digits.total[0]) for h in (signal, mixed))
    cs, cm = (int(h.positions.clusters.total[0]) for h in (signal, mixed))
    hs, hm = int(signal.total[0]), int(mixed.total[0])
    assert (flags & utils.PXD_MATCHED).all() and ds <= signal.capacity and dm <= mixed.capacity          # a true overlay, nothing truncated
    ms = {"match": [], "mixed_hits": []}
    for k in range(args.warmup + args.iters):
        for name, fn in (("match", match), ("mixed_hits", mixed_hits)):
            t = _timed(fn)
            if k >= args.warmup:
                ms[name].append(t)
    torch.cuda.synchronize()
    H.prof_enable(1)
    H.call("ieagan_prof_reset")
    for _ in range(args.iters):
        match()
    torch.cuda.synchronize()
    prof = {p["name"]: p for p in H.prof_collect()}["pxd_match"]
    H.prof_enable(0)
    rounds = math.ceil(math.log2(max(dm, 2)))
    # init writes 3 words a signal cluster and 4 a mixed cluster; digits reads index, charge and label of the signal digits and one index and
    # label of the mixed list per found digit (the probes of the search hit L2 and are counted as latency, not as bytes); clusters reads found
    # and lo, writes lo / hi where nothing was found, reads the mixed accepted list and writes the inverse map; hits reads 5 words a signal hit
    # and about 8 of its clusters, writes 13 bytes
    read = 9 * ds + 8 * ds + 8 * cs + 4 * hm + (5 + 8) * 4 * hs
    written = 12 * cs + 16 * cm + 4 * hm + 13 * hs
    ideal_us = 1e6 * (read + written) / COPY_RATE + rounds * L2_HIT_US
    rec = dict(device=torch.cuda.get_device_name(0), copy_rate_bytes_per_s=COPY_RATE, l2_hit_us=L2_HIT_US, iters=args.iters, warmup=args.warmup,
               method="device events around each call; the two legs alternate call by call in one process", geometry=[S, Hh, Ww],
               signal=dict(digits=ds, clusters=cs, hits=hs, capacity=signal.capacity), mixed=dict(digits=dm, clusters=cm, hits=hm, capacity=mixed.capacity),
               hits=dict(matched=int((flags & utils.PXD_MATCHED).astype(bool).sum()), changed=int((flags & utils.PXD_CHANGED).astype(bool).sum()),
                         shared=int((flags & utils.PXD_SHARED).astype(bool).sum())),
               match_bytes=dict(read=read, written=written), search_rounds=rounds, ideal_us=ideal_us,
               match_launches_us=1e3 * prof["ms"] / prof["launches"])
    for name, v in ms.items():
        rec[name + "_us"] = dict(median=1e3 * statistics.median(v), min=1e3 * min(v), max=1e3 * max(v))
    rec["ratio_mixed_hits_over_match"] = rec["mixed_hits_us"]["median"] / rec["match_us"]["median"]
    rec["match_over_ideal"] = rec["match_us"]["median"] / ideal_us
    rec["condition"] = "median of match below median of mixed_hits"
    rec["condition_met"] = bool(rec["match_us"]["median"] < rec["mixed_hits_us"]["median"])
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
