#!/usr/bin/env python3
"""Measurement of the intra-event correlations on one MI355X: prints one JSON record, the content of
profiles/pxd_correlations.json.

    python tools/corr_bench.py [--iters 50] [--warmup 10] [--out FILE]

One production-sized event, 40 x 250 x 768, synthetic at about 1 % occupancy (the event of tools/match_bench.py), digits at 7 ADU.
``digits``        the chain step that feeds the accumulator and predates it: ``utils.pxd_digits`` of the dense batch -- the yardstick;
``update_1x1`` / ``update_2x4``   ``PXDCorrelations.update`` on the ready ``PXDDigits`` at the two grids (R = 40 and R = 320): the counting
                  launches and the Gram launch (csrc/pxd_corr.hip).
A device event is recorded on the stream in front of each call and one behind it.  The legs alternate call by call in one process; after
``--warmup`` rounds the median, minimum and maximum of ``--iters`` calls of each are reported; every leg includes the host work of its
call (allocations, launches) where the device waits for it.  ``launches_us``: the launches alone, through the library's own event
profiler.  Condition: the median of an update does not exceed the median of ``digits`` plus that leg's own max - min.

Recorded without a condition: ``result()`` (rank transform, Gram of the ranks, the one read-back, the host's integer recipe) at 1 000 and
10 000 accumulated events with R = 320 -- host clock around the call, which ends in a synchronising copy -- beside the same tables from
``scipy.stats.rankdata`` and an int64 matrix product on the CPU threads the process is granted; and ``PXDValidation.update`` with every part
on against every part but the correlations.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.stats
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "iea-gan_amd"), os.path.join(ROOT, "tests")]
import _hip as H              # noqa: E402
import pxd                    # noqa: E402
import utils                  # noqa: E402
import pxd_reference as R     # noqa: E402


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


def _accumulated(E, S, regions, shape, device, seed):
    """A ``PXDCorrelations`` that holds ``E`` events: counts of about 1 % occupancy times a gamma(2, 1) / 2 multiplicity per event."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Rn = S * regions[0] * regions[1]
    mean = 0.01 * shape[0] * shape[1] / (regions[0] * regions[1])
    x = torch.from_numpy(rng.poisson(mean * rng.gamma(2.0, 0.5, (E, 1)), (E, Rn)).astype(np.int32)).to(device)
    acc = utils.PXDCorrelations(n_sensors=S, threshold=7.0, regions=regions, device=device)
    acc.device, acc.shape = torch.device(device), tuple(shape)
    acc.tables = torch.zeros(Rn * Rn + Rn + 1, dtype=torch.int64, device=device)
    pxd._gram(x, acc.tables)
    acc.counts = [x]
    return acc


def _cpu_tables(x):
    """The tables of ``result()`` from SciPy's ranks and int64 matrix products on the host."""
    t0 = time.perf_counter()
    rank2 = torch.from_numpy((2 * scipy.stats.rankdata(x, axis=0)).astype(np.int64))
    xi = torch.from_numpy(x.astype(np.int64))
    out = dict(gram=(xi.T @ xi).numpy(), sum=xi.sum(0).numpy(), rank_gram=(rank2.T @ rank2).numpy(), rank_sum=rank2.sum(0).numpy())
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    S, Hh, Ww = 40, 250, 768
    x = torch.from_numpy(R.synthetic_u8(S, Hh, Ww, seed=41, p_hit=0.01)).to(dev)
    kw = dict(n_sensors=S, threshold=7.0, device=dev)
    digits = utils.pxd_digits(x, 7.0, None, S)                  # the default capacity, one digit per 16 pixels
    total = int(digits.total[0])
    assert total <= digits.capacity
    accs = {g: utils.PXDCorrelations(regions=g, **kw) for g in ((1, 1), (2, 4))}
    legs = dict(digits=lambda: utils.pxd_digits(x, 7.0, None, S), update_1x1=lambda: accs[1, 1].update(digits),
                update_2x4=lambda: accs[2, 4].update(digits))
    rec = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, geometry=[S, Hh, Ww], digits=total,
               capacity=digits.capacity, method="device events around each call; the legs alternate call by call in one process")
    rec["update_us"] = _alternate(legs, args.warmup, args.iters)
    rec["launches_us"] = {name: _profiled(fn, args.iters) for name, fn in legs.items()}
    d = rec["update_us"]["digits"]
    rec["condition"] = "median of update <= median of digits + (max - min) of digits"
    rec["condition_bound_us"] = d["median"] + d["max"] - d["min"]
    rec["condition_met"] = {k: bool(rec["update_us"][k]["median"] <= rec["condition_bound_us"]) for k in ("update_1x1", "update_2x4")}
    # the whole bundle with and without the part
    on = utils.PXDValidation(True, True, correlations=(2, 4), **kw)
    off = utils.PXDValidation(True, True, **kw)
    rec["validation_update_us"] = _alternate(dict(with_correlations=lambda: on.update(x), without=lambda: off.update(x)), args.warmup, args.iters)
    # result() over many events
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rec["result"] = {}
    for E, reps in ((1000, 5), (10000, 3)):
        acc = _accumulated(E, S, (2, 4), (Hh, Ww), dev, seed=E)
        acc.result()                                            # warm-up: code objects, allocator
        wall = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = acc.result()
            wall.append(time.perf_counter() - t0)
        launches = _profiled(acc.result, reps)
        cpu, cpu_s = _cpu_tables(res["counts"])
        same = all(np.array_equal(cpu[k], res[k]) for k in cpu)
        result_ms = dict(median=1e3 * statistics.median(wall), min=1e3 * min(wall), max=1e3 * max(wall))
        rec["result"][str(E)] = dict(events=E, columns=int(res["sum"].size), result_ms=result_ms,
                                     ranks_launch_us=launches["pxd_ranks"], gram_launch_us=launches["pxd_gram"], compares=float(E) * E * res["sum"].size,
                                     cpu_threads=torch.get_num_threads(), cpu_rankdata_matmul_ms=1e3 * cpu_s, cpu_tables_equal=bool(same))
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
