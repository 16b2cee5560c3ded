#!/usr/bin/env python3
"""Measurement of the cluster-level validation path on one MI355X: prints one JSON record, the content of
profiles/pxd_clusters.json.

    python tools/clusters_bench.py [--iters 200] [--host_repeats 3] [--out FILE]

kernel  ``ieagan_pxd_clusters`` (six launches) and ``ieagan_pxd_cluster_stats`` at 40x250x768 fp32 and uint8 (synthetic events, ~1 %
        occupancy plus planted edge values, cut at 7 ADU) through the library's own event profiler (``ieagan_prof_enable(1)``: device events
        around the launches of an entry point), with ``ieagan_pxd_digits`` in the same loop; and the host clock around ``--iters`` calls of
        ``utils.pxd_clusters`` (digits + clusters) and of ``PXDClusterStatistics.update`` (digits + clusters + spectra), ended by one
        device synchronise: what a caller pays per event, enqueue cost included.
host    the host form of the same computation on the fp32 event: ``.cpu()`` of the dense tensor, cut and truncation, labelling
        (``scipy.ndimage.label`` with ones((3, 3)) per image if scipy is importable, otherwise the tests' union-find checker), per-cluster
        sums with ``scipy.ndimage`` / NumPy; best and median of ``--host_repeats``.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "iea-gan_amd"), os.path.join(ROOT, "tests")]
import _hip as H                        # noqa: E402
import utils                            # noqa: E402
import pxd_clusters_reference as CR     # noqa: E402
import pxd_reference as R               # noqa: E402

THRESHOLD = 7.0


def device_times(iters):
    out = {}
    for kind, gen in (("f32", R.synthetic_f32), ("u8", R.synthetic_u8)):
        x = torch.from_numpy(gen(40, 250, 768, seed=31)).cuda()
        acc = utils.PXDClusterStatistics(n_sensors=40, threshold=THRESHOLD)
        for _ in range(10):                     # warm-up: code objects, allocator
            c = acc.update(x)
        torch.cuda.synchronize()
        H.prof_enable(1)
        H.call("ieagan_prof_reset")
        for _ in range(iters):
            c = acc.update(x)
        torch.cuda.synchronize()
        recs = {r["name"]: r for r in H.prof_collect()}
        H.prof_enable(0)
        rec = dict(digits=int(c.digits.total.cpu()), clusters=int(c.total.cpu()), capacity=c.capacity)
        for name in (f"pxd_digits_{kind}", "pxd_clusters", "pxd_cluster_stats"):
            r = recs[name]
            rec[name] = dict(calls=r["launches"], us_per_call=1e3 * r["ms"] / r["launches"])
        for label, fn in (("pxd_clusters_call", lambda: utils.pxd_clusters(x, threshold=THRESHOLD)), ("statistics_update_call", lambda: acc.update(x))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            rec[label] = dict(calls=iters, us_per_call_host_clock=1e6 * (time.perf_counter() - t0) / iters)
        out[kind] = rec
    return out


def host_form(x, repeats):
    """export -> .cpu() -> cut / truncate -> labelling -> per-cluster sums, on the host."""
    try:
        from scipy import ndimage
        labeller = "scipy.ndimage.label"
    except ImportError:
        ndimage, labeller = None, "tests/pxd_clusters_reference.py (NumPy / Python union-find)"
    parts = {k: [] for k in ("copy", "label", "sums", "total")}
    clusters = 0
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dense = x.cpu().numpy()
        t1 = time.perf_counter()
        if ndimage is not None:
            q = np.where(dense >= THRESHOLD, np.minimum(dense, 255.0), 0.0).astype(np.uint8)
            labels, counts = [], []
            for n in range(q.shape[0]):
                lab, cnt = ndimage.label(q[n] > 0, structure=np.ones((3, 3)))
                labels.append(lab)
                counts.append(cnt)
            t2 = time.perf_counter()
            clusters = 0
            for n, (lab, cnt) in enumerate(zip(labels, counts)):
                ids = np.arange(1, cnt + 1)
                ndimage.sum(q[n], lab, ids)
                ndimage.maximum(q[n], lab, ids)
                np.bincount(lab.ravel(), minlength=cnt + 1)
                ndimage.find_objects(lab)
                clusters += cnt
            t3 = time.perf_counter()
        else:
            cl = CR.clusters(dense, THRESHOLD)      # labelling and sums in one
            t2 = t3 = time.perf_counter()
            clusters = cl["total"]
        for k, v in (("copy", t1 - t0), ("label", t2 - t1), ("sums", t3 - t2), ("total", t3 - t0)):
            parts[k].append(v)
    return dict(labeller=labeller, clusters=clusters, repeats=repeats, cpu_threads=torch.get_num_threads(),
                **{f"{k}_ms_best": 1e3 * min(v) for k, v in parts.items()}, **{f"{k}_ms_median": 1e3 * statistics.median(v) for k, v in parts.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host_repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H.require_gpu()
    rec = dict(device=torch.cuda.get_device_name(0), geometry=[40, 250, 768], threshold=THRESHOLD, device_path=device_times(args.iters))
    x = torch.from_numpy(R.synthetic_f32(40, 250, 768, seed=31)).cuda()
    rec["host_path_f32"] = host_form(x, args.host_repeats)
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
