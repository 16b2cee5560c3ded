#!/usr/bin/env python3
"""Measurement of the sparse event store on one MI355X: prints one JSON record, the content of
profiles/pxd_events.json.

    python tools/events_bench.py [--events 24] [--iters 50] [--warmup 10] [--bench FILE] [--out FILE]

event   one production event, 40 x 250 x 768 at about 1 % occupancy, pad 3 -> the network input fp32 [40, 1, 256, 768], two ways:
        ``store``  ``PXDEventStore.ingest`` with a device id tensor (csrc/pxd_events.hip; the digits are resident on the device);
        ``dense``  the path of ``train.py`` on a directory: ``np.load`` of the event's ``.npy`` -> ``from_numpy`` -> ``utils.ingest_event``
                   (pageable host-to-device copy of 7.7 MB, then the dense kernel).
        A device event is recorded on the stream in front of each call and one behind it; the median of ``--iters`` calls after
        ``--warmup`` is reported, with the noise drawn on the device (what training does) and without noise.  ``kernels_us``: the launches
        alone, new and dense, through the library's own event profiler (``ieagan_prof_enable(1)``), with the noise given and without.
train   ``train.run`` at 256 x 768 over ``--events`` events, once from the dense directory and once from the file ``pack_events`` makes of
        it: the host clock between the starts of consecutive train steps (the step returns Python floats, so it ends synchronised), median
        over the steps after the first 8.  ``--bench FILE``: the JSON line of ``bench.py --gpus 1`` from the same machine, set beside them.
"""
import argparse
import contextlib
import glob
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "iea-gan_amd"), os.path.join(ROOT, "tests")]
import _hip as H              # noqa: E402
import train                  # noqa: E402
import train_fns              # noqa: E402
import utils                  # noqa: E402
import pxd_reference as R     # noqa: E402

COPY_RATE = 4.9e12            # bytes/s, the device copy rate DESIGN section 3 quotes


def _median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def one_event(tmp, iters, warmup):
    ev = R.synthetic_u8(40, 250, 768, seed=31)
    path = os.path.join(tmp, "one_event.npy")
    np.save(path, ev)
    store = utils.PXDEventStore.from_dense([ev])
    ids = torch.zeros(1, dtype=torch.int32, device=store.device)
    assert torch.equal(store.ingest(ids, noise=False), utils.ingest_event(torch.from_numpy(ev), noise=False))
    digits = int(store.counts.sum())
    out_bytes = 4 * 40 * 256 * 768
    paths = {
        "store": lambda noise: store.ingest(ids, noise=noise),
        "dense": lambda noise: utils.ingest_event(torch.from_numpy(np.load(path)), noise=noise),
    }
    rec = dict(geometry=[40, 250, 768], pad=3, digits=digits, occupancy=digits / ev.size, iters=iters, warmup=warmup)
    for name, fn in paths.items():
        for tag, noise in (("noise_drawn", None), ("no_noise", False)):
            med, best = _median_ms(lambda: fn(noise), iters, warmup)
            rec[f"{name}_{tag}"] = dict(ms_median=med, ms_best=best)
    # the kernels alone, through the library's own event profiler (device events around each launch, no host work in between)
    u = torch.rand(40, 256, 768, device=store.device)
    dense = store.dense(ids)
    calls = {"pxd_event_ingest": lambda: store.ingest(ids, noise=False), "pxd_event_ingest+noise": lambda: store.ingest(ids, noise=u),
             "pxd_event_dense": lambda: store.dense(ids), "event_ingest": lambda: utils.ingest_event(dense, noise=False),
             "event_ingest+noise": lambda: utils.ingest_event(dense, noise=u)}
    rec["kernels_us"] = {}
    for name, fn in calls.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        H.prof_enable(1)
        H.call("ieagan_prof_reset")
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        r = {p["name"]: p for p in H.prof_collect()}[name.split("+")[0]]
        H.prof_enable(0)
        rec["kernels_us"][name] = dict(us_per_call=1e3 * r["ms"] / r["launches"], bytes_per_call=r["bytes"] / r["launches"],
                                       gbytes_per_s=r["bytes"] / r["ms"] / 1e6)
    # bytes: what has to move for the input of one step, per path
    rec["store_bytes"] = dict(resident_on_device=store.nbytes, host_to_device_per_step=0, file_read_per_step=0, kernel_read=5 * digits,
                              kernel_written=out_bytes)
    rec["dense_bytes"] = dict(file_read_per_step=os.path.getsize(path), host_to_device_per_step=ev.size, kernel_read=ev.size,
                              kernel_written=out_bytes)
    ideal = (5 * digits + out_bytes) / COPY_RATE
    rec["store_ideal_us_no_noise"] = 1e6 * ideal
    rec["kernel_share_of_copy_rate_no_noise"] = 1e6 * ideal / rec["kernels_us"]["pxd_event_ingest"]["us_per_call"]
    return rec


def _timed_run(argv):
    """``train.run`` with the start of every train step stamped on the host clock."""
    stamps = []
    make = train_fns.GAN_training_function

    def stamped(*a, **k):
        step = make(*a, **k)

        class Step:
            def __call__(self, x, y):
                stamps.append(time.perf_counter())
                return step(x, y)

            def __getattr__(self, name):
                return getattr(step, name)
        return Step()
    train_fns.GAN_training_function = stamped
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            train.run(train.parse(argv))
    finally:
        train_fns.GAN_training_function = make
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    return np.diff(stamps)


def training(tmp, n_events):
    d = os.path.join(tmp, "events")
    os.makedirs(d)
    for i in range(n_events):
        np.save(os.path.join(d, f"event_{i:04d}.npy"), train.synthetic_event(40, 250, 768, 500 + i))
    packed = os.path.join(tmp, "events.npz")
    store = utils.PXDEventStore.from_dense(sorted(glob.glob(os.path.join(d, "*.npy"))))
    store.save(packed)
    rec = dict(events=n_events, geometry=[40, 250, 768], dense_dir_bytes=n_events * 40 * 250 * 768, packed_file_bytes=os.path.getsize(packed),
               store_bytes=store.nbytes, skipped_steps=8)
    del store
    for tag, root in (("dense", d), ("packed", packed)):
        dt = _timed_run(["--dataroot", root, "--max_iters", str(n_events), "--num_epochs", "1", "--outputroot", os.path.join(tmp, tag)])
        steady = dt[8:]
        rec[tag] = dict(steps=int(dt.size), s_per_itr_median=float(np.median(steady)), s_per_itr_best=float(steady.min()),
                        s_per_itr_mean=float(steady.mean()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=24)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bench", default=None, help="file with the JSON line of bench.py --gpus 1 from the same machine")
    ap.add_argument("--skip_training", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H.require_gpu()
    rec = dict(device=torch.cuda.get_device_name(0), copy_rate_bytes_per_s=COPY_RATE)
    with tempfile.TemporaryDirectory() as tmp:
        rec["event"] = one_event(tmp, args.iters, args.warmup)
        if not args.skip_training:
            rec["train"] = training(tmp, args.events)
    if args.bench:
        lines = [ln for ln in open(args.bench).read().strip().splitlines() if ln.startswith("{")]
        rec["bench"] = json.loads(lines[-1])
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
