#!/usr/bin/env python3
"""Convert a directory of dense events into one digit file.

    pack_events.py --dataroot DIR --out FILE.npz [--n_sensors 40] [--events N]

Every ``*.npy`` under ``--dataroot`` (uint8 ``[n_sensors, H, W]`` detector images, sorted by name -- the order ``train.py`` and
``validate.py`` read them in) is compacted on the device (``utils.PXDEventStore.from_dense``: ``utils.pxd_digits`` at threshold 0, every
nonzero charge is a digit) and the digits are written in the ``produce.py`` / ``utils.write_digits`` format, which ``train.py --dataroot
FILE.npz`` and ``validate.py`` read back.  Prints one JSON line: events, digits, bytes of both forms.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import utils          # noqa: E402


def run(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataroot", required=True, help="directory with one uint8 *.npy per event")
    ap.add_argument("--out", required=True, help="the digit file (.npz)")
    ap.add_argument("--n_sensors", type=int, default=40)
    ap.add_argument("--events", type=int, default=0, help="pack only the first N events (0: all)")
    args = ap.parse_args(argv)
    files = sorted(glob.glob(os.path.join(args.dataroot, "*.npy")))
    if args.events > 0:
        files = files[:args.events]
    if not files:
        raise SystemExit(f"no *.npy events under {args.dataroot}")
    utils.H.require_gpu()
    store = utils.PXDEventStore.from_dense(files, n_sensors=args.n_sensors)
    store.save(args.out)
    rec = dict(events=len(store), digits=int(store.counts.sum()), shape=list(store.shape), n_sensors=store.n_sensors, store_bytes=store.nbytes,
               dense_bytes=len(store) * store.n_sensors * store.shape[0] * store.shape[1], file_bytes=os.path.getsize(args.out))
    print(json.dumps(rec))
    return rec


def main(argv=None):
    run(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
