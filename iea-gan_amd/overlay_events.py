#!/usr/bin/env python3
"""Lay background events over signal events, digit file in, digit file out.

    overlay_events.py --signal SIGNAL.npz --background BG.npz --out MIXED.npz [--events N] [--seed K] [--shape H W] [--n_sensors S]

Both inputs are digit files in the ``produce.py`` / ``pack_events.py`` / ``utils.write_digits`` format.  Output event ``k`` is signal event
``k % len(signal)`` with background event ``perm[k % len(background)]`` laid over it: every pixel that is a digit in either, charges of a
pixel in both summed and saturated at 255 (``utils.pxd_overlay``: a merge of the two sorted digit lists on the device, no dense image).
``perm`` is a permutation of the background events drawn from ``--seed`` (``numpy.random.default_rng(seed).permutation``); without
``--seed`` it is the identity.  ``--events`` defaults to the number of signal events.

Writes ``MIXED.npz`` (``PXDEventStore.save``) and ``MIXED.npz.json``: ``events``, ``signal_digits``, ``background_digits``, ``digits`` and
``shared``, the number of pixels that held a digit on both sides (``signal_digits + background_digits - digits``).  Prints that record as
one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def pairs(n_signal, n_background, events, seed=None):
    """``(signal ids, background ids)`` of the ``events`` output events."""
    perm = np.arange(n_background) if seed is None else np.random.default_rng(seed).permutation(n_background)
    k = np.arange(events)
    return (k % n_signal).astype(np.int64), perm[k % n_background].astype(np.int64)


def run(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--signal", required=True, help="digit file of the signal events (.npz)")
    ap.add_argument("--background", required=True, help="digit file of the background events (.npz)")
    ap.add_argument("--out", required=True, help="the digit file of the mixed events (.npz); the record goes to OUT.json")
    ap.add_argument("--events", type=int, default=0, help="number of output events (0: one per signal event)")
    ap.add_argument("--seed", type=int, default=None, help="seed of the permutation of the background events (default: identity)")
    ap.add_argument("--shape", type=int, nargs=2, default=(250, 768), metavar=("H", "W"))
    ap.add_argument("--n_sensors", type=int, default=40)
    args = ap.parse_args(argv)
    import torch
    import utils
    utils.H.require_gpu()
    shape, S = tuple(args.shape), args.n_sensors
    signal = utils.PXDEventStore.from_file(args.signal, shape, S)
    background = utils.PXDEventStore.from_file(args.background, shape, S)
    if not len(signal) or not len(background):
        raise SystemExit("overlay_events: a file without events")
    n = args.events if args.events > 0 else len(signal)
    ids_s, ids_b = pairs(len(signal), len(background), n, args.seed)
    step = max(1, 65535 // S)                   # events of one call
    parts, shared = [], 0
    for k in range(0, n, step):
        ov = utils.pxd_overlay(signal, ids_s[k:k + step], background, ids_b[k:k + step])
        parts.append(ov.store())
        shared += int(ov.shared().sum())
    mixed = parts[0]
    if len(parts) > 1:
        counts = np.concatenate([p.counts for p in parts])
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(mixed.device)
        mixed = utils.PXDEventStore._from_device(counts, offsets, torch.cat([p.pos for p in parts]), torch.cat([p.charge for p in parts]), shape, S)
    mixed.save(args.out)
    rec = dict(events=n, signal_digits=int(signal.counts[ids_s].sum()), background_digits=int(background.counts[ids_b].sum()),
               digits=int(mixed.counts.sum()), shared=shared)
    with open(args.out + ".json", "w") as fh:
        json.dump(rec, fh)
    print(json.dumps(rec))
    return rec


def main(argv=None):
    run(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
