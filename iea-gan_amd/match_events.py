#!/usr/bin/env python3
"""What a background does to the signal's hits, hit by hit: digit files in, match statistics out.

    match_events.py --signal S.npz --background B.npz [--compare B2.npz] [--events N] [--seed K] [--threshold T]
                    [--seed_cut S --cluster_cut C --head_tail T --uniform_pitch U V --residual_bin W] [--batch 8] [--out R.npz]
                    [--shape H W] [--n_sensors S]

The inputs are digit files in the ``produce.py`` / ``pack_events.py`` / ``utils.write_digits`` format.  Output event ``k`` pairs signal event
``k % len(signal)`` with background event ``perm[k % len(background)]`` (``overlay_events.pairs``: ``perm`` is the identity, or the
permutation drawn from ``--seed``).  Per batch of ``--batch`` events, all on the device: the background is laid over the signal
(``PXDEventStore.overlay``), both the signal and the mixed events are expanded (``dense``) and reconstructed with the same threshold, cuts,
``--head_tail`` and geometry (``utils.pxd_hits``; the nominal ``PXDGeometry.belle2`` for 40 sensors of 250 x 768 cells, else
``--uniform_pitch U V`` in um), and every signal hit is matched to the mixed hits (``utils.PXDMatchStatistics.update``).  One read-back at
the end.

Prints one JSON line: ``events``, the pooled ``hits`` / ``matched`` / ``changed`` / ``shared`` / ``lost``, the pooled ``efficiency``,
``changed_fraction`` and ``shared_fraction``, the sums of the three histograms, ``residual_bin`` and ``unit_mm``; with ``--compare`` the
same under ``compare`` for the second background laid over the same signal events, and ``distance`` (``utils.pxd_match_distance`` of the
two).  ``--out`` gets every table (``compare_*`` for the second background) and ``R.npz.json`` the record.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from overlay_events import pairs          # noqa: E402

TABLES = ("hits", "matched", "changed", "shared", "lost", "efficiency", "changed_fraction", "shared_fraction", "residual_u", "residual_v",
          "purity", "hits_per_image")


def geometry_of(utils, shape, n_sensors, uniform_pitch=None):
    """``PXDGeometry.belle2`` for 40 sensors of 250 x 768 cells, else ``uniform`` with the cell size ``uniform_pitch = (u, v)`` in um."""
    if uniform_pitch is not None:
        units = [2.0 * float(p) for p in uniform_pitch]         # the geometry unit is 0.5 um
        if any(p != int(p) for p in units):
            raise SystemExit(f"--uniform_pitch {uniform_pitch}: a pitch must be a multiple of 0.5 um")
        try:
            return utils.PXDGeometry.uniform(shape, int(units[0]), int(units[1]), n_sensors)
        except ValueError as e:
            raise SystemExit(f"--uniform_pitch {uniform_pitch}: {e}")
    if tuple(shape) != (250, 768) or n_sensors != 40:
        raise SystemExit(f"the nominal PXD geometry is known for 40 sensors of 250 x 768 cells, not {n_sensors} of {shape[0]} x {shape[1]}: "
                         "give the cell size with --uniform_pitch U V (um)")
    return utils.PXDGeometry.belle2()


def match_stores(utils, signal, background, ids_s, ids_b, geometry, head_tail=3, threshold=7.0, seed_cut=0, charge_cut=0, residual_bin=10,
                 batch=8):
    """``PXDMatchStatistics.result()`` over the pairs ``(ids_s[k], ids_b[k])`` of two ``PXDEventStore``s, ``batch`` events a step.  The
    capacity of a reconstruction is the digits its events hold in their store, a bound the host knows: no step can overflow."""
    acc = utils.PXDMatchStatistics(signal.n_sensors, residual_bin, signal.device)
    hits = lambda store, ids: utils.pxd_hits(store.dense(ids), geometry, head_tail, threshold, seed_cut, charge_cut,
                                             max(int(store.counts[np.asarray(ids)].sum()), 1), store.n_sensors)
    for k in range(0, len(ids_s), batch):
        s, b = ids_s[k:k + batch], ids_b[k:k + batch]
        mixed = signal.overlay(s, background, b)
        acc.update(hits(signal, s), hits(mixed, np.arange(len(s))))
    return acc.result()


def record(result):
    """The JSON record of one ``result()``."""
    pooled = {k: int(result[k].sum()) for k in ("hits", "matched", "changed", "shared", "lost")}
    ratio = lambda a, b: pooled[a] / pooled[b] if pooled[b] else float("nan")
    return dict(events=int(result["n_events"]), **pooled, efficiency=ratio("matched", "hits"), changed_fraction=ratio("changed", "matched"),
                shared_fraction=ratio("shared", "matched"), residual_u_sum=int(result["residual_u"].sum()),
                residual_v_sum=int(result["residual_v"].sum()), purity_sum=int(result["purity"].sum()), residual_bin=int(result["residual_bin"]),
                unit_mm=float(result["unit_mm"]))


def run(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--signal", required=True, help="digit file of the signal events (.npz)")
    ap.add_argument("--background", required=True, help="digit file of the background events (.npz)")
    ap.add_argument("--compare", default=None, help="digit file of a second background, laid over the same signal events")
    ap.add_argument("--events", type=int, default=0, help="number of output events (0: one per signal event)")
    ap.add_argument("--seed", type=int, default=None, help="seed of the permutation of the background events (default: identity)")
    ap.add_argument("--threshold", type=float, default=7.0, help="digit threshold in ADU")
    ap.add_argument("--seed_cut", type=int, default=0, help="seed cut in ADU")
    ap.add_argument("--cluster_cut", type=int, default=0, help="cluster-charge cut in ADU")
    ap.add_argument("--head_tail", type=int, default=3, help="head-tail from this many cells on (0: never)")
    ap.add_argument("--uniform_pitch", type=float, nargs=2, default=None, metavar=("U", "V"), help="cell size in um instead of the nominal geometry")
    ap.add_argument("--residual_bin", type=int, default=10, help="width of a residual bin in geometry units (10 = 5 um)")
    ap.add_argument("--batch", type=int, default=8, help="events per step")
    ap.add_argument("--out", default=None, help="the tables (.npz); the record goes to OUT.json")
    ap.add_argument("--shape", type=int, nargs=2, default=(250, 768), metavar=("H", "W"))
    ap.add_argument("--n_sensors", type=int, default=40)
    args = ap.parse_args(argv)
    if args.seed_cut < 0 or args.cluster_cut < 0 or (args.head_tail != 0 and args.head_tail < 3) or args.residual_bin < 1 or args.batch < 1:
        raise SystemExit("--seed_cut and --cluster_cut must not be negative, --head_tail is 0 or at least 3, --residual_bin and --batch at least 1")
    import utils
    utils.H.require_gpu()
    shape, S = tuple(args.shape), args.n_sensors
    if args.batch * S > 65535:
        raise SystemExit(f"--batch {args.batch}: one step takes at most {65535 // S} events of {S} sensors")
    geometry = geometry_of(utils, shape, S, args.uniform_pitch)
    signal = utils.PXDEventStore.from_file(args.signal, shape, S)
    if not len(signal):
        raise SystemExit("match_events: a file without events")
    n = args.events if args.events > 0 else len(signal)
    rec, tables, results = {}, {}, []
    for name, path in (("", args.background), ("compare", args.compare)):
        if path is None:
            continue
        background = utils.PXDEventStore.from_file(path, shape, S)
        if not len(background):
            raise SystemExit("match_events: a file without events")
        ids_s, ids_b = pairs(len(signal), len(background), n, args.seed)
        res = match_stores(utils, signal, background, ids_s, ids_b, geometry, args.head_tail, args.threshold, args.seed_cut, args.cluster_cut,
                           args.residual_bin, args.batch)
        results.append(res)
        if name:
            rec[name] = record(res)
        else:
            rec.update(record(res))
        tables.update((f"{name}_{k}" if name else k, np.asarray(res[k])) for k in TABLES)
    if len(results) == 2:
        rec["distance"] = utils.pxd_match_distance(*results)
    if args.out:
        with open(args.out, "wb") as fh:
            np.savez(fh, residual_bin=np.int64(args.residual_bin), unit_mm=np.float64(geometry.unit_mm), **tables)
        with open(args.out + ".json", "w") as fh:
            json.dump(rec, fh)
    print(json.dumps(rec))
    return rec


def main(argv=None):
    run(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
