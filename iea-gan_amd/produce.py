#!/usr/bin/env python3
"""Event production: the reference's ``Physics_Analysis/create_g1.py`` up to the digits, without basf2.

    produce.py --weights RUN/weights --events N --out FILE.npz [--events_per_batch E] [--use_ema] [--weight_name S] [--seed S]
               [--threshold T] [--synthetic-weights] [--hits FILE [--seed_cut S --cluster_cut C --head_tail T --uniform_pitch U V --space_points]]

Loads the checkpoint under ``--weights`` the way ``validate.py`` does (the ``weights`` directory of a run; ``--use_ema`` takes
``G_ema.pth``; ``--synthetic-weights`` takes a freshly initialised generator instead, for tests and measurements) and generates ``N``
events of ``n_classes`` sensors: eval mode when ``G_eval_mode``, latents and ``rdof`` from a ``torch.Generator`` of its own seeded with
``--seed`` (per batch of ``E`` events first ``z [E*40, dim_z]``, then ``rdof [E*40, rdof_dim]``), ``y = arange(40).repeat(E)``, through the
export epilogue.  Every batch is compacted on the device (``utils.pxd_digits``: digit iff the truncated uint8 charge is positive and
the value >= ``--threshold``; 0 is the reference's production behaviour, create_g1.py:73-79) and only the header (digits per image)
and the digits are copied, into pinned host buffers: no dense image crosses PCIe.  The loop is double-buffered -- batch k+1 is
enqueued before the host waits for batch k, one wait per batch.  The number of digits copied per batch follows the batch before it
(x 1.5 + 64; the first copies the whole capacity); a batch that exceeds it costs one more copy, one that exceeds the device buffers a
rerun, never a truncation.

``--out`` (``.npz``, see ``utils.write_digits``): ``event_offsets`` int64 ``[N + 1]``, ``sensor`` uint8, ``ucell`` uint8 (row), ``vcell``
uint16 (column), ``charge`` uint8, digits in ``nonzero()`` order inside an event; ``utils.read_digits`` yields the events in the format
``create_g1.generate`` puts on its queue.  ``<out>.json`` carries the checkpoint's sha256 and the arguments (create_g1.py:173-189).
Writing the digits into a basf2 ``RootOutput`` file (create_g1.py:91-122) needs basf2 and ROOT and is out of scope: a ``DigitCreator``
module fed from ``utils.read_digits`` is the bridge.

``--hits FILE`` also reconstructs every batch on the device, on the digits it already has (they are not computed twice): clusters, the cuts
``--seed_cut`` / ``--cluster_cut`` (ADU), positions and ``utils.pxd_hits`` with ``--head_tail`` in the nominal geometry
``utils.PXDGeometry.belle2`` (design values, not checked against basf2; it exists for 40 sensors of 250 x 768 cells only, any other
configured geometry needs ``--uniform_pitch U V``, the cell size in um).  The hits of a batch are one more read-back; ``FILE`` is the hit
file of ``utils.write_hits`` (local positions in mm from the sensor centre) and the record gains ``hits`` and ``hit_waits``.  With
``--space_points`` a second file ``FILE.points.npz`` holds ``x_mm`` / ``y_mm`` / ``z_mm`` float32 per hit in the global frame of
``utils.PXDPlacement.belle2`` (two barrels at the nominal radii with ``--uniform_pitch``), in the hit file's order and with its
``event_offsets`` (``utils.pxd_space_points``; the hit file itself is unchanged).  Position errors and a basf2 writer are out of scope.  One JSON line with the rates is printed at the end.  The network geometry is
given like in ``train.py``: ``--config config.json`` and / or ``--key value``.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model          # noqa: E402
import train          # noqa: E402
import utils          # noqa: E402


def load_generator(cfg, weights, use_ema=False, weight_name=None, synthetic=False, seed=0):
    """(generator on ``cfg['device']``, sha256 of the checkpoint file or None)."""
    dev = torch.device(cfg["device"])
    if synthetic:
        torch.manual_seed(seed)
        return model.Generator(**dict(cfg, no_optim=True)).to(dev), None
    wdir = os.path.abspath(weights)
    if os.path.basename(wdir) != "weights":
        raise SystemExit(f"--weights expects the 'weights' directory of a run, got {wdir}")
    run_dir = os.path.dirname(wdir)
    lcfg = dict(cfg, outputroot=os.path.dirname(run_dir), run_name=os.path.basename(run_dir))
    G = model.Generator(**dict(cfg, skip_init=True, no_optim=True)).to(dev)
    utils.load_weights(None if use_ema else G, None, {}, lcfg, weight_name, G if use_ema else None, load_optim=False)
    name = utils.join_strings("_", ["G_ema" if use_ema else "G", weight_name]) + ".pth"
    with open(os.path.join(wdir, name), "rb") as fh:
        return G, hashlib.sha256(fh.read()).hexdigest()


def event_batches(G, cfg, n_events, per_batch, seed):
    """Yields the dense export ``[e * n_classes, H - 6, W]`` (fp32, on the device) of consecutive batches of ``e <= per_batch`` events."""
    dev = next(G.parameters()).device
    n = int(cfg["n_classes"])
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    was_training = G.training
    if cfg["G_eval_mode"]:
        G.eval()
    try:
        for first in range(0, n_events, per_batch):
            e = min(per_batch, n_events - first)
            z = torch.randn(e * n, G.dim_z, generator=gen, device=dev)
            rdof = torch.randn(e * n, G.rdof_dim, generator=gen, device=dev)
            y = torch.arange(n, dtype=torch.long, device=dev).repeat(e)
            with torch.no_grad():
                x = G(z, y, rdof=rdof, export=True)
            yield x
    finally:
        G.train(was_training)


def hit_geometry(cfg, uniform_pitch=None):
    """The ``PXDGeometry`` of ``--hits`` for the configured sensors: ``belle2`` for 40 sensors of 250 x 768 cells, else ``uniform`` with the
    cell size ``uniform_pitch = (u, v)`` in um; ``SystemExit`` when neither applies."""
    n, shape = int(cfg["n_classes"]), (cfg["resolution"] - 6, cfg["resolution"] * cfg["H_base"])
    if uniform_pitch is not None:
        units = [2.0 * float(p) for p in uniform_pitch]         # the geometry unit is 0.5 um
        if any(p != int(p) for p in units):
            raise SystemExit(f"--uniform_pitch {uniform_pitch}: a pitch must be a multiple of 0.5 um")
        try:
            return utils.PXDGeometry.uniform(shape, int(units[0]), int(units[1]), n)
        except ValueError as e:
            raise SystemExit(f"--uniform_pitch {uniform_pitch}: {e}")
    if shape != (250, 768) or n != 40:
        raise SystemExit(f"--hits: the nominal PXD geometry is known for 40 sensors of 250 x 768 cells, not {n} of {shape[0]} x {shape[1]}: "
                         "give the cell size with --uniform_pitch U V (um)")
    return utils.PXDGeometry.belle2()


def hit_placement(geometry, uniform_pitch=None):
    """The ``PXDPlacement`` that goes with ``hit_geometry``: ``belle2`` for the nominal geometry; with ``--uniform_pitch`` two barrels at the
    nominal radii of 14 and 22 mm, two sensors a ladder (one when the number of sensors is odd) and two ladders in five on the inner one, as
    in the PXD; ``SystemExit`` when the sensors do not fill two barrels."""
    if uniform_pitch is None:
        return utils.PXDPlacement.belle2(geometry)
    per = 2 if geometry.S % 2 == 0 else 1
    ladders = geometry.S // per
    inner = max(1, 2 * ladders // 5)
    if ladders < 2:
        raise SystemExit(f"a placement needs an inner and an outer ladder, {geometry.S} sensor(s) do not make two")
    try:
        return utils.PXDPlacement.barrel(geometry, (14.0, 22.0), (inner, ladders - inner), per)
    except ValueError as e:
        raise SystemExit(f"--uniform_pitch {uniform_pitch}: {e}")


def produce(G, cfg, n_events, per_batch, seed, threshold=0.0, hits=None):
    """Columns of the event file and a small record: ``(event_offsets, sensor, ucell, vcell, charge, rec)``.  With ``hits =
    dict(geometry=, seed_cut=, charge_cut=, head_tail=)`` every batch is also reconstructed (clusters -> positions -> ``utils.pxd_hits`` on
    the batch's own digits) and a seventh element follows: the arguments of ``utils.write_hits`` as a dict.  With ``hits["placement"]`` (a
    ``PXDPlacement``) the hits are also placed in the global frame (``utils.pxd_space_points``) and an eighth element follows: ``x_mm``,
    ``y_mm``, ``z_mm`` float32 per hit, in the order of the hit columns."""
    n = int(cfg["n_classes"])
    h, w = cfg["resolution"] - 6, cfg["resolution"] * cfg["H_base"]
    capacity = max(1024, per_batch * n * h * w // utils.PXD_DIGITS_FRACTION)
    pinned = [(torch.empty(per_batch * n + 1, dtype=torch.int32, pin_memory=True), torch.empty(capacity, dtype=torch.int32, pin_memory=True),
               torch.empty(capacity, dtype=torch.uint8, pin_memory=True)) for _ in range(2)]
    found, per_event, stats = [], [], dict(waits=0, extra_copies=0, bytes_copied=0, last=0)
    found_hits, hits_per_event, found_points = [], [], []
    placement = None if hits is None else hits.get("placement")

    def finish(d, hit, points):
        index, charge, counts = d.cpu()         # copies out of the pinned buffers, which the batch after next reuses
        stats["waits"] += 1
        stats["extra_copies"] += int(index.size > d.copied)
        stats["bytes_copied"] += 4 * (d.shape[0] + 1) + 5 * max(d.copied, index.size)
        stats["last"] = index.size
        found.append((index, charge))
        per_event.append(counts.reshape(-1, n).sum(1))
        if hit is not None:
            host = hit.cpu()                    # the hits of the batch: one more read-back
            found_hits.append(host)
            hits_per_event.append(host["counts"].reshape(-1, n).sum(1))
        if points is not None:
            found_points.append(points.cpu())   # and their space points: one more

    pending = None
    for k, x in enumerate(event_batches(G, cfg, n_events, per_batch, seed)):
        expect = capacity if not stats["last"] else min(capacity, stats["last"] + stats["last"] // 2 + 64)
        d = utils.pxd_digits(x, threshold=threshold, capacity=capacity, n_sensors=n).start_copy(expect, pinned[k % 2])
        hit = points = None
        if hits is not None:                    # enqueued behind the digit copies: the wait for the digits does not wait for the hits
            p = utils.pxd_cluster_positions(utils.pxd_clusters(d), seed_cut=hits["seed_cut"], charge_cut=hits["charge_cut"])
            hit = utils.pxd_hits(p, hits["geometry"], hits["head_tail"])
            points = utils.pxd_space_points(hit, placement) if placement is not None else None
        if pending is not None:
            finish(*pending)            # batch k is already enqueued while the host waits for batch k - 1
        pending = (d, hit, points)
    finish(*pending)
    offsets = np.concatenate([[0], np.cumsum(np.concatenate(per_event))]).astype(np.int64)
    # one split of every position at the end: sensor, row and column do not depend on the batch an image came in
    _, sensor, ucell, vcell, charge = utils.unpack_digits(np.concatenate([f[0] for f in found]), np.concatenate([f[1] for f in found]),
                                                          (per_batch * n, h, w), n)
    rec = dict(events=n_events, digits=int(offsets[-1]), host_waits=stats["waits"], extra_copies=stats["extra_copies"],
               bytes_copied_per_event=stats["bytes_copied"] / n_events,
               dense_bytes_per_event=4 * n * h * w)
    if hits is None:
        return offsets, sensor, ucell, vcell, charge, rec
    columns = {k: np.concatenate([f[k] for f in found_hits]) for k in list(utils.HIT_COLUMNS)[1:]}
    columns.update(event_offsets=np.concatenate([[0], np.cumsum(np.concatenate(hits_per_event))]).astype(np.int64),
                   unit_mm=hits["geometry"].unit_mm)
    rec.update(hits=int(columns["event_offsets"][-1]), hit_waits=len(found_hits))
    if placement is None:
        return offsets, sensor, ucell, vcell, charge, rec, columns
    points = {k: np.concatenate([f[k] for f in found_points]).astype(np.float32) for k in ("x_mm", "y_mm", "z_mm")}
    return offsets, sensor, ucell, vcell, charge, rec, columns, points


def run(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--weights", default=None, help="the weights directory of a run (<outputroot>/<run_name>/weights)")
    ap.add_argument("--synthetic-weights", action="store_true", help="a freshly initialised generator instead of a checkpoint")
    ap.add_argument("--events", type=int, required=True)
    ap.add_argument("--out", required=True, help="the event file (.npz); <out>.json is written next to it")
    ap.add_argument("--events_per_batch", type=int, default=1)
    ap.add_argument("--use_ema", action="store_true", help="produce with G_ema.pth instead of G.pth")
    ap.add_argument("--weight_name", default=None, help="checkpoint suffix (e.g. copy1000)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threshold", type=float, default=0.0, help="digit cut in ADU (0: every nonzero uint8 charge, 7: the evaluation cut)")
    ap.add_argument("--hits", default=None, help="also reconstruct the events and write this hit file (.npz, utils.write_hits)")
    ap.add_argument("--seed_cut", type=int, default=0, help="--hits: seed cut in ADU")
    ap.add_argument("--cluster_cut", type=int, default=0, help="--hits: cluster-charge cut in ADU")
    ap.add_argument("--head_tail", type=int, default=3, help="--hits: head-tail from this many cells on (0: never)")
    ap.add_argument("--uniform_pitch", type=float, nargs=2, default=None, metavar=("U", "V"),
                    help="--hits: one cell size in um instead of the nominal PXD geometry")
    ap.add_argument("--space_points", action="store_true",
                    help="--hits: also write <hits>.points.npz, the hits in the global frame of the nominal placement (x_mm, y_mm, z_mm)")
    args, rest = ap.parse_known_args(argv)
    cfg = train.parse(rest)
    if (args.weights is None) == (not args.synthetic_weights):
        raise SystemExit("give exactly one of --weights DIR and --synthetic-weights")
    if args.events <= 0 or args.events_per_batch <= 0:
        raise SystemExit("--events and --events_per_batch must be positive")
    hits = None
    if args.space_points and args.hits is None:
        raise SystemExit("--space_points needs --hits FILE")
    if args.hits is not None:
        if args.seed_cut < 0 or args.cluster_cut < 0 or (args.head_tail != 0 and args.head_tail < 3):
            raise SystemExit("--seed_cut and --cluster_cut must not be negative, --head_tail is 0 or at least 3")
        hits = dict(geometry=hit_geometry(cfg, args.uniform_pitch), seed_cut=args.seed_cut, charge_cut=args.cluster_cut, head_tail=args.head_tail)
        if args.space_points:
            hits["placement"] = hit_placement(hits["geometry"], args.uniform_pitch)
    utils.H.require_gpu()
    G, digest = load_generator(cfg, args.weights, args.use_ema, args.weight_name, args.synthetic_weights, args.seed)
    with open(args.out + ".json", "w") as fh:
        side = {k: v for k, v in vars(args).items() if hits is not None or k not in ("hits", "seed_cut", "cluster_cut", "head_tail", "uniform_pitch")}
        if not args.space_points:
            del side["space_points"]
        json.dump({"sha256(checkpoint)": digest, **side}, fh, indent=4, sort_keys=True)
    t0 = time.perf_counter()
    offsets, sensor, ucell, vcell, charge, rec, *hit_columns = produce(G, cfg, args.events, args.events_per_batch, args.seed, args.threshold, hits)
    rec["seconds"] = time.perf_counter() - t0
    rec["events_per_s"] = args.events / rec["seconds"]
    utils.write_digits(args.out, offsets, sensor, ucell, vcell, charge)
    if hits is not None:
        try:
            utils.write_hits(args.hits, **hit_columns[0])
        except ValueError as e:                 # e.g. a cluster of more than 65535 digits: no detector event, the digit file stands
            raise SystemExit(f"--hits: {e}; {args.out} is written, {args.hits} is not")
        if args.space_points:                   # the hit file's order and its event_offsets
            with open(args.hits + ".points.npz", "wb") as fh:
                np.savez(fh, event_offsets=hit_columns[0]["event_offsets"], unit_mm=np.float64(hits["geometry"].unit_mm), **hit_columns[1])
    print(json.dumps(rec))
    return rec


def main(argv=None):
    run(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    main()
