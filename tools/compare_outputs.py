#!/usr/bin/env python3
"""Pairwise distances between the arrays of several ``bench.py --dump-outputs DIR`` runs: is a build's train step the parent's?

    python tools/compare_outputs.py DIR_A DIR_B [DIR_C ...] [--out FILE]

For every ``*_state.npy`` the matrix of ``|a - b|_2 / |a|_2`` (float64) over the runs, and the losses of every run.  The train step is
not bit-identical run to run (float atomics of the weight gradients, the side stream), so two builds compute the same
thing when the distances between their runs lie inside the distances between the runs of one of them: run each build several times,
alternately, in one session.
"""
import argparse
import json
import os

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("runs", nargs="+", help="directories written by bench.py --dump-outputs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = [os.path.basename(os.path.normpath(r)) for r in args.runs]
    rec = dict(runs=names, rel_l2={}, losses={})
    for f in sorted(os.listdir(args.runs[0])):
        arrays = [np.load(os.path.join(r, f)).astype(np.float64) for r in args.runs]
        if f.startswith("loss_"):
            rec["losses"][f[5:-4]] = [float(a[0]) for a in arrays]
        else:
            rec["rel_l2"][f[:-4]] = [[float(np.sqrt(((a - b) ** 2).sum() / max((a ** 2).sum(), 1e-300))) for b in arrays] for a in arrays]
    for k, m in rec["rel_l2"].items():
        print(k)
        for n, row in zip(names, m):
            print(f"{n:>10s}", " ".join(f"{v:.2e}" for v in row))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
