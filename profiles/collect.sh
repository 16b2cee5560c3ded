#!/usr/bin/env bash
# Collect the round's evidence on an MI355X, from the repo root:
#   bash profiles/collect.sh r02 <git head>          (output directory: $OUT_DIR, default profiles/out)
# 1. bench line (--full: configs[1] timed, then configs[3], configs[4], per-launch timing, CPU leg) -> <out>/<tag>_bench.json
# 2. rocprofv3 --kernel-trace --stats      -> <out>/<tag>_kernel_stats.csv   (plain bench command, graph replay)
# 3. rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in two separate passes (eager steps) -> <out>/<tag>_pmc_traffic.json
# Copy the three files into profiles/ afterwards (the output directory is scratch).
set -uo pipefail
TAG="${1:-r02}"; HEAD="${2:-unknown}"
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
OUT="${OUT_DIR:-profiles/out}"
mkdir -p "$OUT"
python bench.py --full --steps 10 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
rc=$?
echo "$rc" > $OUT/${TAG}_bench.rc          # the exit status is evidence too (normal interpreter teardown, no masking)
if [ "$rc" -ne 0 ]; then tail -c 3000 $OUT/${TAG}_bench.err; exit 1; fi
echo "bench done"
rm -rf $OUT/${TAG}_trace
rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_trace -o t --output-format csv -- python3 bench.py --steps 16 --no-cpu-baseline --no-configs3 --no-kernel-timing > $OUT/${TAG}_trace.log 2>&1
python - "$TAG" "$OUT" <<'PY'
import csv, glob, sys
tag, d = sys.argv[1], sys.argv[2]
f = glob.glob(f"{d}/{tag}_trace/**/*kernel_stats.csv", recursive=True)
rows = list(csv.DictReader(open(f[0])))
with open(f"{d}/{tag}_kernel_stats.csv", "w", newline="") as out:
    w = csv.writer(out)
    w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs"])
    for r in rows:
        w.writerow([r["Name"][:140], r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["Percentage"], r["MinNs"], r["MaxNs"]])
print("kernel stats:", len(rows), "kernels")
PY
echo "trace done"
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/${TAG}_pmc_$c
  rocprofv3 --pmc $c --kernel-trace -d $OUT/${TAG}_pmc_$c -o p --output-format csv -- python3 bench.py --steps 5 --warmup 1 --no-graph --no-cpu-baseline --no-configs3 --no-kernel-timing > $OUT/${TAG}_pmc_$c.log 2>&1
  echo "pmc $c done"
done
F=$(find $OUT/${TAG}_pmc_FETCH_SIZE -name '*counter_collection.csv' | head -1)
W=$(find $OUT/${TAG}_pmc_WRITE_SIZE -name '*counter_collection.csv' | head -1)
python profiles/pmc_traffic.py "$F" "$W" 6 $OUT/${TAG}_pmc_traffic.json "$HEAD"
rm -rf $OUT/${TAG}_trace $OUT/${TAG}_pmc_FETCH_SIZE $OUT/${TAG}_pmc_WRITE_SIZE
