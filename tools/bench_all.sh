#!/bin/bash
# Run `bench.py --full` on every workload; each run under its own time limit, stopping at the
# first failure.  Output: $OUT/bench_<workload>.log (OUT defaults to bench_out)
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for w in ${@:-cfg3 cfg2 cfg4 cfg5}; do
    echo "=== $w"
    timeout -k 10 400 python bench.py --full --workload $w > "$OUT/bench_$w.log" 2>&1
    rc=$?
    tail -c 2500 "$OUT/bench_$w.log"
    [ $rc -ne 0 ] && { echo "stopping after $w (rc=$rc)"; exit $rc; }
done
exit 0
