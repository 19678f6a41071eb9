#!/bin/bash
# the benchmark with everything it measures (--full), the complete objects kept beside the compact line.
# usage: bash tools/bench_full.sh [output directory, default bench_out]
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd "$(dirname "$0")/.."
OUT=${1:-bench_out}
mkdir -p "$OUT"
( time python bench.py --full --full-out "$OUT/bench_full.json" ) > "$OUT/bench_stdout.log" 2> "$OUT/bench_stderr.log"
grep '^{"metric' "$OUT/bench_stdout.log" | tail -1 > "$OUT/bench_line.json"
cat "$OUT/bench_line.json"
tail -4 "$OUT/bench_stderr.log"
