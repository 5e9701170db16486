#!/usr/bin/env bash
# Round evidence for profiles/<round>/<workload>/: rocprofv3 kernel trace + stats, the two
# PMC passes (FETCH_SIZE, WRITE_SIZE) and the bench line (with its CPU baseline) of the
# same build.  usage: ROUND=r1 WORKLOADS="reuse restir mcpt" bash tools/round_evidence.sh
set -u
R="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
cd "$R"
ROUND=${ROUND:-r1}
for WL in ${WORKLOADS:-reuse restir mcpt}; do
  # (the profile's one-frame-in-flight region traces as the production frames do: one workgroup
  # per segment, the trace launch's only mode)
  TAG=${ROUND}_$WL BENCH_ARGS="--workload $WL" bash tools/profile.sh || { echo "profile $WL failed"; exit 1; }
  # the bench line's log: under $OUT (default build/evidence, which git ignores)
  LOG="${OUT:-build/evidence}/bench_${ROUND}_$WL.log"
  mkdir -p "$(dirname "$LOG")"
  timeout -k 10 400 python3 bench.py --full --workload "$WL" --steps 20 --warmup 3 > "$LOG" 2>&1 \
    || { echo "bench $WL failed"; exit 1; }
  echo "$WL: $(tail -n 1 "$LOG" | cut -c1-200)"
done
