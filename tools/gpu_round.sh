#!/bin/bash
# One GPU call: GPU tests, the whole bench (--full), then the rocprof kernel-trace + PMC profile.
# Usage (on the box, from the repo root): bash tools/gpu_round.sh <tag> [skip-tests]
set -euo pipefail
TAG=${1:-r02}
R=$GRAFT_REPO_ROOT
mkdir -p $R/gpurun_out
cd $R
if [ "${2:-}" != "skip-tests" ]; then
  timeout -k 10 400 python -u -m pytest tests -x -v -m gpu --timeout 120 --timeout-method thread \
      > gpurun_out/gputests_$TAG.log 2>&1
  tail -3 gpurun_out/gputests_$TAG.log
fi
BOUT=${OMV_BENCH_OUT:-scratch}   # where the bench's result line goes
mkdir -p $BOUT
timeout -k 10 500 python -u bench.py --full > $BOUT/bench_$TAG.json 2> $BOUT/bench_$TAG.err
tail -c 600 $BOUT/bench_$TAG.json
bash tools/profile_gpu.sh $TAG
bash tools/pmc_orb_bound.sh bound_$TAG
