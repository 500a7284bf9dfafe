#!/bin/bash
# SearchByProjection candidate stage on the GPU box: matcher parity tests, then per-stage times of one 128-frame
# stream group for the global-memory kernel and the LDS-staged one over chunk sizes (OMV_CAND_PW) x window splits
# (OMV_CAND_SPLIT; a huge value is one lane per window):
#   bash tools/cand_sweep.sh "64 128 256" "8 16 32 1000000000"      (the second list defaults to the built-in split)
set -euo pipefail
R=$GRAFT_REPO_ROOT
cd $R
mkdir -p gpurun_out
PWS=${1:-128}
SPLITS=${2:-default}
timeout -k 10 240 python -u -m pytest tests/test_match_gpu.py tests/test_p1080_gpu.py -x -q --timeout 120 --timeout-method thread > gpurun_out/cs_tests.log 2>&1 || { tail -30 gpurun_out/cs_tests.log; exit 1; }
tail -1 gpurun_out/cs_tests.log
timeout -k 10 240 python -u -m pytest tests/test_cand_balance_gpu.py -x -q --timeout 120 --timeout-method thread 2>&1 | tail -30
echo "== global"
OMV_CAND=global timeout -k 10 120 python tools/match_once.py --frames 128 --reps 3 --timing 2>&1 | grep frames
for PW in $PWS; do
  for SP in $SPLITS; do
    echo "== lds pw $PW split $SP"
    if [ "$SP" = default ]; then unset OMV_CAND_SPLIT; else export OMV_CAND_SPLIT=$SP; fi
    OMV_CAND_PW=$PW timeout -k 10 120 python tools/match_once.py --frames 128 --reps 3 --timing 2>&1 | grep frames
  done
done
