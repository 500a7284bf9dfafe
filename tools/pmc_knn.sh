#!/bin/bash
# Counters of the lapping-knn launch (knn2_kernel / knn2_mfma_kernel), counters only -- no tracing in the same run:
# tools/match_once.py --frames 128 --reps 1 (its warm-up step + 1 = two 128-frame launches), two --pmc passes of
# 8 SQ counters each: instruction mix and wait shares, then the matrix-pipe and LDS counters.
# Usage: [OMV_LIB=other/libomv.so] [OMV_KNN=mfma|lanes] bash tools/pmc_knn.sh <tag> [output directory]
# (default build/pmc/<tag> in the repository; the summary goes to pmc_knn_<tag>.json there)
set -uo pipefail
TAG=${1:-knn}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${2:-$R/build/pmc/$TAG}
mkdir -p $OUT
OUT=$(cd $OUT && pwd)
cd "${TMPDIR:-/tmp}"   # the profiler writes its scratch files into the working directory
CTR1="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS"
CTR2="SQ_WAVES SQ_INSTS_MFMA SQ_INSTS_VALU_MFMA_I8 SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT"
timeout -s KILL 240 rocprofv3 --pmc $CTR1 -d $OUT/mix -o run --output-format csv -- \
    python3 $R/tools/match_once.py --frames 128 --reps 1 > $OUT/mix.txt 2> $OUT/mix.err || { echo "pass 1 failed"; tail -3 $OUT/mix.err; exit 1; }
timeout -s KILL 240 rocprofv3 --pmc $CTR2 -d $OUT/pipe -o run --output-format csv -- \
    python3 $R/tools/match_once.py --frames 128 --reps 1 > $OUT/pipe.txt 2> $OUT/pipe.err || { echo "pass 2 failed"; tail -3 $OUT/pipe.err; exit 1; }
python3 - $OUT $TAG <<'PY'
import csv, sys, collections, re, os, json
out, tag = sys.argv[1], sys.argv[2]
d = collections.defaultdict(lambda: collections.defaultdict(float))
for p in ("mix", "pipe"):
    for r in csv.DictReader(open(os.path.join(out, p, "run_counter_collection.csv"))):
        m = re.search(r"(knn2\w*_kernel)", r["Kernel_Name"])
        if not m:
            continue
        d[m.group(1)][p + "." + r["Counter_Name"]] += float(r["Counter_Value"])
res = {"tag": tag, "program": "tools/match_once.py --frames 128 --reps 1 (two 128-frame knn launches)", "kernels": {}}
for k, v in d.items():
    w, cyc = max(v["mix.SQ_WAVES"], 1), max(v["mix.SQ_WAVE_CYCLES"], 1)
    res["kernels"][k] = {
        "waves": v["mix.SQ_WAVES"], "valu_per_wave": round(v["mix.SQ_INSTS_VALU"] / w, 1),
        "lds_per_wave": round(v["mix.SQ_INSTS_LDS"] / w, 1),
        "mfma_per_wave": round(v["pipe.SQ_INSTS_MFMA"] / max(v["pipe.SQ_WAVES"], 1), 1),
        "mfma_i8_per_wave": round(v["pipe.SQ_INSTS_VALU_MFMA_I8"] / max(v["pipe.SQ_WAVES"], 1), 1),
        "active_share": round(v["mix.SQ_ACTIVE_INST_ANY"] / cyc, 3), "wait_any_share": round(v["mix.SQ_WAIT_ANY"] / cyc, 3),
        "wait_inst_share": round(v["mix.SQ_WAIT_INST_ANY"] / cyc, 3), "busy_cycles": v["mix.SQ_BUSY_CYCLES"],
        "raw": dict(sorted(v.items()))}
print(json.dumps(res, indent=1))
json.dump(res, open(os.path.join(out, f"pmc_knn_{tag}.json"), "w"), indent=1)
PY
