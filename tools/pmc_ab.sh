#!/bin/bash
# Runs ON THE GPU BOX: per env-wave instruction and cycle counters of the per-step kernel for one tree, two rocprofv3
# --pmc passes of their own (no tracing in the same run) over the bench workload, summarised as JSON.
# usage: tools/pmc_ab.sh <tag> [<tree>]   (<tree>: a built checkout, default this one) -> $PMC_OUT/<tag>/pmc_summary.json
# (PMC_OUT: where the passes and the summary go, default pmc_out/ in the directory the script is called from)
set -u
TAG=$1
R=$(pwd)
TREE=${2:-$R}
OUT=${PMC_OUT:-$R/pmc_out}/$TAG
mkdir -p $OUT
export TMPDIR=/tmp
ARGS="--gpus 1 --steps 512 --warmup 64 --repeats 2 --no-cpu-baseline --no-rollout"
cd $TREE
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_WR SQ_INSTS_VMEM_RD SQ_WAVES SQ_INSTS_SMEM SQ_INSTS_BRANCH \
  --output-format csv -d $OUT/pmc_insts -- python3 bench.py $ARGS > $OUT/pmc_insts.log 2>&1 || { echo "insts pass failed"; tail -5 $OUT/pmc_insts.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_VALU \
  --output-format csv -d $OUT/pmc_cycles -- python3 bench.py $ARGS > $OUT/pmc_cycles.log 2>&1 || { echo "cycles pass failed"; tail -5 $OUT/pmc_cycles.log; exit 1; }
python3 - <<PY
import collections, csv, glob, json, re, statistics
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for d in ("pmc_insts", "pmc_cycles"):
    for f in glob.glob("$OUT/%s/**/*counter_collection.csv" % d, recursive=True):
        for r in csv.DictReader(open(f)):
            # the per-step kernels: generic, compiled shape, and its plain-call variant (a sixth template argument)
            if re.search(r"msnake_step_kernel<\d, \d, 0, 1(, \d+){0,2}>", r["Kernel_Name"]):
                acc[r["Kernel_Name"]][r["Counter_Name"]].append(float(r["Counter_Value"]))
out = {}
for k, c in acc.items():
    w = statistics.median(c["SQ_WAVES"])
    out[k] = {"launches": len(c["SQ_WAVES"]), "waves_per_launch": w}
    out[k].update({n + "_per_wave": round(statistics.median(v) / w, 2) for n, v in sorted(c.items()) if n != "SQ_WAVES"})
json.dump(out, open("$OUT/pmc_summary.json", "w"), indent=1)
print(json.dumps(out, indent=1))
PY
