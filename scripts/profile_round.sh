#!/bin/bash
# The round's measurement evidence in one GPU session: scripts/profile_round.sh TAG   (writes $OUT_DIR/*_TAG*, default out/)
#   1. bench.py --full                                                  -> bench_TAG.json
#   2. rocprofv3 --kernel-trace --stats of the timed region only        -> kernel_stats_TAG.csv  (the dominant kernel's
#      (--no_secondary --no_strong: every launch of it is a 10 000-pair launch, so AverageNs IS roofline.avg_launch_ms)
#   3. HBM counters, separate --pmc passes, 10 000 and 1250 pairs       -> pmc_hbm_TAG_10000.json, pmc_hbm_TAG_1250.json
#   4. SQ instruction / wait counters, 10 000 pairs                     -> pmc_sq_TAG.json
#   5. the same for round 3's routing (PO_REG_NEVER=1: beam2d_kernel)   -> *_TAG_legacy*
#   6. the 1-D beam search (config 2): kernel stats + SQ counters       -> beam1d_TAG.txt
tag=${1:-rXX}
root=${GRAFT_REPO_ROOT:-/root/repo}
export OUT_DIR=${OUT_DIR:-$root/out}; out=$OUT_DIR   # (pmc_hbm.sh writes there too)
mkdir -p $out
cd $root
timeout 900 python bench.py --full > $out/bench_$tag.json 2> $out/bench_$tag.err
tail -1 $out/bench_$tag.json | cut -c1-300
cd /tmp && export TMPDIR=/tmp
prof_one() {   # $1 = suffix, env already set
  timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag$1 -- python3 $root/bench.py --steps 3 --warmup 1 --gen_procs 1 --cpu_sample 0 --no_secondary --no_strong > $out/prof_$tag$1.log 2>&1
  f=$(find $out/prof_$tag$1 -name "*kernel_stats.csv" | head -1)
  [ -n "$f" ] && cp $f $out/kernel_stats_$tag$1.csv && head -8 $f | cut -c1-160
  tail -1 $out/prof_$tag$1.log > $out/bench_under_rocprof_$tag$1.json
}
sq_one() {     # $1 = suffix
  timeout 900 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR --output-format csv -d $out/sq_$tag$1 -- python3 $root/bench.py --steps 1 --warmup 1 --gen_procs 1 --cpu_sample 0 --no_secondary --no_strong > $out/sq_$tag$1.log 2>&1
  python3 - <<PY
import csv, glob, collections, json
acc = collections.defaultdict(lambda: collections.defaultdict(float)); last = {}
rows = []
for f in glob.glob("$out/sq_$tag$1/**/*counter_collection.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
for r in rows:
    k = r["Kernel_Name"].split("(")[0].replace("void ", "")
    d = int(r["Dispatch_Id"])
    if k not in last or d > last[k]: last[k] = d
for r in rows:
    k = r["Kernel_Name"].split("(")[0].replace("void ", "")
    if int(r["Dispatch_Id"]) == last[k]: acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
out = {k: dict(v) for k, v in acc.items() if any(x in k for x in ("beam2d", "pair_prep", "viterbi"))}
json.dump({"command": "rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR -- python3 bench.py --steps 1 --warmup 1 --gen_procs 1 --cpu_sample 0 --no_secondary --no_strong",
           "note": "the LAST launch of every kernel (10 000 pairs per launch), counters summed over the device", "kernels": out}, open("$out/pmc_sq_$tag$1.json", "w"), indent=1)
for k, v in out.items():
    if "beam2d" in k: print(k, {a: "%.3e" % b for a, b in v.items()})
PY
}
prof_one ""
cd $root && scripts/pmc_hbm.sh ${tag}_10000 10000 > $out/pmc_hbm_${tag}_10000.txt 2>&1; tail -16 $out/pmc_hbm_${tag}_10000.txt
scripts/pmc_hbm.sh ${tag}_1250 1250 > $out/pmc_hbm_${tag}_1250.txt 2>&1
cd /tmp; sq_one ""
export PO_REG_NEVER=1
prof_one "_legacy"
cd /tmp; sq_one "_legacy"
unset PO_REG_NEVER
# 1-D beam search
cd /tmp
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/b1_$tag -- python3 $root/scripts/quick_time_1d.py 1000 > $out/beam1d_$tag.txt 2>&1
f=$(find $out/b1_$tag -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp $f $out/kernel_stats_beam1d_$tag.csv && grep beam1d $f | cut -c1-200
timeout 400 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS --output-format csv -d $out/b1sq_$tag -- python3 $root/scripts/quick_time_1d.py 1000 >> $out/beam1d_$tag.txt 2>&1
python3 - <<PY
import csv, glob, collections, json
acc = collections.defaultdict(lambda: collections.defaultdict(float)); n = collections.Counter()
for f in glob.glob("$out/b1sq_$tag/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].split("(")[0].replace("void ", "")
        acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
        if r["Counter_Name"] == "SQ_WAVE_CYCLES": n[k] += 1
out = {k: dict(v, launches=n[k]) for k, v in acc.items() if "beam1d" in k}
json.dump({"command": "rocprofv3 --pmc ... -- python3 scripts/quick_time_1d.py 1000", "note": "summed over the launches of the script (W = 10 twice, W = 25 twice)", "kernels": out}, open("$out/pmc_sq_beam1d_$tag.json", "w"), indent=1)
print(out)
PY
