#!/bin/bash
# bench.py plain, then under rocprofv3 --kernel-trace --stats (round-end evidence): scripts/bench_profile.sh TAG
tag=${1:-rXX}
root=${GRAFT_REPO_ROOT:-/root/repo}
out=${OUT_DIR:-$root/out}   # where the results go
mkdir -p $out
cd $root
timeout 900 python bench.py > $out/bench_$tag.json 2> $out/bench_$tag.err
tail -1 $out/bench_$tag.json | cut -c1-600
cd /tmp && export TMPDIR=/tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -- python3 $root/bench.py --full --steps 2 --warmup 1 --gen_procs 1 --cpu_sample 0 > $out/prof_$tag.log 2>&1
f=$(find $out/prof_$tag -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp $f $out/kernel_stats_$tag.csv && head -12 $f
tail -1 $out/prof_$tag.log | cut -c1-300
