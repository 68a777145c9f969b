#!/bin/bash
# rocprofv3 kernel trace of the bench command (`bench.py --full`: every window of the line); the summary table is produced
# on the GPU box because the sqlite output is too large to copy back.  Usage: [OUT=dir] bash profiles/run_trace.sh <tag> [bench args]
# Writes $OUT/trace_<tag>.md and $OUT/trace_<tag>_bench.json (default OUT: evidence_out/).
TAG=${1:-rX}; shift
R=$PWD
O=$(realpath -m "${OUT:-evidence_out}")
export TMPDIR=/tmp
mkdir -p $O/trace_$TAG
cd /tmp
timeout 400 rocprofv3 --kernel-trace --stats -d $O/trace_$TAG -o t -- python $R/bench.py --steps 10 --warmup 2 --no-cpu-baseline --full "$@" > $O/trace_${TAG}_bench.json 2> $O/trace_$TAG/err.log
cd $R
python profiles/summarize_rocpd.py $O/trace_$TAG/t_results.db $O/trace_${TAG}.md "rocprofv3 --kernel-trace --stats -- python bench.py --steps 10 --warmup 2 --no-cpu-baseline --full $*" > /dev/null
rm -rf $O/trace_$TAG
head -40 $O/trace_${TAG}.md; cat $O/trace_${TAG}_bench.json | cut -c1-300
