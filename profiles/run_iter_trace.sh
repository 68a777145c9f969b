#!/bin/bash
# rocprofv3 kernel trace of one training iteration; the timeline is produced on the GPU box.
# Usage: [OUT=dir] bash profiles/run_iter_trace.sh <tag> [image|all|feature]      (writes under $OUT, default evidence_out/)
TAG=${1:-rX}
SCOPE=${2:-image}
R=$PWD
O=$(realpath -m "${OUT:-evidence_out}")
export TMPDIR=/tmp
mkdir -p $O/itrace_$TAG
cd /tmp
timeout 400 rocprofv3 --kernel-trace --stats -d $O/itrace_$TAG -o t -- python $R/profiles/iteration_breakdown.py $SCOPE > $O/itrace_${TAG}_bench.json 2> $O/itrace_$TAG/err.log
cd $R
python profiles/iteration_timeline.py $O/itrace_$TAG/t_results.db $O/itrace_${TAG}_timeline.md > /dev/null
python profiles/summarize_rocpd.py $O/itrace_$TAG/t_results.db $O/itrace_${TAG}_stats.md "rocprofv3 --kernel-trace --stats -- python profiles/iteration_breakdown.py $SCOPE" > /dev/null
rm -rf $O/itrace_$TAG
head -120 $O/itrace_${TAG}_timeline.md
