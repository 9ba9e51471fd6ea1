#!/bin/bash
# rocprofv3 kernel trace of one bench sample (30 network evaluations); rocpd DB -> <out>/prof_<tag>/, where <out> is
# $PROF_OUT (an absolute path) or prof_out/ in this repository
# NOTE: always under `timeout`: the profiled python process has been seen to hang at exit after the
# tool finalised its output.
tag=${1:-r01}
R=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
out=${PROF_OUT:-$R/prof_out}/prof_$tag
rm -rf $out; mkdir -p $out
timeout -s KILL 240 rocprofv3 --kernel-trace --stats -d $out -o bench -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --graph ${GRAPH:-0} > $out/bench.log 2>&1
grep -o '"value": [0-9.]*' $out/bench.log | head -1
ls $out
