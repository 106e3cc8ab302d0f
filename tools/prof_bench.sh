#!/bin/bash
# usage: tools/prof_bench.sh <tag> <workload> [bench args]   (run on the GPU box via gpurun)
# rocprofv3 --kernel-trace --stats of the bench command -> $PROF_OUT/prof_<tag>/ + step timeline $PROF_OUT/prof_<tag>.txt (default prof_out/)
tag=$1; wl=$2; shift; shift
root=$(cd "$(dirname "$0")/.." && pwd); out=${PROF_OUT:-$root/prof_out}; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -- python3 $root/bench.py --full --workload $wl --no-cpu-baseline "$@" > $out/prof_$tag.log 2>&1
python3 $root/tools/trace_step.py $out/prof_$tag > $out/prof_$tag.txt
