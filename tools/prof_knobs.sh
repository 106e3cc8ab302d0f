#!/bin/bash
# usage: tools/prof_knobs.sh <tag> [--knob name=value ...]   (run on the GPU box via gpurun): kernel trace of bench.py under library knobs
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd); out=${PROF_OUT:-$root/prof_out}; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -- python3 $root/bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-probe "$@" > $out/prof_$tag.log 2>&1
python3 $root/tools/trace_step.py $out/prof_$tag > $out/prof_$tag.txt
