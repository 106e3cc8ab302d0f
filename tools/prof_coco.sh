#!/bin/bash
# usage: tools/prof_coco.sh <tag> [batch] [steps] [warmup]   (run on the GPU box via gpurun; >= 30 steps: the host must be ahead of the GPU for the timeline to be the steady state)
root=$(cd "$(dirname "$0")/.." && pwd); out=${PROF_OUT:-$root/prof_out}; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$1 -- python3 $root/bench.py --full --workload coco --batch ${2:-128} --steps ${3:-6} --warmup ${4:-2} --no-cpu-baseline > $out/prof_$1.log 2>&1
python3 $root/tools/trace_step.py $out/prof_$1 > $out/prof_$1.txt
