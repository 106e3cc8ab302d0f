#!/bin/bash
root=$(cd "$(dirname "$0")/.." && pwd); out=${PROF_OUT:-$root/prof_out}; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
export MMVAE_SERIAL=1
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$1 -- python3 $root/bench.py --full --steps 20 --warmup 3 --no-cpu-baseline > $out/prof_$1.log 2>&1
python3 $root/tools/trace_step.py $out/prof_$1 > $out/prof_$1.txt
