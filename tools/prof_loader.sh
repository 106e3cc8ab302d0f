#!/bin/bash
# usage: tools/prof_loader.sh <tag>   (run on the GPU box via gpurun): kernel + memory-copy trace of the loader-fed MultiMNIST loop
tag=$1
root=$(cd "$(dirname "$0")/.." && pwd); out=${PROF_OUT:-$root/prof_out}; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $out/prof_$tag -- python3 $root/bench.py --full --loader --steps 40 --warmup 10 --no-cpu-baseline --no-probe > $out/prof_$tag.log 2>&1
