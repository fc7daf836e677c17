#!/bin/bash
# usage: scripts/env_sweep.sh VAR v1 v2 ...  -> short 128 Mbp bench per value
ROOT=$(cd "$(dirname "$0")/.." && pwd); OUTS=${BWAHIP_OUT:-$ROOT/bench_out}; mkdir -p $OUTS
cd $ROOT
VAR=$1; shift
for v in "$@"; do
  env $VAR=$v timeout -k 10 200 python bench.py --full --genome-mbp 128 --steps 2 --warmup 1 --no-cpu-baseline > $OUTS/sweep_$v.json 2> $OUTS/sweep_$v.log
  python3 -c "
import json; d=json.load(open('$OUTS/sweep_$v.json')); print('$VAR=$v', d['value'], {k: round(x,2) for k,x in d['kernel_ms'].items() if x > 1}, d['tail_us']['chain_build_max'], d['tail_us']['chain_sort_max'])"
done
