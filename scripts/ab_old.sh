#!/bin/bash
# A/B: current library against one with round 2's k_extend.hip (fused dedup, no window), full-size genome, one context, per-kernel durations
ROOT=$(cd "$(dirname "$0")/.." && pwd); OUTS=${BWAHIP_OUT:-$ROOT/bench_out}; mkdir -p $OUTS
cd $ROOT
timeout -k 10 300 python bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-other-configs --no-e2e --reads 2000000 > $OUTS/ab_warm.json 2> $OUTS/ab_warm.log   # builds the index
for v in "" _old ""  _old; do
  export BWAHIP_LIB=$ROOT/bwa-mem-gpu_amd/libbwahip$v.so
  timeout -k 10 300 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-other-configs --no-e2e --reads 3000000 --overlap 1 > $OUTS/abo$v.json 2> $OUTS/abo$v.log || echo "failed $v"
  python3 -c "
import json; d=json.load(open('$OUTS/abo$v.json')); k=d['kernel_ms']; print('variant [$v]: single', d['single_context']['value'], 'k_extend', k['k_extend'], 'spec', k['k_extend_spec'], 'k_chain', k['k_chain'], 'sum', round(sum(k.values()),1), 'tails', d['tail_us']['ext_max'], d['tail_us']['ext_dedup_max'])"
done
