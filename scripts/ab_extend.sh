#!/bin/bash
# A/B of k_extend builds: per-kernel durations of the quick bench for each library variant
ROOT=$(cd "$(dirname "$0")/.." && pwd); OUTS=${BWAHIP_OUT:-$ROOT/bench_out}; mkdir -p $OUTS
cd $ROOT
for v in "" _w6 _w5 _nw _nw5; do
  export BWAHIP_LIB=$ROOT/bwa-mem-gpu_amd/libbwahip$v.so
  OUT=$OUTS/ab$v; mkdir -p $OUT
  (cd /tmp; TMPDIR=/tmp timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 $ROOT/bench.py --full --genome-mbp 128 --reads 2000000 --steps 2 --warmup 1 --overlap 1 --no-cpu-baseline --no-e2e > $OUT/bench.json 2> $OUT/bench.log) || echo "failed $v"
  f=$(find $OUT/trace -name "*kernel_stats.csv" | head -1)
  echo "variant '$v': $(grep -E 'k_extend<3>|k_extend_spec<3>|k_dedup' $f | awk -F, '{printf "%s %.3f ms; ", substr($1,1,50), $4/1e6}')"
  python3 -c "
import json; d=json.load(open('$OUT/bench.json')); print('   single', d['single_context']['value'], 'k_extend stage', d['kernel_ms']['k_extend'], 'ext_max', d['tail_us']['ext_max'])"
done
