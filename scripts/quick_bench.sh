#!/bin/bash
# GPU tests + a short 128 Mbp bench; prints one summary line.  usage: scripts/quick_bench.sh [notest]
ROOT=$(cd "$(dirname "$0")/.." && pwd); OUTS=${BWAHIP_OUT:-$ROOT/bench_out}; mkdir -p $OUTS
cd $ROOT
if [ "$1" != "notest" ]; then timeout -k 5 400 python -m pytest tests -m gpu -q -x > $OUTS/tests.log 2>&1; echo "tests rc=$?"; tail -2 $OUTS/tests.log; fi
timeout -k 10 200 python bench.py --full --genome-mbp 128 --steps 2 --warmup 1 --no-cpu-baseline > $OUTS/bench_q.json 2> $OUTS/bench_q.log; echo "bench rc=$?"
python3 -c "
import json; d=json.load(open('$OUTS/bench_q.json')); print(d['value'], d['ms_per_step'], d['kernel_ms'], d['tail_us'])"
