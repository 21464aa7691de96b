#!/bin/bash
# One GPU round trip: parity tests, then the given bench variants (--full runs:
# each line's topk_vs_reference is read), output under $OUT_ROOT (default bench_out).
# usage (on the GPU box): bash tools/gpu_check.sh [tests|notests] "<bench args>" ...
set -o pipefail
D=${OUT_ROOT:-bench_out}
mkdir -p $D
if [ "$1" = "tests" ]; then
  timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $D/gpu_tests.log 2>&1 || { tail -30 $D/gpu_tests.log; exit 1; }
  tail -2 $D/gpu_tests.log
fi
shift
i=0
for a in "$@"; do
  i=$((i+1))
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-north-star $a > $D/b$i.json 2> $D/b$i.err || { tail -20 $D/b$i.err; exit 1; }
  python -c "import json,sys; d=json.load(open('$D/b$i.json')); print('$a', d['value'], d['kernel']['name'], d['kernel']['avg_ms'], d['kernel']['kernel_gcups'], d['kernel']['wide_count'], d['kernel']['wide_ms_avg'], d['top_hit'], d.get('topk_vs_reference'))"
done
