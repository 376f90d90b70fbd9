#!/bin/bash
# quick GPU check after a kernel change: parity tests of the flat path, then the C2 bench line (kernel_ms, pipeline_ms)
# (bench.py --full for the decode leg; logs go to $TK_OUT_DIR, default bench_out/)
root=${GRAFT_REPO_ROOT:-$(pwd)}
cd $root
OUT=$(realpath -m "${TK_OUT_DIR:-$root/bench_out}")
mkdir -p $OUT
timeout -k 10 300 python -m pytest tests/test_gpu_parity.py -x -q > $OUT/quick_tests.log 2>&1 || { tail -30 $OUT/quick_tests.log; exit 1; }
tail -1 $OUT/quick_tests.log
timeout -k 10 200 python bench.py --full --cpu-passes 0 --extra-legs none ${BENCH_ARGS} 2> $OUT/quick_bench.err | python -c "
import sys, json
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
r = d['roofline']
print('value', d['value'], 'ms_per_step', d['ms_per_step'], 'kernel_ms', r['kernel_ms'], 'frac', r['frac'], 'exact', d.get('bit_exact_vs_cpu'), 'decode', (d.get('decode') or {}).get('ms'))"
