#!/bin/bash
# decode kernels of the C2 bench under rocprofv3 (per-kernel averages) + the round-trip check:  tools/decode_time.sh
# (the decode leg is part of bench.py --full; files go to $TK_OUT_DIR, default bench_out/)
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$(realpath -m "${TK_OUT_DIR:-$R/bench_out}")
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_dec -o dec -- python3 $R/bench.py --full --steps 5 --warmup 2 --cpu-passes 0 --extra-legs none --host-steps 0 --single-docs 0 > $OUT/dec.json 2> $OUT/dec.err || exit 1
cd $R && python -c "
import json, sys; d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print('step', d['ms_per_step'], 'decode ms', d['decode']['ms'], 'round trip exact', d['decode']['round_trip_exact'])" $OUT/dec.json && grep -E "decode" $OUT/prof_dec/dec_kernel_stats.csv | cut -d, -f1-4
