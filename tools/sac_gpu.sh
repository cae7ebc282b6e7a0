#!/bin/bash
# SAC GPU pass: parity tests, bf16 + fp32 bench, rocprofv3 kernel stats ($OUT_DIR, default build/sac)
set -o pipefail
export TMPDIR=/tmp
O=${OUT_DIR:-build/sac}
mkdir -p $O
timeout -k 10 300 python -u -m pytest tests/test_gpu_sac.py -x -q --timeout 120 --timeout-method thread > $O/tests.log 2>&1 || exit $?
timeout -k 10 200 python bench.py --full --algo sac --steps 200 --warmup 20 --cpu-seconds 12 > $O/bench_bf16.json 2> $O/bench_bf16.err || exit $?
timeout -k 10 200 python bench.py --full --algo sac --dtype fp32 --steps 200 --warmup 20 --no-cpu-baseline > $O/bench_fp32.json 2> $O/bench_fp32.err || exit $?
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/stats -o run --output-format csv -- python3 bench.py --full --algo sac --steps 50 --warmup 5 --no-cpu-baseline --roofline-kernel critic_fwd_chain > $O/bench_stats.json 2> $O/stats.err
echo "rocprof rc=$?"
