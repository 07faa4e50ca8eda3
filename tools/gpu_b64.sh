#!/bin/bash
# GPU-box helper for the batched (configs[2]) path: batched decoder tests, the B=64 bench line and
# its rocprofv3 kernel statistics ($BENCH_OUT/prof_b64_summary.txt, default bench_out/).  SKIP_TESTS=1 skips the tests.
set -o pipefail
R=$(pwd)
mkdir -p gpurun_out
if [ -z "$SKIP_TESTS" ]; then
timeout -k 10 400 python -u -m pytest tests/test_gpu_parity.py tests/test_gpu_batched.py -x -q --timeout 200 --timeout-method thread -p no:cacheprovider -k "batch or overlap or ragged or teacher or config" > gpurun_out/pt_b64.log 2>&1 || { echo batched tests failed; grep -E "FAILED|Error" gpurun_out/pt_b64.log | head; tail -30 gpurun_out/pt_b64.log; exit 1; }
tail -2 gpurun_out/pt_b64.log
fi
O=$R/${BENCH_OUT:-bench_out} && mkdir -p $O
timeout -k 10 300 python bench.py --full --batch 64 --lengths uniform --no-cpu-baseline --no-share > $O/bench_b64.json 2> $O/bench_b64.err && python tools/bench_digest.py $O/bench_b64.json || { tail -20 $O/bench_b64.err; exit 1; }
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_b64 -o run --output-format csv -- python $R/bench.py --full --batch 64 --lengths uniform --steps 2 --warmup 1 --no-cpu-baseline --no-profile --no-share > $O/prof_b64_bench.json 2> $O/prof_b64.err || { echo rocprof failed; tail -20 $O/prof_b64.err; exit 1; }
python $R/tools/rocprof_summary.py $O/prof_b64/run_kernel_stats.csv $O/prof_b64_summary.txt | head -16
