#!/bin/bash
# GPU-box helper for the batch-1 (configs[1]) path: resident decoder / encoder tests, the event
# trace, the bench line and its rocprofv3 kernel statistics ($BENCH_OUT/prof_b1_summary.txt, default bench_out/).
set -o pipefail
R=$(pwd)
mkdir -p gpurun_out
timeout -k 10 400 python -u -m pytest tests/test_gpu_resident.py tests/test_gpu_coresidency.py tests/test_gpu_parity.py -x -q --timeout 200 --timeout-method thread -p no:cacheprovider -k "resident or encoder or synthesize or configs1" > gpurun_out/pt_b1.log 2>&1 || { echo b1 tests failed; grep -E "FAILED|Error" gpurun_out/pt_b1.log | head; tail -30 gpurun_out/pt_b1.log; exit 1; }
tail -1 gpurun_out/pt_b1.log
timeout -k 10 200 python tools/resident_trace.py > gpurun_out/trace.json 2>gpurun_out/trace.err || { tail gpurun_out/trace.err; exit 1; }
python -c "
import json;d=json.load(open('gpurun_out/trace.json'))
print('trace us/step', round(d['us_per_step_trace'],3))
for k,v in d['events_rel_step_start_us(min,median,max)'].items(): print(' ', k, v)
print(d['last_cu'])"
O=$R/${BENCH_OUT:-bench_out} && mkdir -p $O
timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-share > $O/bench_b1.json 2> $O/bench_b1.err && python tools/bench_digest.py $O/bench_b1.json || { tail -20 $O/bench_b1.err; exit 1; }
cd /tmp && export TMPDIR=/tmp
TTS_COOP=0 timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_b1 -o run --output-format csv -- python $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-profile --no-share > $O/prof_b1_bench.json 2> $O/prof_b1.err || { echo rocprof failed; tail -20 $O/prof_b1.err; exit 1; }
python $R/tools/rocprof_summary.py $O/prof_b1/run_kernel_stats.csv $O/prof_b1_summary.txt | head -14
