# Round-4 measurement collection (GPU box, repo root): everything under $OUT ; tools/keep_r04.sh copies what is kept
# into profiles/.   bash tools/collect_r04.sh [part]   (part 1: tests + bench lines + traces, part 2: sweeps and
# micro-benchmarks)
set -o pipefail
export OUT=${OUT:?set OUT to the folder the results go to}
mkdir -p $OUT
part=${1:-1}
if [ "$part" = 1 ]; then
timeout -k 10 900 python -m pytest tests -m gpu -x -q -s > $OUT/gpu_tests.log 2>&1; echo "pytest rc=$?"
grep -E "passed|failed" $OUT/gpu_tests.log | tail -2
timeout -k 10 500 python bench.py --full > $OUT/bench_line.json 2> $OUT/bench.err; echo "bench rc=$?"
timeout -k 10 400 python bench.py --full --workload detect > $OUT/bench_detect_line.json 2> $OUT/bench_detect.err; echo "bench detect rc=$?"
( export TMPDIR=${TMPDIR:-/tmp} && timeout -k 10 400 rocprofv3 --kernel-trace -d $OUT/prof_bench -o bench -- python3 bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-detect-record > $OUT/bench_line_under_rocprof.json 2> $OUT/prof_bench.err ); echo "rocprof bench rc=$?"
python tools/prof_summary.py stats $(find $OUT/prof_bench -name "*.db" | head -1) $OUT/bench_kernel_stats.csv && rm -rf $OUT/prof_bench
( export TMPDIR=${TMPDIR:-/tmp} && timeout -k 10 400 rocprofv3 --kernel-trace -d $OUT/prof_detect -o detect -- python3 bench.py --full --workload detect --steps 20 --warmup 3 --no-cpu-baseline > $OUT/bench_detect_line_under_rocprof.json 2> $OUT/prof_detect.err ); echo "rocprof detect rc=$?"
python tools/prof_summary.py stats $(find $OUT/prof_detect -name "*.db" | head -1) $OUT/detect_kernel_stats.csv && rm -rf $OUT/prof_detect
( export TMPDIR=${TMPDIR:-/tmp} && timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/prof_os -o os -- python3 tools/os_pipeline.py --frames 256 --reps 3 > /dev/null 2> $OUT/prof_os.err ); echo "rocprof os rc=$?"
python tools/prof_summary.py stats $(find $OUT/prof_os -name "*.db" | head -1) $OUT/os_kernel_stats.csv && rm -rf $OUT/prof_os
timeout -k 10 300 python tools/os_pipeline.py > $OUT/os_pipeline.json 2> $OUT/os_pipeline.err; echo "os rc=$?"
( timeout -k 10 300 python tools/detect_cus.py --mag32 --splits 32,64,96 && timeout -k 10 100 python tools/detect_cus.py --clocks --splits 32 2>&1 | grep -A1 clocks ) > $OUT/detect_schedules.log 2>&1; echo "schedules rc=$?"
python tools/bench_summary.py $OUT/bench_line.json
else
# (the exactness sweeps: tools/collect_r04_sweeps.sh)
timeout -k 10 400 python tools/kbench.py --frames 1250 --reps 20 > $OUT/kbench.json 2> $OUT/kbench.err; echo "kbench rc=$?"
timeout -k 10 500 python tools/shapes_bench.py > $OUT/shapes.json 2> $OUT/shapes.err; echo "shapes rc=$?"
timeout -k 10 300 python tools/api_latency.py > $OUT/api_latency.json 2> $OUT/api_latency.err; echo "api rc=$?"
fi
