# Round-2 measurement collection (GPU box, repo root): writes everything under $OUT
set -o pipefail
export OUT=${OUT:?set OUT to the folder the results go to}
mkdir -p $OUT
timeout -k 10 600 python -m pytest tests -m gpu -x -q -s > $OUT/gpu_tests.log 2>&1; echo "pytest rc=$?"
grep -E "schedule|sweep|bound divisor|passed|failed" $OUT/gpu_tests.log | tail -12
MMW_SWEEP_FRAMES=2000 MMW_SWEEP_PROCS=32 timeout -k 10 600 python -m pytest tests/test_gpu_sweep.py -m gpu -x -q -s -k os_cfar > $OUT/os_sweep.log 2>&1; grep -E "sweep|passed|failed" $OUT/os_sweep.log
timeout -k 10 400 python bench.py --full > $OUT/bench_line.json 2> $OUT/bench.err; echo "bench rc=$?"
timeout -k 10 400 python bench.py --full --workload detect > $OUT/bench_detect_line.json 2> $OUT/bench_detect.err; echo "bench detect rc=$?"
timeout -k 10 400 python tools/kbench.py --frames 1250 --reps 20 > $OUT/kbench.json 2> $OUT/kbench.err
timeout -k 10 400 python tools/kbench.py --shape 12,63,100 --frames 2048 > $OUT/kbench_63x100.json 2> $OUT/kbench_63x100.err
timeout -k 10 500 python tools/shapes_bench.py > $OUT/shapes.json 2> $OUT/shapes.err
timeout -k 10 300 python tools/membw.py > $OUT/membw.json 2> $OUT/membw.err
timeout -k 10 300 python tools/api_latency.py > $OUT/api_latency.json 2> $OUT/api_latency.err
python - <<'PY'
import json, os
OUT = os.environ["OUT"]
r=json.load(open(f"{OUT}/bench_line.json")); print("bench", r["value"], r["roofline"]["frac"], r["parity_max_rel_err"], r.get("cpu_baseline",{}).get("value"), r.get("cpu_baseline_all_cores",{}).get("value"))
r=json.load(open(f"{OUT}/bench_detect_line.json")); print("detect", r["value"], r["kernels_ms_per_step"], r["parity"], r.get("cpu_baseline",{}).get("value"))
print(open(f"{OUT}/api_latency.json").read())
PY

# ---- copy what is kept into profiles/ (tracked)
cp $OUT/bench_line.json profiles/r02_bench_line.json
cp $OUT/bench_detect_line.json profiles/r02_bench_detect_line.json
cp $OUT/kbench.json profiles/r02_kbench.json
cp $OUT/kbench_63x100.json profiles/r02_kbench_63x100.json
cp $OUT/shapes.json profiles/r02_shapes.json
cp $OUT/membw.json profiles/r02_membw.json
cp $OUT/gpu_tests.log profiles/r02_gpu_tests.log
cp $OUT/os_sweep.log profiles/r02_os_sweep.log
