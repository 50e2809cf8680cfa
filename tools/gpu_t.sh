#!/bin/bash
# the tracer step: its tests, then a short bench (driver line of step3d_t)
set -o pipefail
OUT=${1:?usage: tools/gpu_t.sh OUTDIR}
mkdir -p "$OUT"
python -m pytest tests/test_gpu_kernels.py tests/test_gpu_main3d.py tests/test_masking.py tests/test_basin.py tests/test_golden.py tests/test_gpu_sources.py -q -x -m gpu -k "step3d_t or steps or main3d or levels or tracer or golden or 100" > "$OUT"/t_tests.log 2>&1
echo "t tests rc=$?" >> "$OUT"/t_tests.log
tail -3 "$OUT"/t_tests.log
for r in 1 2; do
python bench.py --steps 30 --warmup 5 --full --no-config5 --no-cpu-baseline > "$OUT"/bench_t.json 2> "$OUT"/bench_t.err
python - "$OUT" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1] + '/bench_t.json').read().strip().splitlines()[-1])
print("ms_per_step", d["ms_per_step"], "step3d_t", d["kernel_ms"]["step3d_t"], "frac", d["roofline"]["frac"], "avg_ms", d["roofline"]["avg_ms"])
PY
done
