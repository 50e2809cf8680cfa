#!/bin/bash
set -o pipefail
OUT=${1:?usage: tools/gpu_s2d.sh OUTDIR}
mkdir -p "$OUT"
python -m pytest tests/test_gpu_kernels.py tests/test_gpu_main3d.py tests/test_masking.py -q -x -m gpu -k "step2d or steps or main3d" > "$OUT"/s2d_tests.log 2>&1
echo "s2d tests rc=$?" >> "$OUT"/s2d_tests.log
tail -3 "$OUT"/s2d_tests.log
python bench.py --steps 20 --warmup 5 --full --no-config5 --no-cpu-baseline > "$OUT"/bench_s2d.json 2> "$OUT"/bench_s2d.err
python - "$OUT" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1] + '/bench_s2d.json').read().strip().splitlines()[-1])
print("ms_per_step", d["ms_per_step"], "step2d_loop", d["kernel_ms"]["step2d_loop"], "lmd_vmix", d["kernel_ms"]["lmd_vmix"])
PY
