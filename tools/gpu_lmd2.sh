#!/bin/bash
set -o pipefail
OUT=${1:?usage: tools/gpu_lmd2.sh OUTDIR}
mkdir -p "$OUT"
python -m pytest tests/ -q -x -m gpu -k "lmd or kpp" > "$OUT"/lmd_tests.log 2>&1
echo "lmd tests rc=$?" >> "$OUT"/lmd_tests.log
tail -3 "$OUT"/lmd_tests.log
python bench.py --steps 20 --warmup 5 --full --no-config5 > "$OUT"/bench_lmd.json 2> "$OUT"/bench_lmd.err
python - "$OUT" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1] + '/bench_lmd.json').read().strip().splitlines()[-1])
print("ms_per_step", d["ms_per_step"], "lmd_vmix", d["kernel_ms"]["lmd_vmix"], "step2d_loop", d["kernel_ms"]["step2d_loop"])
PY
