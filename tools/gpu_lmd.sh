#!/bin/bash
set -o pipefail
OUT=${1:?usage: tools/gpu_lmd.sh OUTDIR}
mkdir -p "$OUT"
python -m pytest tests/ -q -x -m gpu -k "lmd or kpp or physics or smoke" > "$OUT"/lmd_tests.log 2>&1
echo "lmd tests rc=$?" >> "$OUT"/lmd_tests.log
tail -5 "$OUT"/lmd_tests.log
python bench.py --steps 20 --warmup 5 --full --no-config5 --no-cpu-baseline > "$OUT"/bench_lmd.json 2> "$OUT"/bench_lmd.err
python -c "import json; d=json.loads(open('$OUT/bench_lmd.json').read().strip().splitlines()[-1]); print(d['ms_per_step'], d['kernel_ms']['lmd_vmix'])"
