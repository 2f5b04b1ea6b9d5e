#!/bin/bash
# full GPU check: the whole -m gpu suite, then the default bench line with its secondary legs (--full).
#   tools/full_gpu.sh [outdir]   (logs and the bench line go to outdir, default a fresh temporary directory)
O=${1:-$(mktemp -d)}
mkdir -p "$O"; echo "outputs in $O"
timeout -s KILL 1500 python -m pytest tests -m gpu -x -q > "$O/full_gpu_tests.log" 2>&1
echo "pytest rc=$?"; tail -5 "$O/full_gpu_tests.log"
timeout -s KILL 900 python bench.py --full > "$O/bench_cur.json" 2> "$O/bench_cur.err"
echo "bench rc=$?"
python - "$O/bench_cur.json" <<'PY'
import json, sys
j = json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1])
print(j['ms_per_step'], j['value'], j['roofline']['kernel'], j['roofline']['frac'], j.get('hbm_path_frac'), (j.get('alt_arithmetic') or {}).get('ms_per_step'))
for k in j['kernel_breakdown'][:14]: print(k)
PY
