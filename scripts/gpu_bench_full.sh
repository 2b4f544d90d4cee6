cd /root/repo; export TMPDIR=/tmp PYTHONUNBUFFERED=1
OUT=${1:?usage: gpu_bench_full.sh OUT_DIR}; mkdir -p "$OUT"
( while true; do sleep 60; echo "[alive $(date +%T)]" >> "$OUT/bench_alive.log"; done ) &
ALIVE=$!
T0=$(date +%s); timeout -k 10 900 python -u bench.py --full > "$OUT/bench_full.json" 2> "$OUT/bench_full.err"
echo "bench rc=$? wall=$(( $(date +%s) - T0 )) s"; kill $ALIVE

python - "$OUT" <<'PY'
import json, sys
d=json.loads([l for l in open(sys.argv[1] + '/bench_full.json') if l.startswith('{')][-1])
print({k:d[k] for k in ('value','ms_per_step','n_gpus')}, d['roofline']['frac'], d['roofline'].get('traffic_source'))
print(d.get('roofline_group_gemm'))
print(d.get('cpu_baseline'))
PY
