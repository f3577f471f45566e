#!/bin/bash
# two-plane (product) vs three-plane (-DPDSC_W_PLANES=3,
# libpdsc_w3.so) 1x1-conv weights -- per golden the h3 error against the
# reference and against the exact-fp32 mode (tools/parity_report.py), and the
# bench pairs' parity block (bench.py --full's cpu leg runs the oracle on all 128 pairs).
# Logs go to $PDSC_OUT (default: out/ in the repository root).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${PDSC_OUT:-out}
mkdir -p "$OUT"
for v in w2 w3; do
  lv=""; [ "$v" = w3 ] && lv=w3
  PDSC_LIB_VARIANT=$lv timeout -k 10 300 python -u tools/parity_report.py --precision h3 > "$OUT/planes_$v.jsonl" 2> "$OUT/planes_$v.err" || { tail -20 "$OUT/planes_$v.err"; exit 1; }
  PDSC_LIB_VARIANT=$lv timeout -k 10 300 python bench.py --full --steps 5 --warmup 2 --f32-steps 0 --path-n 0 > "$OUT/planes_bench_$v.log" 2>&1 || { tail -20 "$OUT/planes_bench_$v.log"; exit 1; }
  echo "== $v"; tail -1 "$OUT/planes_bench_$v.log" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('ms/step', d['ms_per_step'], 'parity', json.dumps(d['parity']['h3']))"
done
