#!/bin/bash
# per-kernel A/B inside ONE GPU session: bench.py's untimed per-kernel HIP-event table (a --full leg) for two builds
#   tools/ab_kernels.sh <libA> <libB> [out dir]  -> <out dir>/abk_A{1,2}.json, abk_B{1,2}.json + a side-by-side table
A=$1; B=$2; OUT=${3:-ab_kernels_out}
mkdir -p "$OUT"
# every run has its own time limit (AB_TIMEOUT seconds, default 600); the first run that fails ends the script
set -o pipefail
for i in 1 2; do
  SUMA_HIP_LIB=$A timeout -k 10 ${AB_TIMEOUT:-600} python bench.py --full --cpu-scans 0 --adapter-scans 0 --no-host-vectors --profile-scans 40 --kernels-json "$OUT/abk_A$i.json" 2>/dev/null | tail -1 | cut -c1-80 || exit 1
  SUMA_HIP_LIB=$B timeout -k 10 ${AB_TIMEOUT:-600} python bench.py --full --cpu-scans 0 --adapter-scans 0 --no-host-vectors --profile-scans 40 --kernels-json "$OUT/abk_B$i.json" 2>/dev/null | tail -1 | cut -c1-80 || exit 1
done
python - "$OUT" <<'PY'
import json
import sys
def load(p):
    return {k["name"]: k for k in json.load(open(p))["kernels"]}
A = [load(f"{sys.argv[1]}/abk_A{i}.json") for i in (1, 2)]
B = [load(f"{sys.argv[1]}/abk_B{i}.json") for i in (1, 2)]
avg = lambda X, n: sum(x[n]["avg_us"] for x in X if n in x) / max(1, sum(n in x for x in X))
for n in A[0]:
    print(f"{n:28s} A {avg(A, n):8.2f} us   B {avg(B, n):8.2f} us   {100.0 * (avg(B, n) / avg(A, n) - 1.0):+6.1f} %")
PY
