#!/bin/bash
# A/B builds of libsuma_hip.so inside ONE gpurun session (box-to-box variance is ~5 %):
#   tools/ab.sh <libA.so> <libB.so> [more .so ...] [-- bench args]   -> interleaved runs, prints scans/s
# every run has its own time limit (AB_TIMEOUT seconds, default 600); the first run that fails ends the script
set -o pipefail
LIBS=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do LIBS+=("$1"); shift; done
[ "$1" == "--" ] && shift
for i in 1 2 3; do
  for L in "${LIBS[@]}"; do
    v=$(SUMA_HIP_LIB=$L timeout -k 10 ${AB_TIMEOUT:-600} python bench.py --cpu-scans 0 --no-kernel-events --adapter-scans 0 --no-host-vectors "$@" 2>/dev/null | tail -1 | python -c "import sys,json; print(round(json.loads(sys.stdin.read())['value'],1))") || { echo "$L: run failed" >&2; exit 1; }
    echo "$L $v"
  done
done
