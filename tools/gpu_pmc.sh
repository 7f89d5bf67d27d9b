#!/bin/bash
# PMC counter passes (no tracing domains besides kernel-trace) on the C2 build
# and the C3 probe.  Usage: tools/gpu_pmc.sh TAG
# Output: $BLOOMHIP_LOG_DIR/TAG and TAG.log (default bench_logs/).
OUT=${BLOOMHIP_LOG_DIR:-bench_logs}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${1:-pmc}
timeout -k 10 600 rocprofv3 -i tools/pmc/counters.txt --kernel-trace -d "$OUT/$TAG" -o pmc --output-format csv -- python bench.py --steps 10 --warmup 2 --full --no-cpu-baseline > "$OUT/$TAG.log" 2>&1
rc=$?; echo "rc=$rc"; tail -3 "$OUT/$TAG.log"; find "$OUT/$TAG" -name "*.csv" | head -20
