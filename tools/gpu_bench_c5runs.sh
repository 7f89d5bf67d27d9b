#!/bin/bash
# the full bench line (with the C5 eight-run leg) at N=1, and the
# N=2 rehearsal (2 gloo ranks sharing one GPU).  Logs: $BLOOMHIP_LOG_DIR/c5r
# (default bench_logs/c5r).
OUT=${BLOOMHIP_LOG_DIR:-bench_logs}/c5r
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 600 python bench.py --full > "$OUT/bench.log" 2>&1 || { tail -5 "$OUT/bench.log"; exit 1; }
grep -o '"c5_eight_runs": {[^}]*}' "$OUT/bench.log"
BLOOMHIP_DIST_BACKEND=gloo timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \
  --master-addr 127.0.0.1 --master-port 29512 bench.py --gpus 2 --steps 20 --warmup 5 --full --no-cpu-baseline \
  > "$OUT/bench_dist2.log" 2>&1 || { tail -5 "$OUT/bench_dist2.log"; exit 1; }
grep -o '"c5_eight_runs": {[^}]*}' "$OUT/bench_dist2.log"
