#!/bin/bash
# rocprofv3 kernel-trace + stats (round 3): the full bench (--full: vanilla step at bf16 images + fp8 secondary + render), the
# Instant-NGP workload and the Part 4 engine loop; only the per-kernel statistics travel back -> copy into profiles/
#   usage: bash tools/profile_r03.sh <output folder>
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${1:?usage: bash tools/profile_r03.sh <output folder>}
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT" -o bench -- python3 bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --no-instant --no-part4 > "$OUT/bench_stdout.log" 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT" -o instant -- python3 bench.py --workload instant --steps 30 > "$OUT/instant_stdout.log" 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT" -o part4 -- python3 tools/part4_profile_loop.py 96 > "$OUT/part4_stdout.log" 2>&1
# the per-dispatch traces are large: only the per-kernel statistics travel back
find "$OUT" -name '*_kernel_trace.csv' -delete
ls -la "$OUT" | head -30
