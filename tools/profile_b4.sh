#!/bin/bash
# rocprofv3 kernel trace of the default bench (per-GPU batch 4; --full: the kernel_roofline() micro-benchmarks are in the
# trace too) -> <out>/<set>_fwdbwd_b4_{kernel_stats.csv,step_breakdown.txt}
#     bash tools/profile_b4.sh <set> [<out>, default bench_out]
set -e
SET=${1:-rXX}
OUT=${2:-bench_out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_${SET}_b4" -- python bench.py --full --steps 4 --warmup 2 --no-cpu-baseline > "$OUT/${SET}_fwdbwd_b4.log" 2>&1
cp "$(ls -t "$OUT"/prof_${SET}_b4/*/*_kernel_stats.csv | head -1)" "$OUT/${SET}_fwdbwd_b4_kernel_stats.csv"
python tools/step_breakdown.py "$(ls -t "$OUT"/prof_${SET}_b4/*/*_kernel_trace.csv | head -1)" 60 --by-grid > "$OUT/${SET}_fwdbwd_b4_step_breakdown.txt"
rm -rf "$OUT/prof_${SET}_b4"
