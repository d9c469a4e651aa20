#!/bin/bash
# the un-profiled bench lines of a profiles/ set (--full: with the kernel rooflines, and the CPU oracle for the training
# step): default (training step, batch 4), eval forward fp32 / bf16 / fp16 -> <out>/<set>_bench_*.json.log
#     bash tools/final_lines.sh <set> [<out>, default bench_out]
SET=${1:-rXX}
OUT=${2:-bench_out}
mkdir -p "$OUT"
python bench.py --full > "$OUT/${SET}_bench_fwdbwd.json.log" 2>"$OUT/${SET}_bench_fwdbwd.err" && echo fwdbwd done
python bench.py --full --mode fwd --steps 30 --warmup 5 --no-cpu-baseline > "$OUT/${SET}_bench_fwd_f32.json.log" 2>/dev/null && echo fwd done
python bench.py --full --mode fwd --dtype bf16 --steps 30 --warmup 5 --no-cpu-baseline > "$OUT/${SET}_bench_fwd_bf16.json.log" 2>/dev/null && echo bf16 done
python bench.py --full --mode fwd --dtype fp16 --steps 30 --warmup 5 --no-cpu-baseline > "$OUT/${SET}_bench_fwd_fp16.json.log" 2>/dev/null && echo fp16 done
