#!/bin/bash
# Bench lines of every BASELINE config (run through gpurun from the repo root): configs 3/5/2 and
# SVF with CPU baselines + parity witness, SVF with a 49k-sample warm-up (no CPU leg).
#   bash tools/bench_all.sh TAG
# The lines go to $BENCH_OUT (default bench_out/); `--full` asks bench.py for the roofline's
# measured roof, the detector score, the CPU legs and the witness, which a plain run leaves out.
TAG=${1:-r05}
OUT=${BENCH_OUT:-bench_out}
mkdir -p "$OUT"
bash tools/gpu_steps.sh \
  "${TAG}_bench_c3|280|python -u bench.py --full --steps 10 > $OUT/${TAG}_bench_c3.jsonl" \
  "${TAG}_bench_c5|280|python -u bench.py --full --config 5 --steps 10 > $OUT/${TAG}_bench_c5.jsonl" \
  "${TAG}_bench_c2|280|python -u bench.py --full --config 2 --steps 10 > $OUT/${TAG}_bench_c2.jsonl" \
  "${TAG}_bench_svf|280|python -u bench.py --full --baseline svf --steps 10 > $OUT/${TAG}_bench_svf.jsonl" \
  "${TAG}_bench_svf49k|200|MKID_SVF_WARMUP=49140 python -u bench.py --full --baseline svf --steps 10 --no-cpu-baseline > $OUT/${TAG}_bench_svf49k.jsonl"
