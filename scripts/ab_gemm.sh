#!/bin/bash
# A/B of a `make variant` GEMM library (V) against the product build on the cfg2 step:
# GEMM tests on the product build, then bench.py --full (no sub-configs / legs / CPU baseline)
# for each library, alternating, and the per-group times. Output under $OUT_DIR (default
# bench_out/).
cd "$(dirname "$0")/.." && O=${OUT_DIR:-bench_out} && mkdir -p $O
timeout -k 10 300 python -u -m pytest tests/test_gpu_kernels.py -k "gemm" -x -q --timeout 200 --timeout-method thread > $O/ab_gemm_tests.log 2>&1
rc=$?; tail -2 $O/ab_gemm_tests.log; [ $rc -eq 0 ] || exit $rc
for rep in 1 2; do
  for v in base $V; do
    if [ "$v" = "base" ]; then unset PLAGNN_LIB; else export PLAGNN_LIB=$PWD/pla-gnn_amd/plagnn/libplagnn_$v.so; fi
    timeout -k 10 300 python -u bench.py --full --config ${CONFIG:-cfg2} --sub-configs= --no-cpu-baseline --no-legs --steps 30 > $O/ab_gemm_${v}_$rep.json 2> $O/ab_gemm_${v}_$rep.err || { echo "bench $v failed"; tail -5 $O/ab_gemm_${v}_$rep.err; exit 1; }
    python3 -c "
import json;d=json.loads(open('$O/ab_gemm_${v}_$rep.json').read().splitlines()[-1])
print('$v', d['ms_per_step'], d['kernels_ms_per_step'], d['roofline']['achieved'])"
  done
done
