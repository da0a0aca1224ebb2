#!/bin/bash
# In-engine sweep of the backward's out-CSR chunk (bench.py --chunk-bwd) for one config;
# one line per chunk under $OUT_DIR (default bench_out/).
#   CONFIG=cfg5 CHUNKS="128 256 512" bash scripts/chunk_ab.sh
cd "$(dirname "$0")/.." && O=${OUT_DIR:-bench_out} && mkdir -p $O && export TMPDIR=/tmp
for c in ${CHUNKS:-64 128}; do
  timeout -k 10 300 python bench.py --full --config ${CONFIG:-cfg2} --no-cpu-baseline --no-legs --sub-configs= --chunk-bwd $c > $O/chunk_${CONFIG:-cfg2}_$c.json 2> $O/chunk_${CONFIG:-cfg2}_$c.err || exit 1
  python3 -c "
import json
d=json.loads([l for l in open('$O/chunk_${CONFIG:-cfg2}_$c.json') if l.startswith('{')][-1])
print('${CONFIG:-cfg2} chunk $c', d['ms_per_step'], d['kernels_ms_per_step'])"
done
