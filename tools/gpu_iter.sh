#!/bin/bash
# one perf iteration on the GPU box: parity tests, bench (kernel ms), phase cycles.   usage: tools/gpu_iter.sh <tag> <output dir>
TAG=${1:-it}
OUT=${2:?usage: tools/gpu_iter.sh <tag> <output dir>}
mkdir -p $OUT
python -m pytest tests/test_gpu_parity.py tests/test_gpu_scale.py -x -q > $OUT/${TAG}_tests.log 2>&1; tail -3 $OUT/${TAG}_tests.log
python bench.py --full --no-cpu-baseline --steps 2000 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
python -c "
import json; d=json.load(open('$OUT/${TAG}_bench.json')); print('BENCH', d['value'], d['roofline']['kernel_ms'], d['roofline']['kernel_ms_back_to_back'])"
python tools/phase_cycles.py 300 > $OUT/${TAG}_phase.txt 2>&1; tail -17 $OUT/${TAG}_phase.txt
