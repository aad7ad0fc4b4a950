#!/bin/bash
# decode + NMS evidence only (part of round_end.sh): by-grid kernel tables of the hot and the all-candidates input + the bench's nms object
cd "$(dirname "$0")/.."; OUT=${OUT:-evidence}; mkdir -p $OUT; export TMPDIR=/tmp; R=${ROUND:-r04}
rm -rf $OUT/${R}_nms_prof
timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/${R}_nms_prof -o nms -- python tools/nms_prof.py > $OUT/${R}_nms.log 2>&1
python tools/by_grid.py $(find $OUT/${R}_nms_prof -name "nms_kernel_trace.csv" | head -1) > $OUT/${R}_nms_kernels_by_grid.txt
rm -rf $OUT/${R}_nms_prof
timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/${R}_nms_prof -o nms -- python tools/nms_prof.py stress > $OUT/${R}_nms_stress.log 2>&1
python tools/by_grid.py $(find $OUT/${R}_nms_prof -name "nms_kernel_trace.csv" | head -1) > $OUT/${R}_nms_stress_kernels_by_grid.txt
rm -rf $OUT/${R}_nms_prof
timeout 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-roofline --no-extras 2>&1 | tail -1 | python -c "
import json,sys; d=json.loads(sys.stdin.read()); print(json.dumps(d['nms']))" > $OUT/${R}_nms_line.json
cat $OUT/${R}_nms_line.json; head -9 $OUT/${R}_nms_kernels_by_grid.txt | cut -c1-130
