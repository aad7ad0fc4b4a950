#!/bin/bash
# PMC evidence of the training step (GPU box): kernel trace + three counter passes over the same bench command.
export TMPDIR=/tmp; OUT=${OUT:-evidence}; mkdir -p $OUT
R=${ROUND:-r06}
CMD="python bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-nms --no-roofline --no-extras --no-graph"
rocprofv3 -L > $OUT/${R}_counters_list.txt 2>&1
for P in trace fetch write sq; do rm -rf $OUT/${R}_pmc_$P; done
timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/${R}_pmc_trace -- $CMD > $OUT/${R}_pmc_trace.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/${R}_pmc_fetch -- $CMD > $OUT/${R}_pmc_fetch.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/${R}_pmc_write -- $CMD > $OUT/${R}_pmc_write.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/${R}_pmc_sq -- $CMD > $OUT/${R}_pmc_sq.log 2>&1
python tools/pmc_step.py $OUT/${R}_pmc_trace $OUT/${R}_pmc_fetch $OUT/${R}_pmc_write $OUT/${R}_pmc_sq > $OUT/${R}_pmc_step.txt 2> $OUT/${R}_pmc_step.err
head -3 $(find $OUT/${R}_pmc_sq -name "*counter_collection.csv" | head -1) > $OUT/${R}_pmc_sq_head.txt 2>&1
grep -i -E "MFMA|BUSY" $OUT/${R}_counters_list.txt | head -40 > $OUT/${R}_counters_mfma.txt
for P in trace fetch write sq; do rm -rf $OUT/${R}_pmc_$P; done
head -30 $OUT/${R}_pmc_step.txt; cat $OUT/${R}_pmc_step.err | tail -5; cat $OUT/${R}_pmc_sq_head.txt
