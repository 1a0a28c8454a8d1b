#!/bin/bash
# Kernel-stats run and PMC passes (each a run of its own) of the window forecast: tools/pmc_window_forecast.sh <tag> <output directory>
tag=$1
O=${2:?output directory}
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$O" && O=$(cd "$O" && pwd)
W=$(mktemp -d) && cd "$W" && export TMPDIR=$W
CMD="python3 $R/tools/bench_window.py --windows 1024 --ticks 8 --forecast 599 --reps 5"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${tag}_stats -o s -- $CMD > $O/${tag}_stats.log 2>&1
i=0
for c in "FETCH_SIZE" "TCC_HIT_sum TCC_MISS_sum" "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE" "SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_VALU SQ_WAIT_INST_LDS"; do
  i=$((i+1))
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/${tag}_pmc$i -o p -- $CMD > $O/${tag}_pmc$i.log 2>&1
done
