#!/bin/bash
# Per-launch HIP-event times (CGP_PROF_DUMP, printed by the profiled steps of bench.py --full) of the working-tree and the prev library:
#   tools/dump_launches.sh <tag> <bench args...>  -> $CGP_OUT/<tag>_dump_{new,prev}.txt (CGP_OUT: the results' directory, default .)
tag=$1; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${CGP_OUT:-.}
for v in new prev; do
  if [ $v = new ]; then lib=$R/corenav_gp_amd/libcorenav_gp.so; else lib=$R/corenav_gp_amd/libcorenav_gp_prev.so; fi
  CGP_LIB=$lib CGP_PROF_DUMP=1 python3 $R/bench.py --full --no-pmc --no-cpu --no-extra --steps 2 --warmup 1 "$@" 2>&1 >/dev/null | grep "cgp prof" > $O/${tag}_dump_$v.txt
done
