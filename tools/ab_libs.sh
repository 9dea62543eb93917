#!/bin/bash
# A/B of library builds inside ONE gpurun call (boxes of the pool differ by 3-5 %): bash tools/ab_libs.sh out.txt lib1 lib2 ...
# per library and round: back-to-back kernel timings at cfg4 and cfg5 (fp32 storage), then solve loops, then bench.py.
OUT=$1; shift
D=$GRAFT_REPO_ROOT/sfm-python_amd/sfmba
: > $OUT
for round in 1 2; do
  for L in "$@"; do
    SFMBA_LIB=$D/$L python3 tools/time_kernels.py cfg4 0,7,2,4,5,8 64 >> $OUT 2>&1
    SFMBA_LIB=$D/$L python3 tools/time_kernels.py cfg5 0,7,2,4,5,8 32 >> $OUT 2>&1
  done
done
for L in "$@"; do
  for c in cfg4 cfg3 cfg2; do echo -n "$L " >> $OUT; SFMBA_LIB=$D/$L python3 tools/solve_loop.py $c >> $OUT 2>&1; done
  echo -n "$L " >> $OUT; SFMBA_LIB=$D/$L python3 tools/solve_loop.py cfg5 6 32 >> $OUT 2>&1
  echo -n "$L " >> $OUT; SFMBA_LIB=$D/$L python3 tools/solve_loop.py cfg5 6 64 >> $OUT 2>&1
done
# bench.py itself (default arguments), per library and round, alternating: the `value`, launches per iteration and K1's
# in-solve duration of every run on one line
for round in 1 2 3; do
  for L in "$@"; do
    echo -n "$L bench.py " >> $OUT
    SFMBA_LIB=$D/$L timeout -k 10 300 python3 bench.py --gpus 1 2>/dev/null | python3 -c '
import json, sys
for line in sys.stdin:
    if line.startswith("{"):
        r = json.loads(line)
        print("value %.1f" % r["value"], "launches_per_iteration", r.get("launches_per_iteration"),
              "K1 avg_launch_us", (r.get("roofline") or {}).get("avg_launch_us"))' >> $OUT 2>&1
  done
done
cat $OUT
