#!/bin/bash
# dev tool: per-kernel averages (rocprofv3) of the default bench for each prebuilt library variant in csrc/_variants/
R=$(cd "$(dirname "$0")/.." && pwd)
T=${TMPDIR:-/tmp}
cd $T && export TMPDIR=$T
for v in "$@"; do
  cp $R/hcatgnet_amd/csrc/_variants/$v.so $R/hcatgnet_amd/csrc/libhcatgnet_hip.so
  rm -rf $T/prof_$v
  rocprofv3 --kernel-trace --stats --output-format csv -d $T/prof_$v -- python $R/bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-graph > /dev/null 2> $T/log_$v.txt
  f=$(find $T/prof_$v -name "*kernel_stats.csv" | head -1)
  echo "== variant $v: $(grep 'timed eager' $T/log_$v.txt)"
  python - "$f" <<'PY'
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if float(r['TotalDurationNs']) > 5e5: print("  ", r['Name'].replace('(anonymous namespace)::','')[:60].ljust(60), r['Calls'], round(float(r['AverageNs'])/1e3, 2))
PY
done
