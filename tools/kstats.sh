#!/bin/bash
# Kernel-trace summary of one bench configuration (run on the GPU box):  tools/kstats.sh <dataset> [bench args]
# -> $OCN_OUT_DIR/kstats_<dataset>.csv (default bench_out/) and the ten longest kernels on stdout.
C=$1; shift
O=${OCN_OUT_DIR:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
rm -rf $O/prof_k
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_k -o run --output-format csv -- python3 bench.py --full --dataset $C --no-validate-leg --no-cpu-baseline --steps 32 "$@" > $O/kstats_$C.log 2>&1
cp $(find $O/prof_k -name "*kernel_stats.csv" | head -1) $O/kstats_$C.csv
rm -rf $O/prof_k
python3 - <<PY
import csv
for r in list(csv.DictReader(open("$O/kstats_$C.csv")))[:10]:
    print(f"{r['Name'][:70]:70s} {r['Calls']:>5s} {float(r['AverageNs'])/1e3:9.1f} us {r['Percentage']:>6s}%")
PY
