#!/bin/bash
# Top kernels of one bench configuration (GPU box):  tools/kprof.sh citation2 [extra bench flags]
cfg=$1; shift
O=${OCN_OUT_DIR:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
rm -rf $O/kprof_tmp
rocprofv3 --kernel-trace --stats -d $O/kprof_tmp -o run --output-format csv -- python bench.py --full --config $cfg --steps 32 --warmup 5 --no-cpu-baseline --prewarm 8 "$@" > $O/kprof_$cfg.json 2> /dev/null
python - <<PY
import csv, glob, json
f = glob.glob("$O/kprof_tmp/**/*kernel_stats.csv", recursive=True)[0]
for r in list(csv.DictReader(open(f)))[:int("${KPROF_ROWS:-14}")]:
    print(r["Name"][:64].ljust(64), r["Calls"].rjust(5), str(round(float(r["AverageNs"]) / 1e3, 1)).rjust(9), r["MinNs"], r["MaxNs"])
d = json.loads(open("$O/kprof_$cfg.json").read().strip().splitlines()[-1])
print("$cfg", round(d["value"]), d["ms_per_step"])
PY
rm -rf $O/kprof_tmp
