#!/bin/bash
# PMC passes for the F-solve kernel: one rocprofv3 run per counter group, kernel trace only (counters are never combined with
# other tracing).  Every pass runs under its own time limit and the script stops at the first one that fails: nothing more is
# started on a device that has just faulted or hung.
# usage: scripts/pmc_fsolve.sh <outdir> [config: c3 | c5] [passes, e.g. "5 6 7"] [extra env assignments]
#   passes 1-4: SQ / TCP activity; 5: FETCH_SIZE, 6: WRITE_SIZE, 7: TCC_HIT TCC_MISS -- "5 6 7" is all the traffic record needs
#   (scripts/make_traffic_json.py).  Default: all seven.  PMC_TIMEOUT: seconds per pass (default 600).
#   The passes' files go to $PMC_OUT/<outdir> (default build/pmc/<outdir>); the summary is printed.
set -euo pipefail
OUT=$1; shift
CFG=c3
case "${1:-}" in c3|c5) CFG=$1; shift;; esac
PASSES="1 2 3 4 5 6 7"
case "${1:-}" in [1-7]*) PASSES=$1; shift;; esac
R=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp; export TMPDIR=/tmp
D=${PMC_OUT:-$R/build/pmc}/$OUT; mkdir -p $D
COUNTERS=("" \
  "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_VALU_MFMA_BUSY_CYCLES" \
  "SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT" \
  "SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_MISC SQ_INST_CYCLES_VMEM_RD SQ_LDS_IDX_ACTIVE SQ_IFETCH SQ_INSTS_BRANCH SQ_INSTS_SMEM" \
  "GRBM_GUI_ACTIVE GRBM_TA_BUSY TCP_TOTAL_CACHE_ACCESSES TCP_TCC_READ_REQ TCP_PENDING_STALL_CYCLES TCP_TCP_TA_DATA_STALL_CYCLES" \
  "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT TCC_MISS")
FIRST=
for i in $PASSES; do
  FIRST=${FIRST:-$i}
  env "$@" timeout -k 10 ${PMC_TIMEOUT:-600} rocprofv3 --kernel-trace --pmc ${COUNTERS[$i]} --kernel-include-regex "fsolve" --output-format csv \
      -d $D/p$i -o pmc -- python $R/scripts/bench_fsolve.py $CFG > $D/p$i.log 2>&1 \
      || { rc=$?; echo "pass $i failed (exit $rc): $D/p$i.log" >&2; tail -5 $D/p$i.log >&2; exit $rc; }
done
python - <<PY
import csv, glob, collections, os
agg=collections.defaultdict(list)
for i in '$PASSES'.split():
    for f in sorted(glob.glob('$D/p%s/**/*counter_collection.csv' % i, recursive=True)):
        for row in csv.DictReader(open(f)):
            agg[row['Counter_Name']].append(float(row['Counter_Value']))
print(next(l.strip() for l in open('$D/p$FIRST.log') if l.startswith('$CFG nnz=')))      # bench_fsolve.py's line (the log also holds the profiler's)
print('counter averages per dispatch (fsolve kernels), config $CFG:')
for k,v in agg.items(): print('  %-32s %16.1f  (n=%d)' % (k, sum(v)/len(v), len(v)))
PY
