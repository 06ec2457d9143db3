#!/bin/bash
# A/B of two library builds on one GPU: digests (bit-neutrality), then bench lines old / new / old / new.
# usage: scripts/ab_builds.sh <dir of the OLD libs>      (AB_OUT: where the two digest files go, default build/ab)
# Every GPU step runs under its own time limit and the script stops at the first one that fails: nothing more is started on a
# device that has just faulted or hung.  Differing digests end it too (exit 1), before any bench run.
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OLD=$(realpath "$1"); cd "$R"
export HSA_ENABLE_IPC_MODE_LEGACY=0
O=${AB_OUT:-build/ab}; mkdir -p $O
TRMF_CORELIB_DIR=$OLD timeout -k 10 420 python scripts/digest_run.py > $O/digest_old.txt 2>&1
timeout -k 10 420 python scripts/digest_run.py > $O/digest_new.txt 2>&1
if diff $O/digest_old.txt $O/digest_new.txt > /dev/null; then echo "DIGESTS IDENTICAL"
else echo "DIGESTS DIFFER"; diff $O/digest_old.txt $O/digest_new.txt | head || true; exit 1; fi
# iter/s over all windows, the windows' median / min / max, phase times, CG pass
rep() { timeout -k 10 400 python bench.py --full --no-cpu-baseline --no-one-shot "$@" 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); w=d['windows']; print(round(d['value'],1), {k:round(w[k],1) for k in ('iter_per_s_median','iter_per_s_min','iter_per_s_max')}, {k:round(v,4) for k,v in d['phases_ms'].items() if k in ('F','X','Theta')}, (d.get('roofline_x') or {}).get('cg',{}).get('us_per_pass'))"; }
for lib in old new old new; do
  if [ $lib = old ]; then export TRMF_CORELIB_DIR=$OLD; else unset TRMF_CORELIB_DIR; fi
  echo "== $lib c3"; rep
  echo "== $lib c2"; rep --config c2 --steps 40 --warmup 10
  echo "== $lib imp"; rep --config imp          # one launch per CG step (accept_tile_kernel, hv_tile_kernel)
  echo "== $lib imp60"; rep --config imp60      # the unfused path (ar_tile_kernel<AR_CG_STEP>, cg_init_kernel, accept_kernel)
done
