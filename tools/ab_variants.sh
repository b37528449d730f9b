#!/bin/bash
# A/B of experiment builds of the library (hmse_amd/csrc/Makefile: libhmse_hip_<tag>.so): bash tools/ab_variants.sh <bytes> <tag> [<tag> ...]
# ("base" = the product library).  Prints the per-stage sums of bench.py for every variant.
# A variant that fails ENDS the script with a non-zero status — nothing more is started on a GPU that has just faulted; on a shared
# machine call it with one variant per invocation and chain the invocations with &&.
BYTES=$1; shift
OUT=${OUT:-runs}; mkdir -p $OUT
for V in "$@"; do
  if [ "$V" = base ]; then unset HMSE_LIB_VARIANT; else export HMSE_LIB_VARIANT=$V; fi
  HMSE_BENCH_NO_VERIFY=1 HMSE_BENCH_NO_MANIFEST=1 timeout -k 5 300 python bench.py --full --bytes $BYTES --steps 3 --warmup 1 --no-cpu-baseline --no-other-configs > $OUT/ab_$V.json 2> $OUT/ab_$V.err || { echo "$V FAILED"; tail -3 $OUT/ab_$V.err; exit 1; }
  python - <<PY || exit 1
import json
d=json.load(open("$OUT/ab_$V.json")); sr=d["stage_roofline"]
g=lambda pre,suf: sum(v["avg_ms"] for k,v in sr.items() if k.startswith(pre) and k.endswith(suf))
print("%-8s step %.1f ms  cf %.4f | plain %.1f dict %.1f encode %.1f minhash %.1f | " % ("$V", d["ms_per_step"], d["cf"], g("l1_deflate_kernel","false>"), g("l1_deflate_kernel","true>"), sum(v["avg_ms"] for k,v in sr.items() if k.startswith("l1_encode")), g("l4_minhash","")) + " ".join("%.1f" % v["avg_ms"] for k,v in sorted(sr.items(), key=lambda kv:-kv[1]["avg_ms"])[:6]))
PY
done
