#!/bin/bash
# A/B helper: runs the short bench once per environment setting given as arguments ("VAR=1 VAR2=x" strings, "" = default)
# and prints step time + serialized stage times.  Usage: bash tools/ab.sh tag "" "MSLAM_X=1" ...; the bench lines are kept
# under $BENCH_OUT/<tag>/ (default bench_out/).
TAG=$1; shift
OUT=${BENCH_OUT:-bench_out}/$TAG
mkdir -p "$OUT"
i=0
for cfg in "$@"; do
  env $cfg timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-legs --steps 30 ${BENCH_ARGS:-} > "$OUT/ab_$i.json" 2> "$OUT/ab_$i.err" || { echo "FAILED: $cfg"; tail -3 "$OUT/ab_$i.err"; exit 1; }
  python - "$OUT/ab_$i.json" "$cfg" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
r = d["roofline"]
s = r.get("stages_ms_serialized", {})
print("[%s] %.1f M kp/s, %.3f ms/step | alone: %s" % (sys.argv[2], d["value"] / 1e6, d["ms_per_step"], " ".join("%s %.3f" % (k, v) for k, v in s.items())))
PY
  i=$((i+1))
done
