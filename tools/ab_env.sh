#!/bin/bash
# Run bench.py once per environment setting.  Usage: tools/ab_env.sh TAG "bench args" "NAME:VAR=V,VAR=V" ...
# (a setting with no VAR after the colon runs the default build and environment;
# results under ${E2SAR_OUT:-bench_out}/TAG)
set -e
TAG=$1; ARGS=$2; shift 2
O=${E2SAR_OUT:-bench_out}/$TAG
mkdir -p $O
for spec in "$@"; do
  name=${spec%%:*}; vars=${spec#*:}
  env $(echo "$vars" | tr ',' ' ') timeout -k 10 200 python bench.py --full --cpu-seconds 0 $ARGS > $O/$name.json 2> $O/$name.err
done
for spec in "$@"; do
  name=${spec%%:*}
  python - $O/$name.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
c = d.get("reas_cold") or {}
print(sys.argv[1].split("/")[-1], d["value"], d["roofline"]["avg_launch_ms"], c.get("value"), (c.get("roofline") or {}).get("all_launch_ms"))
PY
done
