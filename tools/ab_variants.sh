#!/bin/bash
# Run bench.py once per variant library (build/variants/lib_<name>.so; "base" = in-tree lib).
# Usage: tools/ab_variants.sh TAG "bench args" name...   (results under ${E2SAR_OUT:-bench_out}/TAG)
set -e
TAG=$1; ARGS=$2; shift 2
O=${E2SAR_OUT:-bench_out}/$TAG
mkdir -p $O
for v in "$@"; do
  if [ "$v" = base ]; then L=$GRAFT_REPO_ROOT/e2sar_amd/lib/libe2sar_hip.so; else L=$GRAFT_REPO_ROOT/build/variants/lib_$v.so; fi
  E2SAR_HIP_LIB=$L timeout -k 10 200 python bench.py --full --cpu-seconds 0 $ARGS > $O/$v.json 2> $O/$v.err
done
