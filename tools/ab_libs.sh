#!/bin/bash
# A/B of diagnostic library builds on the bench workload: for each FBR_LIB variant, one sequential
# (FBR_NSUB=1, per-kernel times) and one default (overlapped) bench line.  usage: tools/ab_libs.sh TAG lib...
set -o pipefail
TAG=$1; shift
OUT=${OUT:-ab_out}; mkdir -p $OUT
for L in "$@"; do
  n=$(basename $L .so)
  FBR_LIB=$PWD/$L FBR_NSUB=1 timeout -k 10 200 python3 bench.py --full --batch ${BATCH:-256} --steps 4 --warmup 1 --no-cpu-baseline --profile all > $OUT/ab_${TAG}_${n}_seq.log 2>&1 || exit 31
  FBR_LIB=$PWD/$L timeout -k 10 200 python3 bench.py --full --steps 6 --warmup 2 --no-cpu-baseline > $OUT/ab_${TAG}_${n}.log 2>&1 || exit 32
done
python3 tools/ab_summary.py $OUT/ab_${TAG}_*.log
