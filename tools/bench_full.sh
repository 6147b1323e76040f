#!/bin/bash
# The default bench line (all legs) and the rocprofv3 kernel summary of the same command.
# Usage on the GPU box: bash tools/bench_full.sh TAG -> $OUT/bench_TAG.log,
# $OUT/prof_TAG/run_kernel_stats.csv
set -o pipefail
OUT=${OUT:-bench_out}  # output folder, relative to the repository root
ROOT=$GRAFT_REPO_ROOT
mkdir -p $ROOT/$OUT
TAG=${1:?tag}
export TMPDIR=/tmp
cd $ROOT && timeout -k 10 500 python3 bench.py --full --no-c5 > $OUT/bench_$TAG.log 2>&1 || exit $?
cd /tmp && timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_$TAG -o run \
  -- python3 $ROOT/bench.py --full --no-c5 --no-pmc --no-cpu-baseline > $ROOT/$OUT/prof_$TAG.log 2>&1
