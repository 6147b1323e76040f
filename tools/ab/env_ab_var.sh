#!/bin/bash
# A/B of an environment-variable switch on the training legs: VAR=value vs unset, alternating.
set -o pipefail
OUT=${OUT:-bench_out}  # output folder, relative to the repository root
cd ${GRAFT_REPO_ROOT:-/root/repo}
mkdir -p $OUT
REF="--no-train-ref"; [ "${TRAIN_REF:-0}" = "1" ] && REF=""
for r in ${ROUNDS:-1 2}; do
  for v in on off; do
    if [ $v = on ]; then E="$VAR"; else E="VN_UNUSED=0"; fi
    env $E timeout -k 10 300 python3 bench.py --full --no-c5 --steps 20 --warmup 5 --no-cpu-baseline --no-pmc $REF > $OUT/vab_$v$r.log 2>&1 || exit 1
    echo "$v $r $(grep -o '"ms_per_update": [0-9.]*' $OUT/vab_$v$r.log | tr '\n' ' ')"
  done
done
