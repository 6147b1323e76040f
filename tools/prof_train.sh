set -o pipefail
OUT=${OUT:-bench_out}  # output folder, relative to the repository root
ROOT=$GRAFT_REPO_ROOT
mkdir -p $ROOT/$OUT
export TMPDIR=/tmp
cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_tr -o run -- python3 $ROOT/bench.py --full --no-c5 --steps 20 --warmup 2 --no-cpu-baseline --no-pmc --no-train-ff --no-train-ref --train-steps 4 --train-warmup 1 > $ROOT/$OUT/prof_tr.log 2>&1
