#!/bin/bash
# end-of-session check: smoke + full GPU suite, headline bench + rocprof evidence (TAG), the
# 8-GPU-shard-size line and the config-3 line
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}; mkdir -p $OUT
TAG=${TAG:-r02t} PROFILE=1 bash scripts/gpu_verify.sh || exit $?
out=$OUT/extra_lines.jsonl
: > $out
timeout -k 10 300 python -u bench.py --full --rows 1250000 --steps 300 --warmup 10 --no-cpu >> $out 2> $OUT/extra.err || { rc=$?; tail -20 $OUT/extra.err; exit $rc; }
cut -c1-300 $out
CONFIGS=3 bash scripts/gpu_lines.sh
