#!/bin/bash
# rocprofv3 evidence for the bench: (1) kernel trace + stats, (2) a separate PMC pass for
# HBM bytes (FETCH_SIZE), then summaries under $OUT/profiles (OUT: a directory relative to the
# repository root, default bench_out).
# Usage on the GPU box: TAG=r01 bash scripts/profile.sh; then: cp $OUT/profiles/* profiles/
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
R=$(pwd)
TAG=${TAG:-r01}
OUT=${OUT:-bench_out}; mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python -u bench.py --full > $OUT/bench_full.log 2>&1 || { rc=$?; tail -20 $OUT/bench_full.log; exit $rc; }
tail -1 $OUT/bench_full.log
rm -rf $OUT/prof_trace $OUT/prof_pmc
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/prof_trace" -o trace \
    -- python3 "$R/bench.py" --steps 50 --warmup 20 --no-recall --no-cpu --no-configs > $OUT/prof_trace.log 2>&1 || { rc=$?; tail -20 $OUT/prof_trace.log; exit $rc; }
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$R/$OUT/prof_pmc" -o pmc \
    -- python3 "$R/bench.py" --steps 10 --warmup 2 --no-recall --no-cpu --no-configs > $OUT/prof_pmc.log 2>&1 || { rc=$?; tail -20 $OUT/prof_pmc.log; exit $rc; }
# summaries land in $OUT/profiles; copy them into profiles/ to commit them
PROFILES_DIR=$OUT/profiles python scripts/summarize_prof.py "$TAG" $OUT/prof_trace $OUT/prof_pmc $OUT/bench_full.log
