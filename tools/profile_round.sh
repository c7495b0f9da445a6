#!/bin/bash
# Round profile on the GPU box: kernel trace + stats, then separate PMC passes
# (FETCH_SIZE, WRITE_SIZE; MI355X_MICROARCH.md HBM section: never combined with tracing) of the
# same bench command, plus the all-config suite. Outputs under $PROFILE_OUT/$1/ (default: profile_out/$1/
# in the repository).
#   summarize locally: python tools/pmc_summary.py <that directory> <tag>
set -e
OUT=$1
R=$GRAFT_REPO_ROOT
D=${PROFILE_OUT:-$R/profile_out}/$OUT
mkdir -p $D
cd /tmp && export TMPDIR=/tmp
CMD="$R/bench.py --full --no-cpu-baseline"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D -o trace -- python3 $CMD > $D/bench_trace.log 2>&1
# PMC passes on the dominant-kernel loop only (counter collection serializes every dispatch;
# the whole bench under it does not finish in minutes)
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $D -o pmc_fetch -- python3 $CMD --only-dominant > $D/bench_fetch.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $D -o pmc_write -- python3 $CMD --only-dominant > $D/bench_write.log 2>&1
timeout -k 10 300 python3 $R/bench.py --full > $D/bench.json 2> $D/bench.err
timeout -k 10 600 python3 $R/tools/config_suite.py --out $D/configs.json > $D/configs.log 2>&1
