#!/bin/bash
# On the GPU box: per-kernel durations of the bench frame of a config (eager launches).  usage: tools/cfg_ktrace.sh [config] [extra bench flags]
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
CFG=${1:-cfg4_200k_1024}; shift
OUT=build/prof_cfg
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-graph --no-variants --config $CFG "$@" > /dev/null 2>&1
python tools/rocprof_summary.py $OUT | cut -c1-70,100-150 | head -${LINES_OUT:-22}
rm -rf $OUT
