#!/bin/bash
# usage: kt.sh variant
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
export VOGE_HIP_LIB=$ROOT/build/variants/$1.so
OUT=build/prof_$1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-graph > /dev/null 2>&1
echo "== $1"; python tools/rocprof_summary.py $OUT | cut -c1-150 | grep -E "bin|trace_fwd|prep|tile_order"
