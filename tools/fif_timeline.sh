#!/bin/bash
# ON THE GPU BOX: kernel trace of the default bench line (two frames in flight) -> $OUT/fif_timeline.txt
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/tool_out}; mkdir -p "$OUT"     # output folder (git-ignored default)
rocprofv3 --kernel-trace --output-format csv -d $OUT/fiftl -- python3 $R/bench.py --full --cpu-seconds 0 --no-sweep --steps 40 --warmup 5 > /dev/null 2>&1
f=$(find $OUT/fiftl -name "*kernel_trace.csv" | head -1)
python3 $R/tools/fif_timeline.py $f 40 | tee $OUT/fif_timeline.txt
python3 $R/tools/fif_timeline.py $f 40 > /dev/null
