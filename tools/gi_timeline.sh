cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/tool_out}; mkdir -p "$OUT"     # output folder (git-ignored default)
rocprofv3 --kernel-trace --output-format csv -d $OUT/gitl -- python3 $R/bench.py --full --cpu-seconds 0 --no-sweep --steps 5 --warmup 2 --frames-in-flight 1 --no-two-slots > /dev/null 2>&1
f=$(find $OUT/gitl -name "*kernel_trace.csv" | head -1)
python3 $R/tools/gi_timeline.py $f
