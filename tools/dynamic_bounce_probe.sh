#!/bin/bash
# ON THE GPU BOX: tools/dynamic_bounce_probe.py; then the table kernel alone from a kernel trace of a run of its own
# (MODE=loop, if rocprofv3 is there); then the plain bounce, the resident step and bench.py of this tree against those of a
# built checkout of the parent commit (PARENT=dir, optional: `make all` run in it and this tree's
# tools/dynamic_bounce_probe.py copied into its tools/ -- the detached mode uses entry points the parent has),
# alternating the two processes PAIRS times.  Every step under its own time limit; the script ends at the first that fails.
# Output: $OUT/dynamic_bounce_probe.txt, _detached.txt, _bench.txt and _map_kernel.txt (default OUT: tool_out/).
set -o pipefail
HERE="$(cd "$(dirname "$0")/.." && pwd)"
export OUT="${OUT:-$HERE/tool_out}"
mkdir -p "$OUT"
: > "$OUT/dynamic_bounce_probe_detached.txt"
: > "$OUT/dynamic_bounce_probe_bench.txt"
timeout -k 10 "${PROBE_LIMIT:-420}" python "$HERE/tools/dynamic_bounce_probe.py" || exit $?
if command -v rocprofv3 > /dev/null; then
    rm -rf "$OUT/bounce_trace"
    MODE=loop timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/bounce_trace" -o bounce -- python "$HERE/tools/dynamic_bounce_probe.py" > /dev/null || exit $?
    grep -rh "k_bounce\|\"Name\"" "$OUT/bounce_trace" --include='*stats*.csv' > "$OUT/dynamic_bounce_probe_map_kernel.txt"
    rm -rf "$OUT/bounce_trace"
    cat "$OUT/dynamic_bounce_probe_map_kernel.txt"
fi
if [ -n "$PARENT" ]; then
    for i in $(seq "${PAIRS:-3}"); do
        MODE=detached LABEL=parent timeout -k 10 120 python "$PARENT/tools/dynamic_bounce_probe.py" || exit $?
        MODE=detached LABEL="this tree" timeout -k 10 120 python "$HERE/tools/dynamic_bounce_probe.py" || exit $?
        (cd "$PARENT" && timeout -k 10 180 python bench.py --gpus 1 --steps "${BENCH_STEPS:-200}" --warmup 20 | tail -1 | sed 's/^/parent    /') >> "$OUT/dynamic_bounce_probe_bench.txt" || exit $?
        (cd "$HERE" && timeout -k 10 180 python bench.py --gpus 1 --steps "${BENCH_STEPS:-200}" --warmup 20 | tail -1 | sed 's/^/this tree /') >> "$OUT/dynamic_bounce_probe_bench.txt" || exit $?
    done
fi
cat "$OUT/dynamic_bounce_probe_detached.txt" "$OUT/dynamic_bounce_probe_bench.txt"
