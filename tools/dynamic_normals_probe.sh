#!/bin/bash
# ON THE GPU BOX: tools/dynamic_normals_probe.py, then -- PARENT=dir, a built checkout of the parent commit (`make lib host`
# run in it; this tree's tools/dynamic_normals_probe.py is copied into its tools/, its BASELINE_ONLY mode uses entry points
# the parent has) -- the shadow stage, the G-buffer stage and the resident step, detached and attached without normals, and
# bench.py's line, of the parent against this tree, the two processes alternating PAIRS times.
# Output: $OUT/dynamic_normals_probe.txt with the baseline and benchmark lines appended (default OUT: tool_out/).
set -o pipefail
HERE="$(cd "$(dirname "$0")/.." && pwd)"
export OUT="${OUT:-$HERE/tool_out}"
mkdir -p "$OUT"
: > "$OUT/dynamic_normals_baseline.txt"
if [ -z "$SKIP_PROBE" ]; then
    timeout -k 10 "${PROBE_LIMIT:-420}" python "$HERE/tools/dynamic_normals_probe.py" || exit $?
fi
if [ -n "$PARENT" ]; then
    cp "$HERE/tools/dynamic_normals_probe.py" "$PARENT/tools/dynamic_normals_probe.py" || exit $?
    for i in $(seq "${PAIRS:-3}"); do
        BASELINE_ONLY=1 LABEL=parent timeout -k 10 150 python "$PARENT/tools/dynamic_normals_probe.py" || exit $?
        BASELINE_ONLY=1 LABEL="this tree" timeout -k 10 150 python "$HERE/tools/dynamic_normals_probe.py" || exit $?
    done
    for i in $(seq "${PAIRS:-3}"); do
        for tree in "$PARENT" "$HERE"; do
            line="$(cd "$tree" && timeout -k 10 150 python bench.py --gpus 1 --steps "${BENCH_STEPS:-200}" --warmup 20 | tail -1)" || exit $?
            echo "bench.py in $([ "$tree" = "$HERE" ] && echo 'this tree' || echo parent): $(echo "$line" | grep -o '"ms_per_step": [0-9.]*')" >> "$OUT/dynamic_normals_baseline.txt"
        done
    done
    [ -f "$OUT/dynamic_normals_probe.txt" ] && cat "$OUT/dynamic_normals_baseline.txt" >> "$OUT/dynamic_normals_probe.txt"
fi
cat "$OUT/dynamic_normals_probe.txt" 2>/dev/null || cat "$OUT/dynamic_normals_baseline.txt"
