#!/bin/bash
# ON THE GPU BOX: tools/dynamic_probe.py, then the detached pass and resident step of this tree against those of a built
# checkout of the parent commit (PARENT=dir, optional: `make all` run in it and this tree's tools/dynamic_probe.py copied
# into its tools/ -- the detached mode uses entry points the parent has), alternating the two processes PAIRS times.
# With PARENT the parent's checkout also runs the probe itself (no table lines: it has no vct_set_dynamic_emission; no
# re-upload routes), so that its dynamic kernels without a table stand beside this tree's: $OUT/dynamic_probe_parent.txt.
# PARTS_ONLY=1: instead of the probe itself its parts route (PARTS=1: host and device positions against
# vct_update_dynamic_transforms with 1 and 64 parts) -- $OUT/dynamic_parts_probe.txt, with PARENT also the parent's two
# positions routes, appended to the same file -- and then the detached pairs as above.
# Output: $OUT/dynamic_probe.txt and $OUT/dynamic_probe_detached.txt (default OUT: tool_out/).
set -o pipefail
HERE="$(cd "$(dirname "$0")/.." && pwd)"
export OUT="${OUT:-$HERE/tool_out}"
mkdir -p "$OUT"
: > "$OUT/dynamic_probe_detached.txt"
if [ "$PARTS_ONLY" = 1 ]; then
    export ROUNDS="${ROUNDS:-7}"
    PARTS=1 timeout -k 10 "${PROBE_LIMIT:-420}" python "$HERE/tools/dynamic_probe.py" || exit $?
    if [ -n "$PARENT" ]; then
        PARTS=1 PARTS_FILE=dynamic_parts_probe_parent.txt LABEL=parent timeout -k 10 "${PROBE_LIMIT:-420}" python "$PARENT/tools/dynamic_probe.py" || exit $?
        cat "$OUT/dynamic_parts_probe_parent.txt" >> "$OUT/dynamic_parts_probe.txt"
        for i in $(seq "${PAIRS:-3}"); do
            DETACHED_ONLY=1 LABEL=parent timeout -k 10 120 python "$PARENT/tools/dynamic_probe.py" || exit $?
            DETACHED_ONLY=1 LABEL="this tree" timeout -k 10 120 python "$HERE/tools/dynamic_probe.py" || exit $?
        done
        cat "$OUT/dynamic_probe_detached.txt" >> "$OUT/dynamic_parts_probe.txt"
    fi
    cat "$OUT/dynamic_parts_probe.txt"
    exit 0
fi
timeout -k 10 "${PROBE_LIMIT:-420}" python "$HERE/tools/dynamic_probe.py" || exit $?
if [ -n "$PARENT" ]; then
    cp "$OUT/dynamic_probe.txt" "$OUT/dynamic_probe_this_tree.txt"
    NO_REUPLOAD=1 timeout -k 10 "${PROBE_LIMIT:-420}" python "$PARENT/tools/dynamic_probe.py" || exit $?
    mv "$OUT/dynamic_probe.txt" "$OUT/dynamic_probe_parent.txt"
    mv "$OUT/dynamic_probe_this_tree.txt" "$OUT/dynamic_probe.txt"
    for i in $(seq "${PAIRS:-3}"); do
        DETACHED_ONLY=1 LABEL=parent timeout -k 10 120 python "$PARENT/tools/dynamic_probe.py" || exit $?
        DETACHED_ONLY=1 LABEL="this tree" timeout -k 10 120 python "$HERE/tools/dynamic_probe.py" || exit $?
    done
fi
cat "$OUT/dynamic_probe_detached.txt"
