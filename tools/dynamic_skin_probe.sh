#!/bin/bash
# ON THE GPU BOX: tools/dynamic_skin_probe.py, then the detached pass and the resident step of this tree against those of a
# built checkout of the parent commit (PARENT=dir, optional: `make all` run in it and this tree's tools/dynamic_probe.py
# copied into its tools/ -- the detached mode uses entry points the parent has), alternating the two processes PAIRS times.
# Output: $OUT/dynamic_skin_probe.txt, the detached lines appended (default OUT: tool_out/).
set -o pipefail
HERE="$(cd "$(dirname "$0")/.." && pwd)"
export OUT="${OUT:-$HERE/tool_out}"
mkdir -p "$OUT"
: > "$OUT/dynamic_probe_detached.txt"
timeout -k 10 "${PROBE_LIMIT:-420}" python "$HERE/tools/dynamic_skin_probe.py" || exit $?
if [ -n "$PARENT" ]; then
    for i in $(seq "${PAIRS:-3}"); do
        DETACHED_ONLY=1 LABEL=parent timeout -k 10 120 python "$PARENT/tools/dynamic_probe.py" || exit $?
        DETACHED_ONLY=1 LABEL="this tree" timeout -k 10 120 python "$HERE/tools/dynamic_probe.py" || exit $?
    done
    cat "$OUT/dynamic_probe_detached.txt" >> "$OUT/dynamic_skin_probe.txt"
fi
cat "$OUT/dynamic_skin_probe.txt"
