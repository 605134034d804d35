#!/bin/bash
# ON THE GPU BOX: tools/lights_probe.py, then the detached resident step of this tree against the same step of a built
# checkout of the parent commit (PARENT=dir, optional: `make all` run in it and this tree's tools/lights_probe.py copied
# into its tools/ -- the step-only mode uses entry points the parent has), alternating the two processes PAIRS times.
# Output: $OUT/lights_probe.txt and $OUT/lights_probe_step.txt (default OUT: tool_out/).
set -o pipefail
HERE="$(cd "$(dirname "$0")/.." && pwd)"
export OUT="${OUT:-$HERE/tool_out}"
mkdir -p "$OUT"
: > "$OUT/lights_probe_step.txt"
timeout -k 10 "${PROBE_LIMIT:-420}" python "$HERE/tools/lights_probe.py" || exit $?
if [ -n "$PARENT" ]; then
    for i in $(seq "${PAIRS:-3}"); do
        STEP_ONLY=1 LABEL=parent timeout -k 10 120 python "$PARENT/tools/lights_probe.py" || exit $?
        STEP_ONLY=1 LABEL="this tree" timeout -k 10 120 python "$HERE/tools/lights_probe.py" || exit $?
    done
fi
cat "$OUT/lights_probe_step.txt"
