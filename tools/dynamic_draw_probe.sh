#!/bin/bash
# ON THE GPU BOX: tools/dynamic_draw_probe.py, then the two raster passes of this tree, detached and attached with the
# draw flags off, against those of a built checkout of the parent commit (PARENT=dir, optional: `make all` run in it and
# this tree's tools/dynamic_draw_probe.py copied into its tools/ -- the compat mode uses entry points the parent has),
# alternating the two processes PAIRS times.  Output: $OUT/dynamic_draw_probe.txt and $OUT/dynamic_draw_probe_compat.txt
# (default OUT: tool_out/).
set -o pipefail
HERE="$(cd "$(dirname "$0")/.." && pwd)"
export OUT="${OUT:-$HERE/tool_out}"
mkdir -p "$OUT"
: > "$OUT/dynamic_draw_probe_compat.txt"
timeout -k 10 "${PROBE_LIMIT:-420}" python "$HERE/tools/dynamic_draw_probe.py" || exit $?
if [ -n "$PARENT" ]; then
    for i in $(seq "${PAIRS:-3}"); do
        COMPAT=1 LABEL=parent timeout -k 10 120 python "$PARENT/tools/dynamic_draw_probe.py" || exit $?
        COMPAT=1 LABEL="this tree" timeout -k 10 120 python "$HERE/tools/dynamic_draw_probe.py" || exit $?
    done
fi
cat "$OUT/dynamic_draw_probe_compat.txt"
