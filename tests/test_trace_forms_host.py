"""CPU: the launch plan and the table of kernel forms of csrc/vct_trace_forms.h -- every combination of the facts of a launch
(5 variants x 12 flags x 4 row shapes) against the dispatch of csrc/vct_trace.hip before the header existed, restated
literally in tests/trace_forms_check_main.cpp: same refusal, same kernel family and form, same FASTDIV, same march_form
word; every planned form is in the table, every table entry is planned, GL_REPEAT-only entries never in clamp mode, and
the table gives the 82 k_trace_tile_split kernels of the code object -- in a stand-alone program under ASan + UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voxel-cone-tracing_amd", "csrc")


def test_launch_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "trace_forms_check")
    src = os.path.join(ROOT, "tests", "trace_forms_check_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"trace_forms_check ok: (\d+) cases, (\d+) refused, 23 forms \(17 in clamp mode\), 82 kernels", out.stdout)
    assert m, out.stdout[-2000:]
    assert int(m.group(1)) == 5 * 2 ** 12 * 4 and 0 < int(m.group(2)) < int(m.group(1))
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_header_is_free_of_hip_calls_and_the_kernels_name_their_flags():
    hdr = open(os.path.join(CSRC, "vct_trace_forms.h")).read()
    assert "hip/" not in hdr and not re.search(r"\bhip[A-Z]\w*\(", hdr) and "__global__" not in hdr
    src = open(os.path.join(CSRC, "vct_trace.hip")).read()
    assert "vct_plan_launch(" in src and "kVctSplitForms[" in src
    # no template argument list of a kernel, a march or a level sample with a positional true / false
    for name in ("k_trace_tile_split", "cone_march", "sample_level", "sample_level_reuse", "sample_step_level"):
        for m in re.finditer(r"\b%s<([^;{]*?)>\s*[(),]" % name, src):
            assert not re.search(r"\b(true|false)\b", m.group(1)), m.group(0)
