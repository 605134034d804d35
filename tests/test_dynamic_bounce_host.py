"""CPU: the host side of the second bounce over the dynamic mesh (vct_set_dynamic_bounce) -- what it added to
csrc/vct_dynamic_check.h in a stand-alone program under ASan + UBSan, the header / export / binding triple of the two
entry points, and the demo's option errors, raised before a GPU is touched."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bounce_arithmetic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "dynamic_bounce_check")
    src = os.path.join(ROOT, "tests", "dynamic_bounce_check_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "dynamic_bounce_check ok" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_the_header_declares_the_switch():
    import vctpkg
    vct = vctpkg.load()
    hdr = open(os.path.join(ROOT, "include", "vct.h")).read()
    assert re.search(r"\bint vct_set_dynamic_bounce\(vct_ctx\* ctx, int32_t on\);", hdr)
    assert re.search(r"\bint vct_get_dynamic_bounce\(vct_ctx\* ctx, int32_t\* on\);", hdr)
    for name in ("vct_set_dynamic_bounce", "vct_get_dynamic_bounce"):
        assert name in vct.ABI_SYMBOLS and hasattr(vct.lib(), name), name
    assert hasattr(vct.Context, "set_dynamic_bounce") and isinstance(vct.Context.dynamic_bounce, property)
    # the definition is in the dynamic-mesh section, and the sentences that called it a follow-up are gone
    section = hdr[hdr.index("dynamic mesh wins per voxel"): hdr.index("#define VCT_DYNAMIC_TRIS_MAX")]
    for word in ("vct_set_dynamic_bounce", "where(D.a > 0, Da, Sa)", "where(D.a > 0, Dn, Sn)", "merged", "Capacity", "Known limits"):
        assert word in section, word
    assert "NO textures and NO emission" in hdr
    assert "follow-up" not in section
    L = vct.lib()
    assert L.vct_set_dynamic_bounce(None, 1) != 0
    assert L.vct_get_dynamic_bounce(None, None) != 0


def test_the_demo_checks_dynamic_bounce_before_a_gpu_is_touched(tmp_path):
    exe = os.path.join(ROOT, "voxel-cone-tracing_amd", "vct_demo")
    assert os.path.exists(exe), "build it with `make demo`"
    obj = tmp_path / "tri.obj"
    obj.write_text("v -50 -40 10\nv 60 -30 20\nv 0 70 -10\nf 1 2 3\n")

    def run(*args):
        return subprocess.run([exe, "--voxels", "32", "--size", "32x32", "--shadow", "64", "--frames", "2", *args],
                              capture_output=True, text=True, timeout=120)
    for args, word in ((("--dynamic-bounce",), "needs --dynamic-obj"),
                       (("--dynamic-bounce", "--bounces", "2"), "needs --dynamic-obj"),
                       (("--dynamic-obj", str(obj), "--dynamic-bounce", "--bounces", "2", "--gpus", "2", "--rank", "0", "--idfile",
                         str(tmp_path / "id")), "not with --gpus"),
                       (("--dynamic-obj", str(obj), "--bounces", "2"), "not with"),
                       (("--dynamic-obj", str(tmp_path / "missing.obj"), "--bounces", "2", "--dynamic-bounce"), "cannot load")):
        out = run(*args)
        assert out.returncode == 1 and word in out.stderr, (args, out.returncode, out.stdout[-500:], out.stderr[-500:])
