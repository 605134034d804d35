"""CPU: the host side of vct_set_dynamic_emission -- the table check and the size arithmetic it adds to
csrc/vct_dynamic_check.h in a stand-alone program under ASan + UBSan -- and what the header, the binding, the facade and
the demo say about it."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emission_checks_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "dynamic_emission_check")
    src = os.path.join(ROOT, "tests", "dynamic_emission_check_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "dynamic_emission_check ok" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_header_binding_and_facade_declare_the_emission_table():
    import vctpkg
    vct = vctpkg.load()
    hdr = open(os.path.join(ROOT, "include", "vct.h")).read()
    for name, args in (("vct_set_dynamic_emission", 2), ("vct_get_dynamic_emission", 3)):
        m = re.search(r"\bint " + name + r"\(vct_ctx\* ctx([^;]*)\);", hdr)
        assert m, name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == args, (name, m.group(1))
        assert name in vct.ABI_SYMBOLS and hasattr(vct.lib(), name), name
        assert len(getattr(vct.lib(), name).argtypes) == args
    assert int(re.search(r"#define VCT_ABI_VERSION (\d+)", hdr).group(1)) == 8        # new entry points, no struct change
    for word in ("NO textures and NO emission of its own until vct_set_dynamic_emission attaches a table",
                 "D'.rgb = min(255, D.rgb + DEm.rgb)", "level0 = D.a > 0 ? D' : S'", "8 KiB per brick slot",
                 "carries the table that was attached when its vct_voxelize was issued",
                 "the static table (zeros where none is attached) followed by the dynamic",
                 "Known limits: the drawn mesh has no textures, no gloss class and flat (per-face) normals"):
        assert word in hdr, word
    assert "no textures, no emission, no gloss class" not in hdr       # the limit the table lifts is no longer claimed
    L = vct.lib()
    assert L.vct_set_dynamic_emission(None, None) != 0
    assert L.vct_get_dynamic_emission(None, None, None) != 0
    for method in ("set_dynamic_emission", "dynamic_emission"):
        assert callable(getattr(vct.Context, method))
    facade = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "host", "Voxel_Cone_Tracing.h")).read()
    assert re.search(r"bool SetDynamicEmission\(const float\* table, size_t materials\)", facade)
    # re-applied behind SetDynamicMesh: the mesh drops the table
    body = facade[facade.index("bool SetDynamicMesh("):facade.index("bool UpdateDynamicMesh(")]
    assert body.index("vct_set_dynamic_mesh(") < body.index("vct_set_dynamic_emission(")


def test_binding_refuses_a_table_of_the_wrong_shape():
    """Context.set_dynamic_emission checks the shape against the attached mesh's materials before any pointer is handed
    over (no GPU: the check is the binding's, exercised on an object that stands in for a context whose dynamic mesh has
    three materials)."""
    import vctpkg
    vct = vctpkg.load()

    class Stub:
        _dyn_nmat = 3
        _h = None

        def _ck(self, rc, what):
            raise AssertionError("the table reached the library")
    for shape in ((2, 3), (4, 3), (3, 4), (9,), (1, 3, 3)):
        with pytest.raises(vct.VctError) as e:
            vct.Context.set_dynamic_emission(Stub(), np.zeros(shape, np.float32))
        assert "3 materials" in str(e.value), str(e.value)
    src = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "__init__.py")).read()
    assert "self._dyn_nmat = albedo.shape[0]" in src


def test_the_demo_checks_dynamic_emission_before_a_gpu_is_touched(tmp_path):
    exe = os.path.join(ROOT, "voxel-cone-tracing_amd", "vct_demo")
    assert os.path.exists(exe), "build it with `make demo`"
    obj = tmp_path / "tri.obj"
    obj.write_text("v -50 -40 10\nv 60 -30 20\nv 0 70 -10\nf 1 2 3\n")

    def run(*args):
        return subprocess.run([exe, "--voxels", "32", "--size", "32x32", "--shadow", "64", "--frames", "2", *args],
                              capture_output=True, text=True, timeout=120)
    for args, word in ((("--dynamic-emission", "0=1,1,1"), "needs --dynamic-obj"),
                       (("--dynamic-obj", str(obj), "--dynamic-emission", "0=1,nan,1"), "finite values >= 0"),
                       (("--dynamic-obj", str(obj), "--dynamic-emission", "0=1,inf,1"), "finite values >= 0"),
                       (("--dynamic-obj", str(obj), "--dynamic-emission", "0=1,-0.5,1"), "finite values >= 0"),
                       (("--dynamic-obj", str(obj), "--dynamic-emission", "0=1,1"), "MATERIAL=R,G,B"),
                       (("--dynamic-obj", str(obj), "--dynamic-emission", "0=1,1,1;"), "MATERIAL=R,G,B"),
                       (("--dynamic-obj", str(obj), "--dynamic-emission", "5=1,1,1"), "the OBJ has 1 materials")):
        out = run(*args)
        assert out.returncode == 1 and word in out.stderr, (args, out.returncode, out.stdout[-500:], out.stderr[-500:])
    opts = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "host", "vct_demo_options.h")).read()
    assert "VCT_DEMO_DYNAMIC_EMISSION_USAGE" in opts
