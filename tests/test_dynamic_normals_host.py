"""CPU: the host side of the dynamic mesh's corner normals -- the argument checks and size arithmetic added to
csrc/vct_dynamic_check.h and the corner-frame arithmetic of csrc/vct_import_check.h (the very functions the prepare kernels
call) in a stand-alone program under ASan + UBSan, against literals written out by the NumPy restatement -- and what the
header, the binding, the facade and the demo say about the feature."""
import os
import re
import subprocess

import numpy as np
import pytest

import dynamic_normals_ref as nr
import dyndrawcases as ddc
import dynnormalcases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = (("vct_set_dynamic_normals", 2), ("vct_update_dynamic_normals", 3), ("vct_get_dynamic_normals", 3),
                ("vct_download_dynamic_frames", 4))
SOURCE = os.path.join(ROOT, "tests", "dynamic_normals_check_main.cpp")


def host_literals():
    """The tables of tests/dynamic_normals_check_main.cpp as text: per adversarial corner the normal, the face frame, the
    expected frame and the path; per matrix the twelve elements, a normal and the expected moved normal -- all as the bit
    patterns of the restatement's float32 values."""
    hexes = lambda a: ", ".join(f"0x{int(v):08x}u" for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))
    pos, nrm, _, _ = nc.adversarial()
    (un, ut, ub), _, why = nr.corner_frames(nr.draw_copy(pos), nr.moved_normals(nrm))
    face = ddc.dynamic_frames(pos)
    lines = ["static const CornerCase kCorners[] = {"]
    for name, t, c, _, path in nc.CORNERS:
        at = lambda a: a.reshape(-1, 3, 3)[t, c]
        assert why[t, c] == path
        lines.append(f"    {{\"{name}\", {{{hexes(nrm[t, c])}}}, {{{hexes(np.stack([at(a) for a in face]))}}},")
        lines.append(f"     {{{hexes(np.stack([at(un), at(ut), at(ub)]))}}}, {path}}},")
    lines.append("};")
    lines.append("static const MatrixCase kMatrices[] = {")
    n = np.array([[0.48, -0.6, 0.64]], np.float32)
    for name in nc.MATRICES:
        m = nc.matrix(name)
        moved = nr.moved_normals(n.reshape(1, 1, 3).repeat(3, 1), part=np.zeros(1, np.int32), m=m[None])[0, 0]
        lines.append(f"    {{\"{name}\", {{{hexes(m)}}},")
        lines.append(f"     {{{hexes(n)}}}, {{{hexes(moved)}}}}},")
    lines.append("};")
    return "\n".join(lines) + "\n"


def test_the_program_s_literals_are_the_restatement_s():
    src = open(SOURCE).read()
    assert host_literals() in src, "regenerate the tables of tests/dynamic_normals_check_main.cpp from host_literals()"


def test_normals_checks_and_corner_frames_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "dynamic_normals_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, SOURCE])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "dynamic_normals_check ok" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_header_binding_and_facade_declare_the_normals():
    import vctpkg
    vct = vctpkg.load()
    hdr = open(os.path.join(ROOT, "include", "vct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)          # (a declaration's comments hold commas and semicolons)
    for name, args in ENTRY_POINTS:
        m = re.search(r"\bint " + name + r"\(vct_ctx\* ctx([^;]*)\);", code)
        assert m, name
        assert 1 + len(m.group(1).strip(", \n").split(",")) == args, (name, m.group(1))
        assert name in vct.ABI_SYMBOLS and hasattr(vct.lib(), name), name
        assert len(getattr(vct.lib(), name).argtypes) == args
    assert int(re.search(r"#define VCT_ABI_VERSION (\d+)", hdr).group(1)) == 8        # entry points only, no struct change
    section = hdr[hdr.index("/* ---- dynamic mesh"):hdr.index("#define VCT_DYNAMIC_TRIS_MAX")]
    assert section.index("Skin (vct_set_dynamic_skin; none by default)") < section.index("Normals (vct_set_dynamic_normals; none by default)")
    assert section.index("Normals (vct_set_dynamic_normals; none by default)") < section.index("Known limits")
    for word in ("C_0 = A_1 x A_2,  C_1 = A_2 x A_0,  C_2 = A_0 x A_1", "n'_r = ((C_r.x * n.x + C_r.y * n.y) + C_r.z * n.z)",
                 "cross(A a, A b) = C cross(a, b)", "no division and no determinant test", "nothing fused",
                 "d_f = (u_c.x * u_f.x + u_c.y * u_f.y) + u_c.z * u_f.z", "if !(d_f > 0) the corner takes the face frame",
                 "k_i = t_f_i - u_c_i * d", "if t_c is all zero the corner takes the face frame",
                 "b_c = (u_c.y * t_c.z - u_c.z * t_c.y,  u_c.z * t_c.x - u_c.x * t_c.z,  u_c.x * t_c.y - u_c.y * t_c.x)",
                 "Dn stays the quantised face normal", "vct_set_dynamic_mesh drops them on attach, replace and detach",
                 "survive attaching, replacing and detaching a mover", "ANY fp32 value is accepted as a normal",
                 "Known limits: the drawn mesh has no textures, no gloss class and flat (per-face) normals unless",
                 "every kernel launched, and its argument block, is the one launched without this paragraph"):
        assert word in section, word
    L = vct.lib()
    assert L.vct_set_dynamic_normals(None, None) != 0 and L.vct_update_dynamic_normals(None, None, 0) != 0
    assert L.vct_get_dynamic_normals(None, None, None) != 0 and L.vct_download_dynamic_frames(None, None, None, None) != 0
    for method in ("set_dynamic_normals", "update_dynamic_normals", "dynamic_normals", "download_dynamic_frames"):
        assert callable(getattr(vct.Context, method)), method
    facade = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "host", "Voxel_Cone_Tracing.h")).read()
    assert re.search(r"bool SetDynamicNormals\(const float\* nrm\)", facade)
    assert re.search(r"bool UpdateDynamicNormals\(const float\* nrm, int32_t location = VCT_MEM_HOST\)", facade)
    assert re.search(r"bool DownloadDynamicFrames\(float\* nrm, float\* tan, float\* bit\)", facade)
    shared = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "csrc", "vct_import_check.h")).read()
    assert re.search(r"VCT_IMPORT_FN bool vct_import_corner_frame\(", shared) and "VCT_IMPORT_FN void vct_import_cofactor(" in shared
    kernels = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "csrc", "vct_raster.hip")).read()
    assert "vct_import_corner_frame(" in kernels and "template <DynSrc SRC = DYN_SRC_POS, bool NRM = false>" in kernels


class Stub:
    """Stands in for a context whose dynamic mesh has 150 triangles: the shape checks are the binding's own and run before
    any pointer is handed over (no GPU)."""
    _dyn_ntri = 150
    _h = None

    def _ck(self, rc, what):
        raise AssertionError("the arguments reached the library")


def test_binding_refuses_normals_of_the_wrong_shape():
    import vctpkg
    vct = vctpkg.load()
    for shape in ((149, 3, 3), (151, 3, 3), (150, 3, 4), (150, 3), (150 * 9,), (150, 8), (0, 3, 3), (1, 150, 9), (150, 9, 1)):
        for call in (vct.Context.set_dynamic_normals, vct.Context.update_dynamic_normals):
            with pytest.raises(vct.VctError) as e:
                call(Stub(), np.zeros(shape, np.float32))
            assert "150 triangles" in str(e.value), str(e.value)
    for good in ((150, 3, 3), (150, 9)):          # these reach the library
        with pytest.raises(AssertionError, match="reached the library"):
            vct.Context.set_dynamic_normals(Stub(), np.zeros(good, np.float32))


def test_the_demo_checks_dynamic_smooth_before_a_gpu_is_touched(tmp_path):
    exe = os.path.join(ROOT, "voxel-cone-tracing_amd", "vct_demo")
    assert os.path.exists(exe), "build it with `make demo`"
    obj = tmp_path / "tri.obj"
    obj.write_text("v -50 -40 10\nv 60 -30 20\nv 0 70 -10\nf 1 2 3\n")

    def run(*args):
        return subprocess.run([exe, "--voxels", "32", "--size", "32x32", "--shadow", "64", "--frames", "2", *args],
                              capture_output=True, text=True, timeout=120)
    for args, word in ((("--dynamic-smooth",), "needs --dynamic-obj"),
                       (("--dynamic-obj", str(obj), "--dynamic-smooth"), "needs --dynamic-draw gbuffer|both"),
                       (("--dynamic-obj", str(obj), "--dynamic-draw", "shadow", "--dynamic-smooth"), "needs --dynamic-draw gbuffer|both"),
                       (("--dynamic-smooth", "--dynamic-obj", str(obj), "--dynamic-spin", "0,0,1;5"), "needs --dynamic-draw gbuffer|both")):
        out = run(*args)
        assert out.returncode == 1 and word in out.stderr, (args, out.returncode, out.stdout[-500:], out.stderr[-500:])
        assert "--dynamic-smooth" in out.stderr and "the OBJ's vertex normals" in out.stderr
    opts = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "host", "vct_demo_options.h")).read()
    assert "VCT_DEMO_DYNAMIC_SMOOTH_USAGE" in opts and "vct_demo_check_dynamic_smooth" in opts
