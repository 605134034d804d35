"""CPU: the emissive materials of include/vct.h ("emissive materials") without a GPU -- that the expected values of
tests/emission_ref.py are not degenerate for the inputs the GPU tests use, that zero emission is the plain level 0, the
saturating byte add of the resolve restated on every pair of bytes, Ke through the OBJ / MTL reader and the scene cache
(old caches included), the header against the binding, and the table check of vct_upload_emission in a stand-alone
program under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emission_ref as er
import voxcases
from test_gpu_parity import light_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_random_scene_expectation_is_not_degenerate(oracle):
    V = 32
    pos, mat, alb = voxcases.random_scene(300, 7)
    depth, vp = light_setup(64, 3)
    p = oracle.default_params(V)
    want, L, Em = er.level0(oracle, p, pos, mat, alb, er.EMISSION, shadow_depth=depth, light_vp=vp)
    n = er.non_degeneracy(L, Em, er.EMISSION)
    assert n["same_alpha"], "L and Em must cover the same voxels"
    assert n["saturating"] >= 50 and n["both"] >= 50 and n["mixed_values"] >= 1, n
    # a fractional shadow term in a good part of the lit voxels: L is not just albedo or 0
    unshadowed = oracle.voxelize_conservative(p, oracle.make_scene(pos, mat, alb))
    lit = L[..., 3] > 0
    frac = ((L[..., :3] != unshadowed[..., :3]).any(-1) & (L[..., :3] > 0).any(-1) & lit).sum() / lit.sum()
    assert frac > 0.1, frac
    assert (want[..., 3] == L[..., 3]).all() and (want[..., :3] >= L[..., :3]).all() and (want[..., :3] >= Em[..., :3]).all()
    assert (want[~lit] == 0).all()


def test_crowded_brick_expectation_is_not_degenerate(oracle):
    pos, mat, alb, ms, G, V = voxcases.whole_grid_and_a_crowded_brick()
    depth, vp = light_setup(64, 3)
    _, L, Em = er.level0(oracle, oracle.default_params(V, G=G), pos, mat, alb, er.EMISSION, ms, shadow_depth=depth, light_vp=vp)
    n = er.non_degeneracy(L, Em, er.EMISSION)
    assert n["same_alpha"] and n["saturating"] >= 50 and n["both"] >= 50 and n["mixed_values"] >= 1, n


def test_zero_emission_is_the_plain_level0(oracle):
    V = 32
    pos, mat, alb = voxcases.random_scene(300, 7)
    depth, vp = light_setup(64, 3)
    want, L, Em = er.level0(oracle, oracle.default_params(V), pos, mat, alb, np.zeros((5, 3), np.float32),
                            shadow_depth=depth, light_vp=vp)
    assert np.array_equal(want, L) and not Em[..., :3].any() and np.array_equal(Em[..., 3], L[..., 3])
    # ... and a map that shadows everything leaves the emission term alone
    dark, _, Em2 = er.level0(oracle, oracle.default_params(V), pos, mat, alb, er.EMISSION,
                             shadow_depth=np.zeros((64, 64), np.float32), light_vp=vp)
    assert np.array_equal(dark, Em2) and Em2[..., :3].any()


def add_sat_rgba8(a, b):
    """csrc/vct_voxelize.hip add_sat_rgba8, operation for operation, on uint32 arrays."""
    a, b = a.astype(np.uint32), b.astype(np.uint32)
    m, one = np.uint32(0x00ff00ff), np.uint32(0x00010001)
    even = (a & m) + (b & m)
    odd = ((a >> np.uint32(8)) & m) + ((b >> np.uint32(8)) & m)
    even_s = (even | (((even >> np.uint32(8)) & one) * np.uint32(0xff))) & m
    odd_s = (odd | (((odd >> np.uint32(8)) & one) * np.uint32(0xff))) & m
    return even_s | (odd_s << np.uint32(8))


def test_saturating_byte_add_on_every_pair_of_bytes():
    x, y = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
    want = np.minimum(255, x + y)
    r = np.random.default_rng(1)
    for lane in range(4):
        # the pair in one lane, random bytes in the others: no carry may cross a lane
        a = r.integers(0, 2 ** 32, x.shape, dtype=np.uint64).astype(np.uint32)
        b = r.integers(0, 2 ** 32, x.shape, dtype=np.uint64).astype(np.uint32)
        sh = np.uint32(8 * lane)
        keep = ~(np.uint32(0xff) << sh)
        a, b = (a & keep) | (x << sh), (b & keep) | (y << sh)
        got = add_sat_rgba8(a, b)
        for k in range(4):
            s = np.uint32(8 * k)
            exp = np.minimum(255, ((a >> s) & np.uint32(0xff)).astype(np.int64) + ((b >> s) & np.uint32(0xff)).astype(np.int64))
            assert np.array_equal(((got >> s) & np.uint32(0xff)).astype(np.int64), exp), (lane, k)
        assert np.array_equal((got >> sh) & np.uint32(0xff), want)


OBJ = ("mtllib lamps.mtl\nv -500 -400 100\nv 600 -300 200\nv 0 700 -100\nv -300 -200 -50\nv 400 -100 60\nv 100 500 30\n"
       "v 0 0 0\nv 100 0 0\nv 0 100 0\nusemtl wall\nf 1 2 3\nusemtl lamp\nf 4 5 6\nusemtl screen\nf 7 8 9\n")
MTL = ("newmtl wall\nKd 0.5 0.5 0.5\nKs 0.3 0.0 0.0\n"
       "newmtl lamp\nKd 0.9 0.9 0.9\nKe 1.5 0.75 0.25\nKs 0.2 0.4 0.6\n"
       "newmtl screen\n  Ke 0 0.125 2\nKd 0.1 0.2 0.3\n")


def _scene_lib():
    import vctpkg
    vctpkg.load()
    from voxel_cone_tracing_amd import scene as sc
    return sc


def test_mtl_ke_is_read(tmp_path):
    sc = _scene_lib()
    (tmp_path / "lamps.mtl").write_text(MTL)
    (tmp_path / "lamps.obj").write_text(OBJ)
    s = sc.Scene(str(tmp_path / "lamps.obj"))
    assert s.ntri == 3 and s.nmat == 3
    # straight through the C entry point, into a buffer of exactly nmat * 3 floats
    lib = C.CDLL(sc.LIB_PATH)
    lib.vcth_scene_get_emission.argtypes = [C.c_void_p, C.c_void_p]
    em = np.full((3, 3), -1.0, np.float32)
    lib.vcth_scene_get_emission(s._h, em.ctypes.data)
    assert em.tolist() == [[0.0, 0.0, 0.0], [1.5, 0.75, 0.25], [0.0, 0.125, 2.0]]
    assert np.array_equal(s.emission, em)
    assert np.allclose(s.albedo[:, :3], [[0.5, 0.5, 0.5], [0.9, 0.9, 0.9], [0.1, 0.2, 0.3]])      # Kd and Ks still land where they did
    assert np.allclose(s.specular[1], [0.2, 0.4, 0.6])
    # the procedural scenes emit nothing (their goldens and bench lines do not move)
    for kind in (sc.CORNELL, sc.ATRIUM, sc.ATRIUM_TEXTURED, sc.BISTRO):
        assert not sc.Scene(kind, 0.1, 1234).emission.any()


def test_scene_cache_keeps_emission_and_old_caches_load(tmp_path):
    sc = _scene_lib()
    (tmp_path / "lamps.mtl").write_text(MTL)
    (tmp_path / "lamps.obj").write_text(OBJ)
    lit = sc.Scene(str(tmp_path / "lamps.obj"))
    new = str(tmp_path / "lit.vctscene")
    lit.save(new)
    back = sc.Scene(new)
    assert np.array_equal(back.emission, lit.emission) and np.array_equal(back.pos, lit.pos) and np.array_equal(back.albedo, lit.albedo)
    # a cache as it was written before emission existed: the same file without the trailing block (8-byte count + floats)
    blob = open(new, "rb").read()
    tail = 8 + 4 * lit.nmat * 3
    assert np.frombuffer(blob[-tail:-tail + 8], np.uint64)[0] == lit.nmat * 3
    old = str(tmp_path / "old.vctscene")
    open(old, "wb").write(blob[:-tail])
    prev = sc.Scene(old)
    assert not prev.emission.any() and np.array_equal(prev.pos, lit.pos) and np.array_equal(prev.material, lit.material)
    # a scene that emits nothing writes exactly that older format: no trailing block
    plain = str(tmp_path / "plain.vctscene")
    sc.Scene(sc.CORNELL).save(plain)
    cornell = sc.Scene(plain)
    assert not cornell.emission.any() and cornell.nmat == 4
    (tmp_path / "dark.mtl").write_text(MTL.replace("Ke", "#Ke"))
    (tmp_path / "dark.obj").write_text(OBJ.replace("lamps.mtl", "dark.mtl"))
    dark = str(tmp_path / "dark.vctscene")
    sc.Scene(str(tmp_path / "dark.obj")).save(dark)
    assert open(dark, "rb").read() == blob[:-tail]
    # a damaged trailing block is refused, not half read
    for cut in (3, 9, tail - 1):
        bad = str(tmp_path / f"cut{cut}.vctscene")
        open(bad, "wb").write(blob[:-cut])
        with pytest.raises(ValueError):
            sc.Scene(bad)


def test_header_and_binding_agree():
    import vctpkg
    vct = vctpkg.load()
    hdr = open(os.path.join(ROOT, "include", "vct.h")).read()
    for name, args in (("vct_upload_emission", 2), ("vct_set_pixel_emission", 4), ("vct_download_pixel_emission", 2)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        params = re.sub(r"/\*.*?\*/", "", m.group(1))
        assert len(params.split(",")) == args, (name, m.group(1))
        assert name in vct.ABI_SYMBOLS and hasattr(vct.lib(), name)
        assert len(getattr(vct.lib(), name).argtypes) == args
    for py, c_name in ((vct.GB_LINEAR, "VCT_GB_LINEAR"), (vct.GB_TILED, "VCT_GB_TILED"), (vct.MEM_HOST, "VCT_MEM_HOST"),
                       (vct.MEM_DEVICE, "VCT_MEM_DEVICE")):
        assert int(re.search(c_name + r"\s*=\s*(\d+)", hdr).group(1)) == py
    assert int(re.search(r"VCT_SHOW_ALL\s*=\s*(\d+)", hdr).group(1)) == vct.SHOW_ALL == 31      # no new mask bit
    for method in ("upload_emission", "set_pixel_emission", "download_pixel_emission"):
        assert callable(getattr(vct.Context, method))
    internal = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "csrc", "vct_internal.h")).read()
    assert int(re.search(r"#define VCT_EMIS_NPLANES (\d+)", internal).group(1)) == 3


def test_binding_refuses_a_table_of_another_size():
    """Context.upload_emission checks the row count against the mesh's materials before any pointer is handed over (no
    GPU: the check is the binding's, exercised on an object that stands in for a context with a five-material mesh)."""
    import vctpkg
    vct = vctpkg.load()

    class Stub:
        _nmat = 5
        _h = None

        def _ck(self, rc, what):
            raise AssertionError("the table reached the library")
    for rows in (4, 6, 1):
        with pytest.raises(vct.VctError) as e:
            vct.Context.upload_emission(Stub(), np.zeros((rows, 3), np.float32))
        assert "5 materials" in str(e.value)
    src = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "__init__.py")).read()
    assert "self._nmat = albedo.shape[0]" in src


def test_table_check_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "emission_check")
    src = os.path.join(ROOT, "tests", "emission_check_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "emission_check ok" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
