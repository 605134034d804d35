"""Independent cross-check of the oracle's gather + composite against what the reference's own shader TEXT computes.

The reference's cone-trace fragment shader (S/VoxelConeTracing.fs) and voxelization shaders (S/Voxelization.gs / .fs)
were rewritten mechanically into C++ (qualifiers dropped, GLSL array constructors -> braces, multi-component swizzles ->
calls, `discard` -> a flag), compiled against tests/glsl_shim.h, a minimal GLSL stand-in written for this test, and run
on seeded inputs by tests/golden/make_shader_golden.py where the reference tree exists; the shaders' outputs are stored
in tests/golden/ref_shader_text.npz (the shader text itself never is).  Here the inputs are regenerated from their seeds
and oracle/vct_oracle.cpp runs on them: vcto_shade_pixel on 10^4 random G-buffer pixels, the fragment-level
restatements of the voxelization stages on 20,000 triangles and 12,000 fragments.

What it shows: the oracle's restatement of trace.fs:82-107 (march), :165-228 (frame, 6 + 1 cones, composite, the .rrra
rule, discard) agrees with the shader as written -- operation by operation but for rounding (the stand-in uses the GLSL
definitions of normalize / reflect / inverse and no fused multiply-adds; the oracle fixes its own fp32 order).
What it does NOT show by itself: `textureLod` under the shader was the oracle's own sampler and the material / height /
shadow samplers are per-pixel constants, so this test alone pins no output value.  (tests/test_ref_gl.py holds the
oracle to what the reference's shaders produce when executed unmodified by a GL driver; this text-level cross-check
stays as a second, driver-independent reading of the same shaders.)"""
import ctypes as C
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_shader_golden as mg  # noqa: E402 -- the seeded inputs of the stored shader outputs


def stored():
    return mg.load_fixture()          # the shaders' outputs, bit for bit as generated


def test_oracle_agrees_with_the_reference_shader_text():
    import synth
    from oracle import pyoracle
    lib = C.CDLL(mg.ORACLE)
    lib.vcto_shade_pixel.argtypes = [C.c_void_p] * 6
    ref = stored()
    for V, seed in mg.TRACE_CASES:
        chain, gb, spec_raw, shadow_k = mg.trace_inputs(V, seed)
        n = gb.shape[0]
        p = pyoracle.default_params(V)
        # the shader's colour, steps and discards; the oracle gets the pixel with the shader's own bump normal, resolved
        # specular colour (trace.fs:210) and shadow term as INPUTS
        outs, ss = ref[f"trace_V{V}_color"], ref[f"trace_V{V}_steps"].astype(np.int32)
        disc = ref[f"trace_V{V}_discarded"].astype(np.int32)
        gbu = gb.copy()
        gbu[:, mg.GB_SHADER_COLS] = ref[f"trace_V{V}_gb_shader_cols"]
        outo = np.zeros((n, 4), np.float32)
        st = np.zeros((n, 7), np.uint8)
        for i in range(n):
            lib.vcto_shade_pixel(C.byref(p), chain.ctypes.data, gbu[i].ctypes.data, outo[i].ctypes.data, st[i].ctypes.data,
                                 None)
        so_ = st.astype(np.int32)
        live = disc == 0
        # discard: the shader discards exactly the pixels the oracle does not shade (alpha < 0.5, trace.fs:169-172)
        assert np.array_equal(disc == 1, gb[:, 18] < np.float32(0.5))
        assert live.sum() > 0.9 * n
        # executed steps, cone by cone
        same = (ss[live] == so_[live]).all(axis=1)
        print(f"V={V}: {live.sum()} live pixels, step counts differ on {np.count_nonzero(~same)}, steps {so_[live].sum()}")
        assert same.mean() > 0.999, f"step counts differ on {np.count_nonzero(~same)} of {live.sum()} pixels"
        a, b = outs[live][same], outo[live][same]
        rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
        assert rel.max() <= 1e-5, rel.max()
        # (a pixel whose alpha lands within an ulp of MAX_ALPHA may take one step more in one of the two evaluations --
        # the stand-in has no fused multiply-add, the oracle's accumulation has: still within the frame tolerance)
        if (~same).any():
            assert synth.rel_l2(outs[live][~same], outo[live][~same]) <= 1e-3
        assert so_[live].sum() > 20 * live.sum()                                # the march really ran


# ---- the voxelization shaders (S/Voxelization.gs: dominant axis + projection; S/Voxelization.fs: voxel index, PCF,
# stored value) against the oracle's fragment-level restatements (vcto_dominant_axis, vcto_voxel_proj,
# vcto_frag_to_voxel, vcto_pcf25) -------------------------------------------------------------------------------------
def test_oracle_agrees_with_the_reference_voxelization_shaders():
    """S/Voxelization.gs main() (dominant axis, projection by ProjX / ProjY / ProjZ) and S/Voxelization.fs main() (voxel
    index from gl_FragCoord, 25-tap PCF / 25, imageStore of albedo * shadow), as run by the C++ rewrite, next to the
    oracle's fragment-level restatements.  Same caveats as above: the shadow sampler under the shader was the oracle's
    bilinear fetch, the diffuse sampler a per-fragment constant (the executed-shader check of these stages is
    tests/test_ref_gl.py)."""
    lib = C.CDLL(mg.ORACLE)
    ref = stored()
    tri, frags = mg.vox_inputs()
    n = tri.shape[0]
    # ---- geometry stage ----
    proj = mg.voxel_proj(lib)
    axis_s, clip = ref["vox_gs_axis"].astype(np.int32), ref["vox_gs_clip"]
    assert axis_s.shape == (n,) and clip.shape == (n, 3, 4)
    lib.vcto_dominant_axis.argtypes = [C.c_void_p] * 3
    lib.vcto_dominant_axis.restype = C.c_int
    axis_o = np.array([lib.vcto_dominant_axis(t[0:3].ctypes.data_as(C.c_void_p), t[3:6].ctypes.data_as(C.c_void_p),
                                              t[6:9].ctypes.data_as(C.c_void_p)) for t in tri], np.int32)
    degenerate = ~np.isfinite(clip).all(axis=(1, 2))
    assert degenerate.mean() < 0.02
    assert np.array_equal(axis_s[~degenerate], axis_o[~degenerate])
    assert set(np.unique(axis_o)) == {1, 2, 3}
    # the projection the shader applied is the oracle's matrix of that axis
    hom = np.concatenate([tri.reshape(n, 3, 3), np.ones((n, 3, 1), np.float32)], axis=2).astype(np.float64)
    want = np.einsum("nrc,nkc->nkr", proj[axis_o - 1].reshape(n, 4, 4).transpose(0, 2, 1).astype(np.float64), hom)
    ok = ~degenerate
    assert np.abs(clip[ok] - want[ok]).max() <= 1e-4 * max(1.0, np.abs(want[ok]).max())
    # ---- fragment stage ----
    lib.vcto_frag_to_voxel.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]
    lib.vcto_pcf25.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_float]
    lib.vcto_pcf25.restype = C.c_int
    for V, S, depth, frag, albedo in frags:
        m = frag.shape[0]
        voxel, value = ref[f"vox_fs_V{V}_voxel"].astype(np.int32), ref[f"vox_fs_V{V}_value"]
        assert voxel.shape == (m, 3) and value.shape == (m, 4)
        wv = np.zeros((m, 3), np.int32); cnt = np.zeros(m, np.int32)
        for i in range(m):
            lib.vcto_frag_to_voxel(V, int(frag[i, 3]), C.c_float(frag[i, 0]), C.c_float(frag[i, 1]), C.c_float(frag[i, 2]),
                                   wv[i].ctypes.data_as(C.c_void_p))
            cnt[i] = lib.vcto_pcf25(depth.ctypes.data_as(C.c_void_p), S, frag[i, 4:7].ctypes.data_as(C.c_void_p), C.c_float(0.002))
        assert np.array_equal(voxel, wv)
        assert 0 < (cnt == 0).sum() and 0 < (cnt == 25).sum() and ((cnt > 0) & (cnt < 25)).sum() > m // 20
        shadow = cnt.astype(np.float32) / np.float32(25.0)
        want_rgb = albedo[:, :3] * shadow[:, None]
        assert np.abs(value[:, :3] - want_rgb).max() <= 1e-6 and (value[:, 3] == 1.0).all()
