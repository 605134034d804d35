"""The GPU raster input stages (csrc/vct_raster.hip) on meshes built to hit their decision points (tests/geomcases.py:
near-plane fans with clipped polygons beyond 2^16 and 2^23 pixels, vertices exactly on z = -w and w = 0, pixel centres
exactly on edges and vertices, exact depth ties, depth exactly 0 and 1, slivers and zero-area triangles, one triangle
over every bin, a single triangle, alpha-tested cards), at model_scale = 1/16 and raw view-projection matrices.

* Bit for bit against the CPU checker: shadow map and all 23 G-buffer planes, with the direct and the binned form,
  texture_mipmaps 1 and 0 where a case is textured, a scissored pass between two whole-frame passes on one context,
  the bin-capacity overflow path, and once through vct_gi_pass.
* Against the independent float64 ray caster (tests/raster_f64.py) with the bars measured on the CPU checker
  (test_raster_cases.py's docstring has the table): the GPU's own error sets no bar.
* Watertightness on a subdivided rectangle, and the non-default scene scales (model_scale, grid_world_size) through
  both raster stages.
Every test asserts the float64 classifier's counts first, so a case cannot quietly stop exercising what it is named for.
"""
import os

import numpy as np
import pytest

import geomcases
import raster_f64
import raster_oracle
import vctpkg
import voxcases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available()
    return vctpkg.load()


def make_context(vct, case, path, mips=1, V=32, **kw):
    """A context for a geomcases.Case with VCT_RASTER_PATH = path while it is created (read at vct_create)."""
    old = os.environ.pop("VCT_RASTER_PATH", None)
    if path:
        os.environ["VCT_RASTER_PATH"] = path
    try:
        ctx = vct.Context(vct.default_config(voxel_dim=V, width=case.w, height=case.h, shadow_map_size=case.shadow_size,
                                             model_scale=case.model_scale, texture_mipmaps=mips, **kw))
    finally:
        os.environ.pop("VCT_RASTER_PATH", None)
        if old is not None:
            os.environ["VCT_RASTER_PATH"] = old
    ctx.upload_triangles(case.pos, case.material, case.albedo)
    ctx.upload_mesh_attributes(*case.frames(), case.specular)
    if case.textures:
        ctx.upload_mesh_uvs(case.uv)
        ctx.upload_textures(case.textures, case.mat_tex)
    return ctx


def assert_same_bits(got, want, case, cls, what):
    g = np.ascontiguousarray(got, np.float32).reshape(-1, case.h * case.w) if what != "shadow" else \
        np.ascontiguousarray(got, np.float32).reshape(1, -1)
    w = np.ascontiguousarray(want, np.float32).reshape(g.shape)
    bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).any(0))[0]
    if bad.size:
        lines = [f"{case.name} {what}: {bad.size} pixels differ"]
        for i in bad[:6]:
            planes = np.nonzero(g[:, i].view(np.uint32) != w[:, i].view(np.uint32))[0]
            line = f"  pixel {i}: planes {planes[:8].tolist()} got {g[planes[:4], i].tolist()} want {w[planes[:4], i].tolist()}"
            if what != "shadow":
                line += f" classifier: {geomcases.verdict(cls, i // case.w, i % case.w)}"
            lines.append(line)
        raise AssertionError("\n".join(lines))


@pytest.mark.parametrize("path", ["direct", "binned"])
@pytest.mark.parametrize("name", geomcases.CASE_NAMES)
def test_adversarial_case_bit_exact(vct, name, path):
    case = geomcases.get_case(name)
    cls = geomcases.check_minimum(case)
    rows = (case.h + 7) // 8
    r0, r1 = (rows // 3, max(rows // 3 + 1, 2 * rows // 3))
    for mips in ((1, 0) if case.textures else (1,)):
        depth, want = raster_oracle.case_reference(case, bool(mips))
        ctx = make_context(vct, case, path, mips)
        ctx.render_shadow_map(case.light_vp)
        assert_same_bits(ctx.download_shadow_map(), depth, case, cls, "shadow")
        ctx.render_gbuffer(case.vp)
        assert_same_bits(ctx.download_gbuffer(), want, case, cls, f"gbuffer mips={mips}")
        ctx.render_gbuffer_rows(case.vp, r0, r1)                                   # a scissored pass in between
        y0, y1 = r0 * 8, min(r1 * 8, case.h)
        got = ctx.download_gbuffer().reshape(23, case.h, case.w)[:, y0:y1]
        ref = want.reshape(23, case.h, case.w)[:, y0:y1]
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)), (r0, r1)
        ctx.render_shadow_map(case.light_vp)
        ctx.render_gbuffer(case.vp)
        assert_same_bits(ctx.download_gbuffer(), want, case, cls, f"gbuffer, second whole pass, mips={mips}")
        assert_same_bits(ctx.download_shadow_map(), depth, case, cls, "shadow")
        ctx.close()


@pytest.mark.parametrize("name", geomcases.CASE_NAMES)
def test_adversarial_case_through_gi_pass(vct, name):
    case = geomcases.get_case(name)
    cls = geomcases.check_minimum(case)
    depth, want = raster_oracle.case_reference(case)
    ctx = make_context(vct, case, None)
    for _ in range(2):
        ctx.gi_pass(case.light_vp, case.vp)
        assert_same_bits(ctx.download_shadow_map(), depth, case, cls, "shadow")
        assert_same_bits(ctx.download_gbuffer(), want, case, cls, "gbuffer of vct_gi_pass")
    ctx.close()


@pytest.mark.parametrize("caps", ["40,1000000", "1000000,300", "64,64"])
@pytest.mark.parametrize("name", ["full_frame_and_small", "near_plane_fan"])
def test_adversarial_case_with_bin_capacity_overflow(vct, name, caps):
    case = geomcases.get_case(name)
    cls = geomcases.check_minimum(case)
    depth, want = raster_oracle.case_reference(case)
    os.environ["VCT_BIN_TEST_CAPS"] = caps
    try:
        ctx = make_context(vct, case, "binned")
        ctx.render_shadow_map(case.light_vp)
        ctx.render_gbuffer(case.vp)
    finally:
        os.environ.pop("VCT_BIN_TEST_CAPS", None)
    assert_same_bits(ctx.download_shadow_map(), depth, case, cls, "shadow")
    assert_same_bits(ctx.download_gbuffer(), want, case, cls, "gbuffer")
    ctx.close()


def gpu_render(vct, case, path):
    ctx = make_context(vct, case, path)
    ctx.render_shadow_map(case.light_vp)
    ctx.render_gbuffer(case.vp)
    out = ctx.download_shadow_map().copy(), ctx.download_gbuffer().copy()
    ctx.close()
    return out


@pytest.mark.parametrize("path", ["direct", "binned"])
@pytest.mark.parametrize("name", raster_f64.RC_NAMES)
def test_library_against_the_float64_ray_caster(vct, name, path):
    case = raster_f64.rc_case(name)
    depth, planes = gpu_render(vct, case, path)
    raster_f64.check_against_ray_caster(name, planes, depth, f"gpu/{path}")


@pytest.mark.parametrize("path", ["direct", "binned"])
def test_library_is_watertight_on_a_subdivided_rectangle(vct, path):
    geomcases.check_watertight(lambda case: gpu_render(vct, case, path)[1])


# ---- non-default scene scales through both raster stages ----------------------------------------------------------
SCALES = [(ms, G) for ms in (0.05, 1.0, 0.0137) for G in (150.0, 100.0, 317.3)]


def rescaled_scene(sc, scene, w, h, cam, light, model_scale, G):
    """(scene object with the mesh rescaled so that it fills a grid of G at model_scale as it fills 150 at 0.05, camera
    matrix, light matrix): the matrices see the rescaled world as the originals saw the original."""
    k = G / 150.0

    class Scaled:
        pos = voxcases.rescale(scene.pos, model_scale, G)
        material, albedo, specular, uv, mat_tex, textures = (scene.material, scene.albedo, scene.specular, scene.uv,
                                                             scene.mat_tex, scene.textures)
        frames = staticmethod(scene.frames)

    def seen_as_before(m):                       # column-major float32[16]: rows of the reshaped array are columns
        m = np.asarray(m, np.float64).reshape(4, 4).copy()
        m[:3, :] /= k
        return m.astype(np.float32).reshape(16)
    return Scaled, seen_as_before(sc.camera_view_proj(cam, w, h)), seen_as_before(sc.light_view_proj(light))


def scaled_reference(sc, scene, w, h, S, cam, light, model_scale, G):
    scaled, vp, lvp = rescaled_scene(sc, scene, w, h, cam, light, model_scale, G)
    depth = raster_oracle.pyoracle.render_shadow_map(raster_oracle.mesh_of(scaled, model_scale), lvp, S)
    planes = raster_oracle.pyoracle.render_gbuffer(raster_oracle.mesh_of(scaled, model_scale), vp, w, h, depth, lvp)
    return scaled, vp, lvp, depth, planes


@pytest.mark.parametrize("path", ["direct", "binned"])
@pytest.mark.parametrize("model_scale,G", SCALES)
def test_raster_stages_at_other_scene_scales(vct, model_scale, G, path):
    from voxel_cone_tracing_amd import scene as sc
    scene = sc.Scene(1, 0.15, 1234)
    w, h, S = 160, 90, 256
    cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
    light = (0.0, 1.0, 0.25)
    _, _, _, depth0, planes0 = scaled_reference(sc, scene, w, h, S, cam, light, 0.05, 150.0)
    scaled, vp, lvp, depth, want = scaled_reference(sc, scene, w, h, S, cam, light, model_scale, G)
    # the band, from the default case itself: rescaling mesh and matrix together may move a few boundary pixels only
    cov0, cov = (planes0[18] >= 0.5).mean(), (want[18] >= 0.5).mean()
    sh0, sh = (depth0 < 1.0).mean(), (depth < 1.0).mean()
    assert cov0 > 0.9 and sh0 > 0.1 and abs(cov - cov0) <= 0.01 and abs(sh - sh0) <= 0.01, (cov, cov0, sh, sh0)
    old = os.environ.pop("VCT_RASTER_PATH", None)
    os.environ["VCT_RASTER_PATH"] = path
    try:
        ctx = vct.Context(vct.default_config(voxel_dim=32, width=w, height=h, shadow_map_size=S, model_scale=model_scale,
                                             grid_world_size=G))
    finally:
        os.environ.pop("VCT_RASTER_PATH", None)
        if old is not None:
            os.environ["VCT_RASTER_PATH"] = old
    ctx.upload_scene(scaled)
    ctx.render_shadow_map(lvp)
    ctx.render_gbuffer(vp)
    assert np.array_equal(ctx.download_shadow_map().view(np.uint32), depth.view(np.uint32))
    got = ctx.download_gbuffer()
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(0))[0]
    assert bad.size == 0, (bad[:10], got[:, bad[:1]].ravel(), want[:, bad[:1]].ravel())
    ctx.close()


# ---- the vertex contract of include/vct.h ---------------------------------------------------------------------------
def test_upload_refuses_vertices_outside_the_contract_and_keeps_the_old_mesh(vct):
    case = geomcases.get_case("full_frame_and_small")
    cls = geomcases.check_minimum(case)
    depth, want = raster_oracle.case_reference(case)
    ctx = make_context(vct, case, None)
    beyond = voxcases.at_the_bound(case.model_scale, 150.0, inside=False)      # the first fp32 value outside
    for value in (np.nan, np.inf, -np.inf, beyond, -beyond):
        for slot in (0, 4, case.ntri * 9 - 1):
            pos = case.pos.copy()
            pos.reshape(-1)[slot] = value
            with pytest.raises(vct.VctError) as e:
                ctx.upload_triangles(pos, case.material, case.albedo)
            assert "vertex contract" in str(e.value)
    # the refused uploads changed nothing: the context still draws the mesh it had
    ctx.render_shadow_map(case.light_vp)
    ctx.render_gbuffer(case.vp)
    assert_same_bits(ctx.download_shadow_map(), depth, case, cls, "shadow")
    assert_same_bits(ctx.download_gbuffer(), want, case, cls, "gbuffer after refused uploads")
    ctx.close()


def test_upload_accepts_a_vertex_just_inside_the_contract(vct):
    """One vertex at 0.999 of the bound (2^20 grid widths): accepted, and both raster stages still agree with the
    checker bit for bit."""
    base = geomcases.get_case("slivers")
    big = np.float32(2.0 ** 20 * 150.0 * 0.999) / np.float32(base.model_scale)
    tri = np.array([[10.0 / base.model_scale, 5.0 / base.model_scale, -0.5 / base.model_scale,
                     big, 20.0 / base.model_scale, -0.5 / base.model_scale,
                     10.0 / base.model_scale, 60.0 / base.model_scale, -0.5 / base.model_scale]], np.float32)
    case = geomcases.Case("inside_bound", np.concatenate([tri, base.pos]), base.vp, base.w, base.h, base.model_scale,
                          dict(beyond23=1, front=100))
    cls = geomcases.check_minimum(case)
    depth, want = raster_oracle.case_reference(case)
    for path in ("direct", "binned"):
        ctx = make_context(vct, case, path)
        ctx.render_shadow_map(case.light_vp)
        ctx.render_gbuffer(case.vp)
        assert_same_bits(ctx.download_shadow_map(), depth, case, cls, "shadow")
        assert_same_bits(ctx.download_gbuffer(), want, case, cls, "gbuffer")
        ctx.close()
