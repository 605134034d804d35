"""GPU: emissive materials (include/vct.h "emissive materials") -- the emission pool and the saturating add of the
resolve, the pixel-emission planes of the G-buffer pass and the composite's last add -- bit for bit against
tests/emission_ref.py, which forms every expected value from the CPU oracle as it is.

Level 0 runs at V = 32, frames at 64 x 48 (six tile rows).  The composite cases use a random G-buffer with discarded
pixels whose shadow plane is 0 (every pixel in shadow, the emitter-only set-up of the header): the direct specular term
is powf(...) * shadow, and numpy's pow and the device's differ in the last place for some arguments, so with a shadow
term the restatement of tests/components_ref.py is itself only good to >= 99.9 % of the fp16 values (what
test_gpu_components.py asks of it).  With shadow = 0 that term is exactly 0 on both sides, every other operation of
the composite is a single correctly rounded fp32 multiply or add, and the frame can be held bit for bit -- ambient,
indirect diffuse and indirect specular all stay non-zero, so the order ((A + D) + S) + E is still what is compared."""
import os
import subprocess
import sys

import numpy as np
import pytest

import components_ref as cr
import diffuse_rate_ref as drr
import emission_ref as er
import raster_oracle
import synth
import vctpkg
import voxcases
from test_gpu_parity import light_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, W, H = 32, 64, 48
CAM, LIGHT = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)
ALL_AOV = cr.AOV_INDIRECT_DIFFUSE | cr.AOV_INDIRECT_SPECULAR | cr.AOV_DIRECT


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available()
    return vctpkg.load()


def invalid(vct, call, *args):
    with pytest.raises(vct.VctError) as e:
        call(*args)
    assert "(-1)" in str(e.value), str(e.value)      # VCT_ERR_INVALID
    return str(e.value)


def run_pass(ctx):
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    return ctx.download_chain()


def assert_chain(got, want, what=""):
    bad = np.argwhere((got[: V ** 3] != want[: V ** 3]).any(-1).reshape(V, V, V))
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:6].tolist())
    assert np.array_equal(got, want), what


# ---- level 0, chain, bounce -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lit(oracle):
    """random_scene(300, 7) under a 64^2 random-depth shadow map, flat and with one diffuse texture: expected level 0
    and chain with er.EMISSION, and the plain ones."""
    pos, mat, alb = voxcases.random_scene(300, 7)
    depth, vp = light_setup(64, 3)
    p = oracle.default_params(V)
    r = np.random.default_rng(11)
    tex = r.integers(0, 256, (8, 8, 4), dtype=np.uint8)
    tex[..., 3] = 255
    uv = r.uniform(0.0, 2.0, (pos.shape[0], 6)).astype(np.float32)
    mat_tex = np.full((5, 3), -1, np.int32)
    mat_tex[1, 0] = 0                                   # material 1 emits AND takes its albedo from the texture
    out = dict(pos=pos, mat=mat, alb=alb, depth=depth, vp=vp, p=p, uv=uv, tex=[tex], mat_tex=mat_tex)
    for name, kw in (("flat", {}), ("textured", dict(uv=uv, mat_tex=mat_tex, textures=[tex], mipmaps=True))):
        want, L, Em = er.level0(oracle, p, pos, mat, alb, er.EMISSION, shadow_depth=depth, light_vp=vp, **kw)
        out[name] = dict(want=want, L=L, Em=Em, chain=oracle.build_mips(want), plain=oracle.build_mips(L))
    assert not np.array_equal(out["flat"]["L"], out["textured"]["L"])
    assert np.array_equal(out["flat"]["Em"], out["textured"]["Em"])       # Em takes no texture
    return out


def lit_ctx(vct, lit, textured=False, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=8, height=8, **kw))
    ctx.upload_triangles(lit["pos"], lit["mat"], lit["alb"])
    if textured:
        ctx.upload_mesh_uvs(lit["uv"])
        ctx.upload_textures(lit["tex"], lit["mat_tex"])
    ctx.upload_shadow_map(lit["depth"], lit["vp"])
    return ctx


@pytest.mark.parametrize("kind", ["flat", "textured"])
def test_level0_and_chain(vct, lit, kind):
    n = er.non_degeneracy(lit[kind]["L"], lit[kind]["Em"], er.EMISSION)
    assert n["saturating"] >= 50 and n["both"] >= 50 and n["mixed_values"] >= 1, n
    with lit_ctx(vct, lit, textured=kind == "textured") as ctx:
        ctx.upload_emission(er.EMISSION)
        for _ in range(2):                              # the second pass reuses the pool
            assert_chain(run_pass(ctx), lit[kind]["chain"], kind)


def test_multi_chunk_slots(vct, oracle):
    pos, mat, alb, ms, G, Vc = voxcases.whole_grid_and_a_crowded_brick()
    assert Vc == V
    depth, vp = light_setup(64, 3)
    p = oracle.default_params(V, G=G)
    want, L, Em = er.level0(oracle, p, pos, mat, alb, er.EMISSION, ms, shadow_depth=depth, light_vp=vp)
    n = er.non_degeneracy(L, Em, er.EMISSION)
    assert n["saturating"] >= 50 and n["both"] >= 50 and n["mixed_values"] >= 1, n
    with vct.Context(vct.default_config(voxel_dim=V, width=8, height=8, model_scale=ms, grid_world_size=G)) as ctx:
        ctx.upload_triangles(pos, mat, alb)
        ctx.upload_shadow_map(depth, vp)
        counts = ctx.stage_counts()
        assert counts["vox_items"] > counts["accumulator_bricks"], counts      # a slot was cut into chunks
        ctx.upload_emission(er.EMISSION)
        for _ in range(2):
            assert_chain(run_pass(ctx), oracle.build_mips(want))
        ctx.upload_emission(None)                       # ... and the accumulators were left clean for the plain pass
        assert_chain(run_pass(ctx), oracle.build_mips(L))


def test_bounce_gathers_the_emission(vct, oracle, lit):
    p, f = lit["p"], lit["flat"]
    sc = oracle.make_scene(lit["pos"], lit["mat"], lit["alb"], shadow_depth=lit["depth"], light_vp=lit["vp"])
    l0, alb, nrm = oracle.voxelize_conservative_attr(p, sc)
    assert np.array_equal(l0, f["L"])
    want_l1, want_steps = oracle.bounce(p, f["chain"], alb, nrm, nthreads=8)
    plain_l1, _ = oracle.bounce(p, f["plain"], alb, nrm, nthreads=8)
    assert want_steps > 0 and not np.array_equal(want_l1, plain_l1)
    with lit_ctx(vct, lit, voxel_attributes=1) as ctx:
        ctx.upload_emission(er.EMISSION)
        assert_chain(run_pass(ctx), f["chain"])
        got_alb, got_nrm = ctx.voxel_attributes()
        assert np.array_equal(got_alb, alb) and np.array_equal(got_nrm, nrm)      # the no-emission attributes
        ctx.bounce()
        assert ctx.last_step_count() == want_steps
        assert_chain(ctx.download_chain(), oracle.build_mips(want_l1))


def test_state(vct, oracle, lit):
    f, p = lit["flat"], lit["p"]
    other = np.array([[0.5, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.2, 1.5], [0.0, 0.0, 0.0], [0.1, 0.1, 0.1]], np.float32)
    want_other, _, _ = er.level0(oracle, p, lit["pos"], lit["mat"], lit["alb"], other, shadow_depth=lit["depth"], light_vp=lit["vp"])
    depth2, vp2 = light_setup(64, 9)
    want_moved, L_moved, _ = er.level0(oracle, p, lit["pos"], lit["mat"], lit["alb"], other, shadow_depth=depth2, light_vp=vp2)
    dark = np.zeros((64, 64), np.float32)
    want_dark, L_dark, Em_dark = er.level0(oracle, p, lit["pos"], lit["mat"], lit["alb"], other, shadow_depth=dark, light_vp=vp2)
    assert not L_dark[..., :3].any() and np.array_equal(want_dark, Em_dark) and Em_dark[..., :3].any()
    assert not np.array_equal(L_moved, f["L"])
    with lit_ctx(vct, lit) as ctx:
        assert_chain(run_pass(ctx), f["plain"], "no table")
        ctx.upload_emission(np.zeros((5, 3), np.float32))           # all zero: detached
        invalid(vct, ctx.download_pixel_emission)                   # ... so no planes either
        assert_chain(run_pass(ctx), f["plain"], "all-zero table")
        ctx.upload_emission(er.EMISSION)
        assert_chain(ctx.download_chain(), f["plain"], "before the next pass")
        assert_chain(run_pass(ctx), f["chain"], "first table")
        ctx.upload_emission(other)                                  # a changed table: not before the next voxelize + inject
        assert_chain(ctx.download_chain(), f["chain"], "changed table, before the next pass")
        invalid(vct, ctx.inject_light)                              # (nothing voxelized: inject alone is refused as ever)
        ctx.voxelize()
        assert_chain(ctx.download_chain(), f["chain"], "voxelized, not injected")
        ctx.inject_light()
        invalid(vct, ctx.trace, synth.random_gbuffer(64, seed=1))   # level 0 changed since the last mip build: the rule applies
        ctx.build_mips()
        assert_chain(ctx.download_chain(), oracle.build_mips(want_other), "changed table")
        ctx.upload_shadow_map(depth2, vp2)                          # a moved light with emission attached: the pool is reused
        assert_chain(run_pass(ctx), oracle.build_mips(want_moved), "moved light")
        ctx.upload_shadow_map(dark, vp2)                            # everything in shadow: level 0 is Em exactly
        assert_chain(run_pass(ctx), oracle.build_mips(Em_dark), "dark map")
        ctx.upload_emission(None)                                   # detached: bricks only emission made non-zero go back to 0 rgb
        assert_chain(run_pass(ctx), oracle.build_mips(L_dark), "detached under the dark map")
        ctx.upload_shadow_map(lit["depth"], lit["vp"])
        ctx.upload_emission(er.EMISSION)
        assert_chain(run_pass(ctx), f["chain"], "attached again")
        ctx.upload_triangles(lit["pos"], lit["mat"], lit["alb"])    # a new mesh detaches
        invalid(vct, ctx.download_pixel_emission)
        assert_chain(run_pass(ctx), f["plain"], "after re-uploading the triangles")


def test_refusals(vct, lit):
    f = lit["flat"]
    planes = synth.random_gbuffer(W * H, seed=5, discard_frac=0.05)
    with vct.Context(vct.default_config(voxel_dim=V, width=W, height=H)) as ctx:
        invalid(vct, ctx.upload_emission, er.EMISSION)              # before any mesh
        ctx.upload_triangles(lit["pos"], lit["mat"], lit["alb"])
        ctx.upload_shadow_map(lit["depth"], lit["vp"])
        ctx.upload_emission(er.EMISSION)
        assert_chain(run_pass(ctx), f["chain"])
        frame = ctx.trace(planes)
        for value in (np.nan, -1e-30, -1.0, np.inf, -np.inf):
            for at in ((0, 0), (4, 2)):
                bad = er.EMISSION.copy()
                bad[at] = value
                msg = invalid(vct, ctx.upload_emission, bad)
                assert "material %d" % at[0] in msg
            assert_chain(run_pass(ctx), f["chain"], value)          # the context kept the table it had
        invalid(vct, ctx.voxelize, vct.VOX_REFERENCE)               # the shaders as written have no emission
        assert_chain(run_pass(ctx), f["chain"], "after reference mode was refused")
        for variant in (1, 2, 3, 4):                                # planes are attached (the table attached them)
            invalid(vct, ctx.set_trace_variant, variant)
        assert np.array_equal(ctx.trace(planes), frame)
        invalid(vct, ctx.set_lighting_components, 32)               # no new mask bit
        invalid(vct, ctx.set_pixel_emission, np.zeros((3, W * H), np.float32), 2)      # unknown layout
        ctx.upload_emission(None)
        ctx.voxelize(vct.VOX_REFERENCE)                             # detached: reference mode works again
        ctx.inject_light(); ctx.build_mips()
        for variant in (1, 2, 3, 4):
            ctx.set_trace_variant(variant)
            invalid(vct, ctx.set_pixel_emission, np.zeros((3, W * H), np.float32))
            invalid(vct, ctx.upload_emission, er.EMISSION)
        ctx.set_trace_variant(0)
        assert_chain(run_pass(ctx), f["plain"], "after the refusals")


# ---- pixel-emission planes of the G-buffer pass ------------------------------------------------------------------------
CORNELL_EMISSION = np.array([[0.0, 0.0, 0.0], [3.0, 0.25, 0.0], [0.0, 0.0, 0.0], [0.5, 0.5, 1.75]], np.float32)

CHILD = r"""
import os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path[:0] = [root, os.path.join(root, "tests")]
import vctpkg
vct = vctpkg.load()
from voxel_cone_tracing_amd import scene as sc
import test_gpu_emission as t
scene = sc.Scene(sc.CORNELL)
cam = sc.default_camera(position=(0.0, 0.0, 160.0), yaw=-80.0, pitch=5.0)
with vct.Context(vct.default_config(voxel_dim=t.V, width=t.W, height=t.H, shadow_map_size=128)) as ctx:
    ctx.upload_scene(scene)
    ctx.upload_emission(t.CORNELL_EMISSION)
    ctx.render_shadow_map(sc.light_view_proj((0.0, 1.0, 0.25)))
    ctx.render_gbuffer(sc.camera_view_proj(cam, t.W, t.H))
    np.savez(out, E=ctx.download_pixel_emission(), planes=ctx.download_gbuffer(), form=ctx.stage_counts().get("raster_form", -1))
"""


def cornell(oracle):
    from voxel_cone_tracing_amd import scene as sc
    scene = sc.Scene(sc.CORNELL)
    cam = sc.default_camera(position=(0.0, 0.0, 160.0), yaw=-80.0, pitch=5.0)
    light = (0.0, 1.0, 0.25)
    depth, lvp_row = raster_oracle.shadow_map(sc, scene, light, 128)
    planes = raster_oracle.gbuffer(sc, scene, cam, W, H, depth, lvp_row)
    E = er.pixel_emission(planes, scene.albedo, CORNELL_EMISSION)
    covered = planes[18] >= 0.5
    assert 0.5 < covered.mean() < 0.98 and (E[:, ~covered] == 0).all()       # some pixels show no surface
    assert len({tuple(v) for v in E.T.tolist()}) >= 3                        # both emitters and a non-emitter are in view
    return sc, scene, cam, light, planes, E


@pytest.mark.parametrize("path", ["direct", "binned"])
def test_gbuffer_pass_writes_the_planes_under_each_raster_path(vct, oracle, tmp_path, path):
    _, _, _, _, planes, E = cornell(oracle)
    out = str(tmp_path / f"{path}.npz")
    env = dict(os.environ, VCT_RASTER_PATH=path)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(out)
    assert int(got["form"]) == {"direct": 1, "binned": 2}[path]        # the form that was asked for did run
    assert np.array_equal(got["planes"].view(np.uint32), planes.view(np.uint32))
    assert np.array_equal(got["E"].view(np.uint32), E.view(np.uint32))


def test_gbuffer_rows_and_the_textured_instantiation(vct, oracle):
    sc, scene, cam, light, planes, E = cornell(oracle)
    vp = sc.camera_view_proj(cam, W, H)
    y = np.arange(W * H) // W
    with vct.Context(vct.default_config(voxel_dim=V, width=W, height=H, shadow_map_size=128)) as ctx:
        ctx.upload_scene(scene)
        ctx.upload_emission(CORNELL_EMISSION)
        assert not ctx.download_pixel_emission().any()               # attached: zeroed planes until a pass writes them
        ctx.render_shadow_map(sc.light_view_proj(light))
        ctx.set_pixel_emission(np.full((3, W * H), 7.0, np.float32))
        ctx.render_gbuffer_rows(vp, 1, 3)                            # tile rows 1, 2 = pixel rows 8 .. 23
        got = ctx.download_pixel_emission()
        inside = (y >= 8) & (y < 24)
        assert np.array_equal(got[:, inside].view(np.uint32), E[:, inside].view(np.uint32))
        assert (got[:, ~inside] == 7.0).all()
        ctx.render_gbuffer(vp)
        assert np.array_equal(ctx.download_pixel_emission().view(np.uint32), E.view(np.uint32))
        # an opaque SPECULAR map on one material: the scene has textures (the other k_gbuffer_shade instantiation),
        # visibility and the albedo planes stay what they were
        r = np.random.default_rng(4)
        tex = r.integers(0, 256, (8, 8, 4), dtype=np.uint8)
        tex[..., 3] = 255
        mat_tex = np.full((scene.nmat, 3), -1, np.int32)
        mat_tex[1, 1] = 0
        ctx.upload_mesh_uvs(scene.uv)
        ctx.upload_textures([tex], mat_tex)
        ctx.set_pixel_emission(np.full((3, W * H), 7.0, np.float32))
        ctx.render_gbuffer(vp)
        g = ctx.download_gbuffer()
        assert np.array_equal(g[15:19].view(np.uint32), planes[15:19].view(np.uint32))
        assert not np.array_equal(g[19:22].view(np.uint32), planes[19:22].view(np.uint32))      # the map is in use
        assert np.array_equal(ctx.download_pixel_emission().view(np.uint32), E.view(np.uint32))
        # the table detached: planes the CALLER set stay, and a G-buffer pass leaves them alone; his detach frees them
        ctx.set_pixel_emission(np.full((3, W * H), 7.0, np.float32))
        ctx.upload_emission(None)
        ctx.render_gbuffer(vp)
        assert (ctx.download_pixel_emission() == 7.0).all()
        ctx.set_pixel_emission(None)
        invalid(vct, ctx.download_pixel_emission)
        # ... while planes the table attached go with it
        ctx.upload_emission(CORNELL_EMISSION)
        ctx.render_gbuffer(vp)
        assert np.array_equal(ctx.download_pixel_emission().view(np.uint32), E.view(np.uint32))
        ctx.upload_emission(None)
        invalid(vct, ctx.download_pixel_emission)


# ---- the composite -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded(oracle):
    chain = oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.06))
    planes = synth.random_gbuffer(W * H, seed=21, discard_frac=0.05)
    planes[22] = 0.0                                    # every pixel in shadow (module docstring)
    r = np.random.default_rng(8)
    E = (r.normal(size=(3, W * H)) * r.choice([0.0, 0.5, 3.0, 1e4], size=(1, W * H))).astype(np.float32)
    alive = ~(planes[18] < 0.5)
    assert 0.02 < (~alive).mean() < 0.1 and (E[:, alive] != 0).any(0).mean() > 0.5
    return dict(chain=chain, planes=planes, E=E, alive=alive, p=oracle.default_params(V, camera_pos=CAM, light_dir=LIGHT))


def frame_ctx(vct, s, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=W, height=H, **kw))
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    ctx.upload_chain(s["chain"])
    return ctx


def tiled(E):
    """linear [3, H*W] -> tiled [tile][3][64]."""
    t = E.reshape(3, H // 8, 8, W // 8, 8).transpose(1, 3, 0, 2, 4)
    return np.ascontiguousarray(t.reshape(-1, 3, 64))


def want_frame(s, cones, mask=cr.SHOW_ALL, E=None):
    rgba = cr.composite(s["planes"], cones, CAM, LIGHT, s["p"].ambient_factor, s["p"].shininess, mask)["rgba32f"]
    return er.frame(rgba, s["planes"], s["E"] if E is None else E).reshape(H, W, 4)


def test_composite_adds_the_planes(vct, seeded):
    import torch
    s = seeded
    E, alive = s["E"], s["alive"]
    with frame_ctx(vct, s, debug_outputs=1) as ctx:
        plain = ctx.trace(s["planes"])
        cones = ctx.cones()
        assert np.array_equal(plain.reshape(-1, 4), er.frame(
            cr.composite(s["planes"], cones, CAM, LIGHT, s["p"].ambient_factor, s["p"].shininess)["rgba32f"], s["planes"],
            np.full_like(E, -0.0))), "the restatement holds the plain frame bit for bit on this G-buffer"
        want = want_frame(s, cones)
        assert (want[..., :3] != plain[..., :3]).any(-1).reshape(-1)[alive].mean() > 0.5
        dev_lin, dev_til = torch.from_numpy(E).cuda(), torch.from_numpy(tiled(E)).cuda()
        for what, arg, layout in (("host linear", E, vct.GB_LINEAR), ("host tiled", tiled(E), vct.GB_TILED),
                                  ("device linear", dev_lin.data_ptr(), vct.GB_LINEAR),
                                  ("device tiled", dev_til.data_ptr(), vct.GB_TILED)):
            ctx.set_pixel_emission(None)
            assert np.array_equal(ctx.trace(s["planes"]), plain), what
            ctx.set_pixel_emission(arg, layout)
            assert np.array_equal(ctx.download_pixel_emission().view(np.uint32), E.view(np.uint32)), what
            assert np.array_equal(ctx.trace(s["planes"]), want), what
            assert np.array_equal(ctx.cones(), cones), what
        ctx.synchronize()
        # two other masks, and an output on (the outputs themselves unchanged by the planes)
        for mask in (cr.SHOW_DIFFUSE | cr.SHOW_INDIRECT_SPECULAR, cr.SHOW_INDIRECT_DIFFUSE | cr.SHOW_AMBIENT_OCCLUSION):
            ctx.set_lighting_components(mask)
            got = ctx.trace(s["planes"])
            assert np.array_equal(got, want_frame(s, ctx.cones(), mask)), mask
        ctx.set_lighting_components(cr.SHOW_ALL)
        ctx.set_pixel_emission(None)
        ctx.set_aov_outputs(ALL_AOV)
        assert np.array_equal(ctx.trace(s["planes"]), plain)
        aovs = [ctx.download_aov(b).copy() for b in (1, 2, 4)]
        ctx.set_pixel_emission(E)
        assert np.array_equal(ctx.trace(s["planes"]), want)
        for b, a in zip((1, 2, 4), aovs):
            assert np.array_equal(ctx.download_aov(b), a), b
        ctx.set_aov_outputs(0)
        # a NaN in E changes its own pixel's rgb only; in a discarded pixel it changes nothing
        k, dead = int(np.flatnonzero(alive)[17]), int(np.flatnonzero(~alive)[3])
        E2 = E.copy()
        E2[1, k] = np.nan
        E2[:, dead] = np.nan
        ctx.set_pixel_emission(E2)
        got = ctx.trace(s["planes"]).reshape(-1, 4)
        w2 = want.reshape(-1, 4).copy()
        assert (got[k, 1] & 0x7fff) > 0x7c00 and got[k, 0] == w2[k, 0] and got[k, 2] == w2[k, 2] and got[k, 3] == w2[k, 3]
        w2[k, 1] = got[k, 1]
        assert np.array_equal(got, w2)
        # +0 planes on the G-buffer WITH its shadow term: x + 0 is x (a -0 sum aside), so the frame is the plain one
        lit_planes = synth.random_gbuffer(W * H, seed=21, discard_frac=0.05)
        ctx.set_pixel_emission(None)
        base = ctx.trace(lit_planes)
        ctx.set_pixel_emission(np.zeros_like(E))
        got = ctx.trace(lit_planes)
        assert np.array_equal(got[base != 0x8000], base[base != 0x8000]) and (got[base == 0x8000] == 0).all()


def test_composite_adds_the_planes_to_a_lit_frame(vct, seeded):
    """The same add with the G-buffer's shadow term alive, so that the direct terms in D and S are not 0.  A pixel whose
    specular lobe is exactly 0 -- max(dot(E, R), 0) = 0, and pow(0, 20) is 0 on the host and on the device -- has no powf
    in its value: those pixels are held bit for bit, diffuse direct term included.  The whole frame is held to the
    criterion test_gpu_components.py holds the restatement to (relative L2 <= 1e-4, >= 99.9 % of the fp16 values equal),
    which is the restatement's own error: the two pow implementations differ in the last place for some arguments."""
    s = seeded
    planes = synth.random_gbuffer(W * H, seed=21, discard_frac=0.05)
    alive = ~(planes[18] < 0.5)
    E = np.abs(s["E"]) + np.float32(0.25)                # non-zero everywhere, of the frame's own magnitude or above
    with frame_ctx(vct, s, debug_outputs=1) as ctx:
        ctx.set_pixel_emission(E)
        got = ctx.trace(planes).reshape(-1, 4)
        comp = cr.composite(planes, ctx.cones(), CAM, LIGHT, s["p"].ambient_factor, s["p"].shininess)
        want = er.frame(comp["rgba32f"], planes, E)
        ctx.set_pixel_emission(None)
        plain = ctx.trace(planes).reshape(-1, 4)
    direct = comp["direct"]                              # (shadow * cos_theta, spec * shadow, shadow, 1) per pixel
    no_lobe = alive & (direct[:, 1] == 0) & (planes[22] > 0)
    lit_diffuse = no_lobe & (direct[:, 0] > 0)
    print(f"lit frame: {alive.sum()} live pixels, {no_lobe.sum()} without a specular lobe, {lit_diffuse.sum()} of them with a "
          f"diffuse direct term; fp16 values equal overall: {(got == want).mean():.5f}")
    assert no_lobe.sum() >= 500 and lit_diffuse.sum() >= 200
    assert np.array_equal(got[no_lobe], want[no_lobe])
    assert (got[alive, :3] != plain[alive, :3]).any(-1).all()                   # E reached every live pixel
    assert synth.rel_l2(vct.half_to_float(got), vct.half_to_float(want)) <= 1e-4
    assert (got == want).mean() >= 0.999
    assert np.array_equal(got[~alive], want[~alive])


def test_demo_emission_option(vct):
    """vct_demo --emission: the facade's SetEmission, its upload and re-voxelization in Render(); a bad list is refused."""
    exe = os.path.join(ROOT, "voxel-cone-tracing_amd", "vct_demo")
    base = [exe, "--scene", "procedural:cornell", "--voxels", "32", "--size", "64x48", "--shadow", "128", "--frames", "2"]

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, timeout=300)
    plain, lit_, again = run(), run("--emission", "1=3,0.25,0;3=0.5,0.5,1.75"), run("--emission", "1=0,0,0")
    for r in (plain, lit_, again):
        assert r.returncode == 0, r.stdout + r.stderr

    def checksum(r):
        line = [ln for ln in r.stdout.splitlines() if "fnv1a=" in ln]
        assert line, r.stdout
        return line[-1].split("fnv1a=")[1].split()[0]
    assert checksum(lit_) != checksum(plain)
    assert checksum(again) == checksum(plain)            # an all-zero table is no emission
    for bad in ("9=1,1,1", "1=1,1", "1=1,1,1,3=1,1,1", "x"):
        r = run("--emission", bad)
        assert r.returncode == 1 and "--emission" in r.stderr, (bad, r.stdout + r.stderr)
    neg = run("--emission", "1=-1,0,0")                  # the library's refusal reaches the caller
    assert neg.returncode != 0 and "vct_upload_emission" in neg.stdout, neg.stdout + neg.stderr


def test_row_slabs_and_rate_2(vct, seeded):
    s = seeded
    with frame_ctx(vct, s, debug_outputs=1) as ctx:
        ctx.set_pixel_emission(s["E"])
        whole = ctx.trace(s["planes"])
        cones = ctx.cones()
        assert np.array_equal(whole, want_frame(s, cones))
        # the three slabs of the frame equal the whole frame
        ctx.set_pixel_emission(None)
        cleared = ctx.trace(s["planes"])
        assert not np.array_equal(cleared, whole)
        ctx.set_pixel_emission(s["E"])
        for row0 in (0, 2, 4):
            ctx.trace_gbuffer_rows(row0, row0 + 2)
        assert np.array_equal(ctx.download_frame(), whole)
        # rate 2 on a screen-coherent G-buffer (most pixels interpolated): the rate-2 expectation plus E
        planes2 = drr.mixed_gbuffer(W, H)
        planes2[22] = 0.0
        alive2 = ~(planes2[18] < 0.5)
        ctx.set_pixel_emission(None)
        ctx.trace(planes2)
        ref = dict(cones=ctx.cones(), steps=ctx.steps())
        vs = np.float32(s["p"].G) / np.float32(V)
        r2 = drr.restate(planes2, W, H, vs, ref, CAM, LIGHT, s["p"].ambient_factor, s["p"].shininess)
        assert r2["cls"]["marched"].sum() < 0.6 * alive2.sum()
        ctx.set_diffuse_rate(2)
        assert np.array_equal(ctx.trace(planes2), er.frame(r2["rgba32f"], planes2, np.full_like(s["E"], -0.0)).reshape(H, W, 4))
        ctx.set_pixel_emission(s["E"])
        want2 = er.frame(r2["rgba32f"], planes2, s["E"]).reshape(H, W, 4)
        full = er.frame(cr.composite(planes2, ref["cones"], CAM, LIGHT, s["p"].ambient_factor, s["p"].shininess)["rgba32f"],
                        planes2, s["E"]).reshape(H, W, 4)
        assert not np.array_equal(want2, full)                        # rate 2 is not rate 1 here
        assert np.array_equal(ctx.trace(planes2), want2)


def test_two_frame_slots_keep_their_planes(vct, seeded):
    s = seeded
    E0, E1 = s["E"], (s["E"][::-1] * np.float32(0.5)).copy()
    with frame_ctx(vct, s, debug_outputs=1) as one:
        one.trace(s["planes"])
        cones = one.cones()
    want0, want1 = want_frame(s, cones, E=E0), want_frame(s, cones, E=E1)
    assert not np.array_equal(want0, want1)
    with frame_ctx(vct, s) as ctx:
        ctx.set_frames_in_flight(2)
        ctx.select_frame_slot(0)
        ctx.set_pixel_emission(E0)
        ctx.select_frame_slot(1)
        invalid(vct, ctx.download_pixel_emission)                    # the other slot's planes are its own
        ctx.set_pixel_emission(tiled(E1), vct.GB_TILED)
        for _ in range(2):
            ctx.select_frame_slot(0)
            f0 = ctx.trace(s["planes"])
            ctx.select_frame_slot(1)
            f1 = ctx.trace(s["planes"])
            assert np.array_equal(f0, want0) and np.array_equal(f1, want1)
        ctx.select_frame_slot(0)
        assert np.array_equal(ctx.download_pixel_emission().view(np.uint32), E0.view(np.uint32))
        ctx.set_frames_in_flight(1)
        assert np.array_equal(ctx.trace(s["planes"]), want0)


# ---- whole passes ------------------------------------------------------------------------------------------------------
def room_setup(oracle):
    from voxel_cone_tracing_amd import scene as sc
    room = er.Room()
    cam = sc.default_camera(**room.camera)
    light = (0.0, 1.0, 0.25)
    return sc, room, cam, light, sc.light_view_proj(light), sc.camera_view_proj(cam, W, H)


def test_gi_pass_equals_the_staged_calls(vct, oracle):
    sc, room, cam, light, lvp, vp = room_setup(oracle)
    S = 128
    depth, lvp_row = raster_oracle.shadow_map(sc, room, light, S)
    p = oracle.default_params(V, camera_pos=tuple(cam.position), light_dir=light)
    want, L, Em = er.level0(oracle, p, room.pos, room.material, room.albedo, room.emission, shadow_depth=depth, light_vp=lvp_row)
    assert L[..., :3].any() and Em[..., :3].any()
    planes = raster_oracle.gbuffer(sc, room, cam, W, H, depth, lvp_row)
    E = er.pixel_emission(planes, room.albedo, room.emission)
    assert E.any()
    cfg = dict(voxel_dim=V, width=W, height=H, shadow_map_size=S)
    with vct.Context(vct.default_config(**cfg)) as fused, vct.Context(vct.default_config(**cfg)) as ref:
        for c in (fused, ref):
            c.upload_scene(room)
            c.upload_emission(room.emission)
            c.set_camera_position(tuple(cam.position))
            c.set_light_direction(light)
        for _ in range(2):
            fused.gi_pass(lvp, vp)
            ref.render_shadow_map(lvp)
            ref.voxelize(); ref.inject_light(); ref.build_mips()
            ref.render_gbuffer(vp)
            ref.trace_resident()
            assert np.array_equal(ref.download_chain(), oracle.build_mips(want))
            assert np.array_equal(ref.download_pixel_emission().view(np.uint32), E.view(np.uint32))
            assert np.array_equal(fused.download_chain(), ref.download_chain())
            assert np.array_equal(fused.download_gbuffer().view(np.uint32), ref.download_gbuffer().view(np.uint32))
            assert np.array_equal(fused.download_pixel_emission().view(np.uint32), ref.download_pixel_emission().view(np.uint32))
            assert np.array_equal(fused.download_frame(), ref.download_frame())
            assert fused.last_step_count() == ref.last_step_count() > 0
        ref.upload_emission(None)                        # the frame did take the planes
        ref.render_gbuffer(vp)
        ref.trace_resident()
        assert not np.array_equal(fused.download_frame(), ref.download_frame())


def test_an_emissive_panel_lights_the_room(vct, oracle):
    """Nothing but the panel emits and the shadow map shadows everything: without the panel's emission the volume and the
    indirect diffuse output are black; with it the open half of the floor receives more than the half under the plate."""
    sc, room, cam, light, lvp, vp = room_setup(oracle)
    dark = np.zeros((64, 64), np.float32)
    lvp_row = lvp.reshape(4, 4).T.copy()
    planes = raster_oracle.gbuffer(sc, room, cam, W, H, dark, lvp_row)
    E = er.pixel_emission(planes, room.albedo, room.emission)
    floor = (planes[15:19].view(np.uint32) == room.albedo[room.FLOOR].view(np.uint32)[:, None]).all(0)
    under, open_ = floor & (planes[0] < -3.0), floor & (planes[0] > 3.0)
    panel = (E != 0).any(0)
    assert under.sum() >= 100 and open_.sum() >= 100 and panel.sum() >= 50 and not planes[22].any()
    with vct.Context(vct.default_config(voxel_dim=V, width=W, height=H, debug_outputs=1)) as ctx:
        ctx.upload_scene(room)                           # (takes the scene's emission along, as it takes Ke of an MTL file)
        ctx.upload_emission(None)
        ctx.upload_shadow_map(dark, lvp_row)
        ctx.set_camera_position(tuple(cam.position))
        ctx.set_light_direction(light)
        ctx.set_aov_outputs(cr.AOV_INDIRECT_DIFFUSE)
        chain = run_pass(ctx)
        assert (chain[: V ** 3, 3] > 0).mean() > 0.05 and not chain[..., :3].any()
        ctx.render_gbuffer(vp)
        assert np.array_equal(ctx.download_gbuffer().view(np.uint32), planes.view(np.uint32))
        ctx.trace_resident()
        assert not ctx.download_aov(cr.AOV_INDIRECT_DIFFUSE)[..., :3].any()
        ctx.upload_emission(room.emission)
        chain = run_pass(ctx)
        assert chain[: V ** 3, :3].any()
        ctx.render_gbuffer(vp)
        ctx.trace_resident()
        frame = ctx.download_frame().reshape(-1, 4)
        ind = vct.half_to_float(ctx.download_aov(cr.AOV_INDIRECT_DIFFUSE).reshape(-1, 4))[:, :3]
        m_under, m_open = float(ind[under].mean()), float(ind[open_].mean())
        print(f"indirect diffuse, mean over the floor: under the plate {m_under:.6f}, open {m_open:.6f}")
        assert m_open > m_under > 0.0
        assert np.array_equal(ctx.download_pixel_emission().view(np.uint32), E.view(np.uint32))
        p = oracle.default_params(V, camera_pos=tuple(cam.position), light_dir=light)
        rgba = cr.composite(planes, ctx.cones(), tuple(cam.position), light, p.ambient_factor, p.shininess)["rgba32f"]
        want = er.frame(rgba, planes, E)
        assert np.array_equal(frame[panel], want[panel])
        assert (vct.half_to_float(frame[panel])[:, 0] >= 2.0).all()      # the panel's red is its emission of 2 and more
        assert np.array_equal(frame, want)
