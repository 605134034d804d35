"""GPU: local lights (include/vct.h "local lights") -- k_light_voxels behind vct_inject_light and k_light_pixels in front
of every composite launch -- against tests/lights_ref.py, the fp32 numpy restatement of both.

Level 0 runs at V = 32 on voxcases.random_scene(300, 7) (tests/test_lights_restatement.py holds the counts that keep
these comparisons from passing vacuously), frames are 61 x 43 so that both edges are ragged (8 x 6 tiles).  Chains,
lit planes and frames are held bit for bit wherever no powf is involved: the G-buffers of those cases have specular
planes 0, so Ssum * 0 = +0 on both sides whatever powf returns.  The specular term itself is held to the criterion
tests/test_gpu_components.py holds its own powf term to (>= 99.9 % of the fp16 values equal), every other value
within one fp16 ulp."""
import numpy as np
import pytest

import components_ref as cr
import emission_ref as er
import gbcases
import lights_ref as lr
import point_query_ref as pq
import pqcases
import synth
import vctpkg
import voxcases
from test_gpu_parity import light_setup

pytestmark = pytest.mark.gpu

V, W, H, G = 32, 61, 43, 150.0
TX, TY = (W + 7) // 8, (H + 7) // 8
CAM, LIGHT = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)
NPIX = W * H


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


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_pass(ctx):
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    return ctx.download_chain()


def assert_chain(got, want, what=""):
    bad = np.argwhere((got[: V ** 3] != want[: V ** 3]).any(-1).reshape(V, V, V))
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:6].tolist())
    assert np.array_equal(got, want), what


# ---- level 0, chain, bounce, readers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vox(oracle):
    """random_scene(300, 7) under a 64^2 random-depth shadow map, flat and with one diffuse texture: the oracle's level 0
    and attributes, and the restated chains with lr.LIGHTS."""
    pos, mat, alb = voxcases.random_scene(300, 7)
    depth, vp = light_setup(64, 3)
    p = oracle.default_params(V)
    r = np.random.default_rng(11)
    tex = r.integers(0, 256, (8, 8, 4), dtype=np.uint8)
    tex[..., 3] = 255
    uv = r.uniform(0.0, 2.0, (pos.shape[0], 6)).astype(np.float32)
    mat_tex = np.full((5, 3), -1, np.int32)
    mat_tex[1, 0] = 0
    out = dict(pos=pos, mat=mat, alb=alb, depth=depth, vp=vp, p=p, uv=uv, tex=[tex], mat_tex=mat_tex)
    for name, kw in (("flat", {}), ("textured", dict(uv=uv, mat_tex=mat_tex, textures=[tex], mipmaps=True))):
        sc = oracle.make_scene(pos, mat, alb, shadow_depth=depth, light_vp=vp, **kw)
        l0, aa, an = oracle.voxelize_conservative_attr(p, sc)
        want = lr.level0(l0, aa, an, lr.LIGHTS, G)
        assert ((want != l0).any(-1)).sum() >= 200
        out[name] = dict(l0=l0, aa=aa, an=an, want=want, chain=oracle.build_mips(want), plain=oracle.build_mips(l0), kw=kw)
    assert not np.array_equal(out["flat"]["want"], out["textured"]["want"])
    return out


def vox_ctx(vct, vox, textured=False, w=8, h=8, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, voxel_attributes=1, **kw))
    ctx.upload_triangles(vox["pos"], vox["mat"], vox["alb"])
    if textured:
        ctx.upload_mesh_uvs(vox["uv"])
        ctx.upload_textures(vox["tex"], vox["mat_tex"])
    ctx.upload_shadow_map(vox["depth"], vox["vp"])
    return ctx


@pytest.mark.parametrize("kind", ["flat", "textured"])
def test_level0_and_chain(vct, vox, kind):
    f = vox[kind]
    with vox_ctx(vct, vox, textured=kind == "textured") as ctx:
        assert_chain(run_pass(ctx), f["plain"], "before any lights")
        ctx.set_lights(lr.LIGHTS)
        assert_chain(ctx.download_chain(), f["plain"], "attached, before the next pass")
        for k in range(2):                              # two passes in a row: the resolve rewrites what the lights changed
            assert_chain(run_pass(ctx), f["chain"], (kind, k))
            got_alb, got_nrm = ctx.voxel_attributes()
            assert np.array_equal(got_alb, f["aa"]) and np.array_equal(got_nrm, f["an"])
        ctx.set_lights(None)
        assert_chain(ctx.download_chain(), f["chain"], "detached, before the next pass")
        assert_chain(run_pass(ctx), f["plain"], "detached")
        got_alb, got_nrm = ctx.voxel_attributes()
        assert np.array_equal(got_alb, f["aa"]) and np.array_equal(got_nrm, f["an"])


def test_with_emission_attached(vct, oracle, vox):
    f = vox["flat"]
    lit0, L, Em = er.level0(oracle, vox["p"], vox["pos"], vox["mat"], vox["alb"], er.EMISSION, shadow_depth=vox["depth"], light_vp=vox["vp"])
    assert np.array_equal(L, f["l0"])
    want = lr.level0(lit0, f["aa"], f["an"], lr.LIGHTS, G)
    both = (Em[..., :3] > 0).any(-1) & (want != lit0).any(-1)
    assert both.sum() >= 20 and not np.array_equal(want, f["want"])  # voxels that take emission AND local light
    with vox_ctx(vct, vox) as ctx:
        ctx.upload_emission(er.EMISSION)
        ctx.set_lights(lr.LIGHTS)
        for k in range(2):
            assert_chain(run_pass(ctx), oracle.build_mips(want), k)
        ctx.set_lights([])
        assert_chain(run_pass(ctx), oracle.build_mips(lit0), "emission alone")


def test_multi_chunk_slots(vct, oracle):
    pos, mat, alb, ms, Gc, Vc = voxcases.whole_grid_and_a_crowded_brick()
    assert Vc == V and Gc == G
    depth, vp = light_setup(64, 3)
    p = oracle.default_params(V, G=Gc)
    l0, aa, an = oracle.voxelize_conservative_attr(p, oracle.make_scene(pos, mat, alb, ms, shadow_depth=depth, light_vp=vp))
    want = lr.level0(l0, aa, an, lr.LIGHTS, Gc)
    assert (want != l0).any(-1).sum() >= 200
    with vct.Context(vct.default_config(voxel_dim=V, width=8, height=8, model_scale=ms, grid_world_size=Gc, voxel_attributes=1)) as ctx:
        ctx.upload_triangles(pos, mat, alb)
        ctx.upload_shadow_map(depth, vp)
        counts = ctx.stage_counts()
        assert counts["vox_items"] > counts["accumulator_bricks"], counts      # a slot was cut into chunks
        ctx.set_lights(lr.LIGHTS)
        for k in range(2):
            assert_chain(run_pass(ctx), oracle.build_mips(want), k)
        ctx.set_lights(None)
        assert_chain(run_pass(ctx), oracle.build_mips(l0))


def test_64_lights(vct, oracle, vox):
    """The full table: every brick culls most of it, and for some brick slot light 0 is the only survivor."""
    f = vox["flat"]
    lights = lr.many_lights()
    cull = lr.brick_cull(lights, V, G)
    slots = lr.per_brick(f["aa"][..., 3] == 255)
    assert (slots & cull[..., 0] & (cull.sum(-1) == 1)).any()
    want = lr.level0(f["l0"], f["aa"], f["an"], lights, G)
    assert (want != f["l0"]).any(-1).sum() >= 100
    with vox_ctx(vct, vox) as ctx:
        ctx.set_lights(lights)
        got = ctx.lights()
        assert len(got) == 64 and bytes(got[63]) == bytes(ctx._light(lights[63]))
        assert_chain(run_pass(ctx), oracle.build_mips(want))
        ctx.set_lights(lights[:1])                      # a shorter table: the tail is gone
        assert len(ctx.lights()) == 1
        assert_chain(run_pass(ctx), oracle.build_mips(lr.level0(f["l0"], f["aa"], f["an"], lights[:1], G)))


def test_bounce_and_point_queries_read_the_lit_chain(vct, oracle, vox):
    f, p = vox["flat"], vox["p"]
    want_l1, want_steps = oracle.bounce(p, f["chain"], f["aa"], f["an"], nthreads=8)
    plain_l1, _ = oracle.bounce(p, f["plain"], f["aa"], f["an"], nthreads=8)
    assert want_steps > 0 and not np.array_equal(want_l1, plain_l1)
    pts = pqcases.scatter(96, seed=5)
    ref = pq.gather(oracle, p, f["chain"], pts)
    ref_plain = pq.gather(oracle, p, f["plain"], pts)
    assert not np.array_equal(u32(ref["gather"]), u32(ref_plain["gather"]))
    with vox_ctx(vct, vox) as ctx:
        ctx.set_lights(lr.LIGHTS)
        assert_chain(run_pass(ctx), f["chain"])
        pq.assert_floats_match(ctx.gather_points(pts), ref["gather"], "gather on the lit chain")
        ctx.bounce()
        assert ctx.last_step_count() == want_steps
        assert_chain(ctx.download_chain(), oracle.build_mips(want_l1), "bounce")


# ---- the lit planes -----------------------------------------------------------------------------------------------------
def pixel_lights():
    """Lights for synth.random_gbuffer's positions (uniform in [-70, 70]^3): each reaches part of the frame only."""
    return [lr.point((10.0, 0.0, -20.0), (400.0, 300.0, 200.0), 60.0, 2.0),
            lr.spot((-40.0, 30.0, 20.0), (900.0, 900.0, 500.0), 80.0, 1.5, (1.0, -0.5, -0.3), 0.9, 0.3),
            lr.point((50.0, -50.0, 50.0), (50.0, 100.0, 150.0), 35.0, 1.0),
            lr.spot((0.0, -60.0, -50.0), (200.0, 500.0, 800.0), 70.0, 2.5, (0.1, 0.8, 0.6), 0.7, 0.2)]


@pytest.fixture(scope="module")
def seeded(oracle):
    chain = oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.06))
    planes = synth.random_gbuffer(NPIX, seed=21, discard_frac=0.05)
    planes[22] = 0.0                                    # every pixel in shadow: no powf in the composite's direct term
    planes[19:22] = 0.0                                 # specular planes 0: no powf in the lit planes
    r = np.random.default_rng(8)
    E = (r.normal(size=(3, NPIX)) * r.choice([0.0, 0.5, 3.0, 1e4], size=(1, NPIX))).astype(np.float32)
    alive = ~(planes[18] < 0.5)
    p = oracle.default_params(V, camera_pos=CAM, light_dir=LIGHT)
    lights = pixel_lights()
    lit = lr.lit_planes(planes, lights, CAM, p.shininess)
    assert 0.02 < (~alive).mean() < 0.1
    assert (lit[:, alive] > 0).any(0).sum() >= 500 and (lit[:, alive] == 0).all(0).sum() >= 100      # lit and unlit live pixels
    return dict(chain=chain, planes=planes, E=E, alive=alive, p=p, lights=lights, lit=lit,
                lit_E=lr.lit_planes(planes, lights, CAM, p.shininess, E=E))


def frame_ctx(vct, s, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=W, height=H, voxel_attributes=1, **kw))
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    ctx.upload_chain(s["chain"])
    return ctx


def rows_mask(row0, row1):
    y = np.arange(NPIX) // W
    return (y >= row0 * 8) & (y < row1 * 8)


def test_lit_planes_with_and_without_emission_and_masks(vct, seeded):
    s = seeded
    with frame_ctx(vct, s) as ctx:
        ctx.set_lights(s["lights"])
        assert not ctx.cfg.trace_variant
        invalid(vct, ctx.download_pixel_lights)                      # before the slot's first composite launch
        ctx.trace(s["planes"])
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(s["lit"]))
        ctx.set_pixel_emission(s["E"])
        ctx.trace(s["planes"])
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(s["lit_E"]))
        assert np.array_equal(u32(ctx.download_pixel_emission()), u32(s["E"]))      # the slot's own planes are untouched
        ctx.set_lighting_components(cr.SHOW_ALL & ~cr.SHOW_DIFFUSE)
        ctx.trace(s["planes"])
        want = lr.lit_planes(s["planes"], s["lights"], CAM, s["p"].shininess, mask=cr.SHOW_ALL & ~cr.SHOW_DIFFUSE, E=s["E"])
        assert np.array_equal(want[:, s["alive"]], s["E"][:, s["alive"]])            # E + 0
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(want))
        ctx.set_lighting_components(cr.SHOW_ALL)
        ctx.set_pixel_emission(None)
        ctx.trace(s["planes"])
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(s["lit"]))


def test_lit_planes_follow_every_gbuffer_hand_over(vct, seeded):
    import torch
    s = seeded
    tiled, in_frame = gbcases.to_tiled(s["planes"], W, H)
    poisoned = gbcases.poison_padding(tiled, in_frame)               # lanes outside the ragged frame hold NaN, inf, 3e38
    other = synth.random_gbuffer(NPIX, seed=5, discard_frac=0.05)
    other[19:22] = 0.0
    lit_other = lr.lit_planes(other, s["lights"], CAM, s["p"].shininess)
    assert not np.array_equal(u32(lit_other), u32(s["lit"]))
    dev = torch.from_numpy(poisoned).cuda()
    with frame_ctx(vct, s) as ctx:
        ctx.set_lights(s["lights"])
        for what, arg, layout in (("host linear", s["planes"], vct.GB_LINEAR), ("host tiled", poisoned, vct.GB_TILED),
                                  ("device tiled, zero-copy", dev.data_ptr(), vct.GB_TILED)):
            ctx.trace(other)
            assert np.array_equal(u32(ctx.download_pixel_lights()), u32(lit_other)), what
            if isinstance(arg, int):
                out = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
                ctx.trace(arg, layout=layout, out_device_ptr=out.data_ptr())
                ctx.synchronize()
            else:
                ctx.trace(arg, layout=layout)
            assert np.array_equal(u32(ctx.download_pixel_lights()), u32(s["lit"])), what
        # slab and resident rows: rows outside the range keep what they held
        ctx.trace(other)
        ctx.trace(s["planes"], rows=(1, 3))
        m = rows_mask(1, 3)
        got = ctx.download_pixel_lights()
        assert np.array_equal(u32(got[:, m]), u32(s["lit"][:, m])) and np.array_equal(u32(got[:, ~m]), u32(lit_other[:, ~m]))
        ctx.trace_gbuffer_rows(4, TY)                                # the ragged last tile row, of the resident G-buffer
        m2 = rows_mask(4, TY)
        got = ctx.download_pixel_lights()
        assert np.array_equal(u32(got[:, m | m2]), u32(s["lit"][:, m | m2]))
        assert np.array_equal(u32(got[:, ~(m | m2)]), u32(lit_other[:, ~(m | m2)]))
        ctx.trace_gbuffer_strided(0, TY, 2)                          # a strided launch may fill every row of its range
        got = ctx.download_pixel_lights()
        even = np.zeros(NPIX, bool)
        for r0 in range(0, TY, 2):
            even |= rows_mask(r0, r0 + 1)
        assert np.array_equal(u32(got[:, even | m | m2]), u32(s["lit"][:, even | m | m2]))
        ctx.trace_current()
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(s["lit"]))


def test_lit_planes_on_the_second_slot_at_rate_2_and_after_an_import(vct, seeded):
    s = seeded
    with frame_ctx(vct, s) as ctx:
        ctx.set_lights(s["lights"])
        ctx.set_frames_in_flight(2)                                  # a later second slot gets lit planes of its own
        ctx.select_frame_slot(1)
        invalid(vct, ctx.download_pixel_lights)
        ctx.set_pixel_emission(s["E"])
        ctx.trace(s["planes"])
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(s["lit_E"]))
        ctx.select_frame_slot(0)
        invalid(vct, ctx.download_pixel_lights)                      # slot 0 has launched nothing
        ctx.trace(s["planes"])
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(s["lit"]))
        ctx.select_frame_slot(1)
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(s["lit_E"]))
        ctx.select_frame_slot(0)
        ctx.set_frames_in_flight(1)
        ctx.set_diffuse_rate(2)
        other = synth.random_gbuffer(NPIX, seed=5, discard_frac=0.05)
        other[19:22] = 0.0
        ctx.trace(other)
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(lr.lit_planes(other, s["lights"], CAM, s["p"].shininess)))
        ctx.set_diffuse_rate(1)
        # an import writes the slot's own tiled buffer: the lit planes are of what it wrote
        g = s["planes"]
        albedo = np.ascontiguousarray(g[15:19].T)
        ctx.import_gbuffer(np.ascontiguousarray(g[0:3].T), np.ascontiguousarray(g[12:15].T), albedo,
                           specular=np.zeros((NPIX, 4), np.float32), shadow=np.zeros(NPIX, np.float32))
        ctx.trace_current()
        imported = ctx.download_gbuffer()
        assert np.array_equal(u32(imported[0:3]), u32(g[0:3])) and not imported[19:22].any()
        want = lr.lit_planes(imported, s["lights"], CAM, s["p"].shininess)
        assert (want != 0).any()
        assert np.array_equal(u32(ctx.download_pixel_lights()), u32(want))


def test_frame_bit_for_bit(vct, seeded):
    """The emitter-only set-up of test_gpu_emission.py (shadow plane 0, specular planes 0): the frame is the restated
    composite with E + Lit in the place of E."""
    s = seeded
    with frame_ctx(vct, s, debug_outputs=1) as ctx:
        plain = ctx.trace(s["planes"])
        cones = ctx.cones()
        rgba = cr.composite(s["planes"], cones, CAM, LIGHT, s["p"].ambient_factor, s["p"].shininess)["rgba32f"]
        assert np.array_equal(plain.reshape(-1, 4), er.frame(rgba, s["planes"], np.full_like(s["E"], -0.0)))
        ctx.set_lights(s["lights"])
        got = ctx.trace(s["planes"])
        assert np.array_equal(ctx.cones(), cones)
        want = er.frame(rgba, s["planes"], s["lit"]).reshape(H, W, 4)
        assert (want[..., :3] != plain[..., :3]).any(-1).reshape(-1)[s["alive"]].mean() > 0.2
        assert np.array_equal(got, want)
        ctx.set_pixel_emission(s["E"])
        assert np.array_equal(ctx.trace(s["planes"]), er.frame(rgba, s["planes"], s["lit_E"]).reshape(H, W, 4))
        for mask in (cr.SHOW_DIFFUSE | cr.SHOW_INDIRECT_SPECULAR, cr.SHOW_INDIRECT_DIFFUSE | cr.SHOW_AMBIENT_OCCLUSION):
            ctx.set_lighting_components(mask)
            got = ctx.trace(s["planes"])
            rgba_m = cr.composite(s["planes"], ctx.cones(), CAM, LIGHT, s["p"].ambient_factor, s["p"].shininess, mask)["rgba32f"]
            lit_m = lr.lit_planes(s["planes"], s["lights"], CAM, s["p"].shininess, mask=mask, E=s["E"])
            assert np.array_equal(got, er.frame(rgba_m, s["planes"], lit_m).reshape(H, W, 4)), mask
        ctx.set_lighting_components(cr.SHOW_ALL)
        ctx.set_pixel_emission(None)
        ctx.set_lights(None)
        assert np.array_equal(ctx.trace(s["planes"]), plain)


def f16_ulps(a, b):
    """|a - b| in fp16 ulps of the bit patterns, for non-negative values."""
    return np.abs(cr.to_f16_bits(a).astype(np.int32) - cr.to_f16_bits(b).astype(np.int32))


def test_specular_term(vct, seeded):
    """Non-zero specular planes, shininess 20 and two gloss classes: the planes rounded to fp16 against the restatement
    (numpy's pow against the device's powf), by the share test_gpu_components.py asks of its own powf term; every value
    that differs is within one fp16 ulp."""
    s = seeded
    planes = synth.random_gbuffer(NPIX, seed=21, discard_frac=0.05)
    alive = ~(planes[18] < 0.5)
    classes = [(0.07, 20.0), (0.105, 6.0)]
    plane = ((np.arange(NPIX) // 3) % 3).astype(np.uint8)            # classes 0, 1 and a byte beyond the table (-> class 0)
    with frame_ctx(vct, s) as ctx:
        assert ctx.cfg.shininess == 20.0
        ctx.set_lights(s["lights"])
        for what, shin in (("config.shininess", 20.0), ("gloss classes", lr.class_shininess(plane, classes))):
            if what == "gloss classes":
                ctx.set_gloss_classes(classes)
                ctx.set_pixel_gloss(plane)
            ctx.trace(planes)
            got = ctx.download_pixel_lights()
            want = lr.lit_planes(planes, s["lights"], CAM, shin)
            diffuse_only = lr.lit_planes(planes, s["lights"], CAM, shin, mask=cr.SHOW_ALL & ~cr.SHOW_SPECULAR)
            has_spec = (want != diffuse_only)[:, alive]
            assert (got >= 0).all() and np.isfinite(got).all() and has_spec.any(0).sum() >= 300, what
            d = f16_ulps(got, want)
            print(f"{what}: fp16 values equal {(d == 0).mean():.5f}, max {d.max()} ulp; fp32 bits equal {(u32(got) == u32(want)).mean():.5f}")
            assert (d == 0).mean() >= 0.999, what
            assert d.max() <= 1, what
            assert not got[:, ~alive].any()
        uniform = lr.lit_planes(planes, s["lights"], CAM, 20.0)
        assert not np.array_equal(cr.to_f16_bits(uniform), cr.to_f16_bits(want))      # the classes did change the exponent


# ---- contract -----------------------------------------------------------------------------------------------------------
def test_contract(vct, vox, seeded):
    f = vox["flat"]
    good = lr.LIGHTS

    def edited(j, **kw):
        out = [dict(l) for l in good]
        out[j].update(kw)
        return out
    bad_tables = [
        edited(0, radius=0.0), edited(0, radius=-1.0), edited(2, source_radius=0.0), edited(0, color=(1.0, -1e-30, 0.0)),
        edited(0, position=(np.nan, 0.0, 0.0)), edited(0, radius=np.inf), edited(2, color=(0.0, np.inf, 0.0)),
        edited(0, direction=(0.0, np.nan, 0.0)), edited(0, cos_inner=np.nan),
        edited(1, direction=(0.0, 0.0, 0.0)), edited(1, cos_outer=0.92), edited(1, cos_outer=0.95), edited(1, cos_outer=-1.5),
        edited(3, cos_inner=1.25), edited(0, flags=2), edited(1, flags=5),
    ]
    with vox_ctx(vct, vox, w=W, h=H) as ctx:
        ctx.set_lights(good)
        given = [bytes(l) for l in ctx.lights()]
        assert given == [bytes(ctx._light(l)) for l in good]
        assert_chain(run_pass(ctx), f["chain"])
        for k, table in enumerate(bad_tables):
            invalid(vct, ctx.set_lights, table)
            assert [bytes(l) for l in ctx.lights()] == given, k
        with pytest.raises(vct.VctError):
            ctx.set_lights(lr.many_lights() + good[:1])              # 65 lights
        L = vct.lib()
        arr = (vct.Light * 1)(ctx._light(good[0]))
        import ctypes as C
        assert L.vct_set_lights(ctx._h, C.cast(arr, C.c_void_p), -1) == -1
        assert L.vct_set_lights(ctx._h, C.cast(arr, C.c_void_p), 65) == -1
        assert [bytes(l) for l in ctx.lights()] == given
        assert_chain(run_pass(ctx), f["chain"], "the context kept what it had")
        invalid(vct, ctx.voxelize, vct.VOX_REFERENCE)                # the shaders as written have no local lights
        assert_chain(run_pass(ctx), f["chain"], "after reference mode was refused")
        for variant in (1, 2, 3, 4):
            invalid(vct, ctx.set_trace_variant, variant)
        # timing: two positive values with trace timing on, refused with it off
        invalid(vct, ctx.last_lights_ms)                             # no composite launch yet
        ctx.trace(seeded["planes"])
        ms = ctx.last_lights_ms()
        assert ms[0] > 0 and ms[1] > 0, ms
        print(f"V = {V}, {W} x {H}, 4 lights: voxel kernel {ms[0]:.4f} ms, pixel kernel {ms[1]:.4f} ms")
        ctx.set_trace_timing(False)
        run_pass(ctx)
        ctx.trace(seeded["planes"])
        invalid(vct, ctx.last_lights_ms)
        ctx.set_trace_timing(True)
        ctx.set_lights(None)
        assert ctx.lights() == []
        invalid(vct, ctx.download_pixel_lights)
        invalid(vct, ctx.last_lights_ms)
        ctx.voxelize(vct.VOX_REFERENCE)                              # detached: reference mode works again
        ctx.inject_light(); ctx.build_mips()
        for variant in (1, 2, 3, 4):
            ctx.set_trace_variant(variant)
            invalid(vct, ctx.set_lights, good)
        ctx.set_trace_variant(0)
        assert_chain(run_pass(ctx), f["plain"], "after the refusals")
    with vct.Context(vct.default_config(voxel_dim=V, width=8, height=8)) as ctx:      # config.voxel_attributes = 0
        invalid(vct, ctx.set_lights, good)
        assert ctx.lights() == []


def test_demo_light_option(vct):
    """vct_demo --light: the facade's SetLights, its hand-over and the re-voxelization in Render()."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "voxel-cone-tracing_amd", "vct_demo")
    base = [exe, "--scene", "procedural:cornell", "--voxels", "32", "--size", "64x48", "--shadow", "128", "--frames", "2"]

    def run(*extra):
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        line = [ln for ln in r.stdout.splitlines() if "fnv1a=" in ln]
        assert line, r.stdout
        return line[-1].split("fnv1a=")[1].split()[0]
    plain = run()
    lamp = run("--light", "0,8,0;400,300,200;60;0.5")
    both = run("--light", "0,8,0;400,300,200;60;0.5", "--light", "10,0,20;0,300,600;50;1;0,-1,-0.5;20;40")
    assert lamp != plain and both != lamp and both != plain


def test_detached_is_untouched(vct, oracle):
    """attach -> detach, then a full vct_gi_pass: chain, frame and step count are those of a context that never had
    lights, and the march form reported is the same."""
    from voxel_cone_tracing_amd import scene as sc
    room = er.Room()
    cam = sc.default_camera(**room.camera)
    light = (0.0, 1.0, 0.25)
    lvp, vp = sc.light_view_proj(light), sc.camera_view_proj(cam, W, H)
    cfg = dict(voxel_dim=V, width=W, height=H, shadow_map_size=128, voxel_attributes=1)
    room_lights = [lr.point((0.0, -20.0, 10.0), (300.0, 200.0, 100.0), 50.0, 2.0),
                   lr.spot((20.0, 0.0, -20.0), (500.0, 500.0, 500.0), 60.0, 1.0, (0.0, -1.0, 0.2), 0.9, 0.5)]
    with vct.Context(vct.default_config(**cfg)) as fresh, vct.Context(vct.default_config(**cfg)) as ctx:
        for c in (fresh, ctx):
            c.upload_scene(room)
            c.upload_emission(None)
            c.set_camera_position(tuple(cam.position))
            c.set_light_direction(light)
        fresh.gi_pass(lvp, vp)
        ctx.set_lights(room_lights)
        ctx.gi_pass(lvp, vp)
        lit_chain, lit_frame = ctx.download_chain(), ctx.download_frame()
        assert not np.array_equal(lit_chain, fresh.download_chain()) and not np.array_equal(lit_frame, fresh.download_frame())
        assert ctx.download_pixel_lights().any()
        ctx.set_lights(None)
        ctx.gi_pass(lvp, vp)
        assert np.array_equal(ctx.download_chain(), fresh.download_chain())
        assert np.array_equal(ctx.download_frame(), fresh.download_frame())
        assert ctx.last_step_count() == fresh.last_step_count() > 0
        assert ctx.stage_counts()["march_division"] == fresh.stage_counts()["march_division"]
        assert np.array_equal(u32(ctx.download_gbuffer()), u32(fresh.download_gbuffer()))
