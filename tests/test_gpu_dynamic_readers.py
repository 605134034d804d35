"""GPU: the readers that include/vct.h says follow the dynamic mesh, with its three switches on (vct_set_dynamic_draw,
vct_set_dynamic_bounce, vct_set_dynamic_emission) -- part C of tests/test_gpu_dynamic_features.py's sweep.  Run here and
in no earlier file:

  - a rank context (vct_comm_init(.., 0, 1), then vct_gi_pass, vct_bounce, vct_trace_resident) with the mover drawn, glowing
    and bounced, against a single context
  - the pixel-lights kernel over a G-buffer that holds dynamic pixels
  - the half-rate diffuse gather and the per-component outputs over such a G-buffer: the flat per-face normals of adjacent
    dynamic triangles are what a quad's normal test has to split
  - directional chains and the voxel view over D' and over the bounced merged chain

Bit-equal to the CPU oracle, to the NumPy restatements or to a second context; the rate-2 frame goes through
tests/test_gpu_diffuse_rate.py's own comparison, unchanged.  Every test asserts, on the reference's output, the
non-degeneracy of what it compares."""
import numpy as np
import pytest

import components_ref as cr
import diffuse_rate_ref as dr
import dynbouncecases as db
import dyncases as dc
import dyndrawcases as ddc
import dynemiscases as de
import lights_ref as lr
import voxel_view_ref as vv
from test_gpu_diffuse_rate import ALL_AOV, _check_against_restatement
from test_gpu_dynamic import NONE, run_pass, shadow_maps, static_ctx
from test_gpu_dynamic_bounce import assert_bounced
from test_gpu_dynamic_draw import BOTH, assert_planes, bits, draw, make_ctx, upload_static, vct  # noqa: F401
from test_gpu_dynamic_emission import assert_pass

pytestmark = pytest.mark.gpu
V, G, MS = dc.V, dc.G, dc.MS
W, H = ddc.W, ddc.H


@pytest.fixture(scope="module")
def world(oracle):
    """dyncases' world at 64^3 without a shadow map: the layers, DEm and D' at A and B."""
    w = dict(static=dc.static_scene(), A=dc.dynamic_mesh(dc.A), B=dc.dynamic_mesh(dc.B), maps=shadow_maps())
    w["S", NONE] = dc.layer(oracle, *w["static"])
    for k in "AB":
        w[k, NONE] = dc.layer(oracle, *w[k])
        w[k, "D'"] = de.add(w[k, NONE][0], de.dem(oracle, w[k][0], w[k][1]))
    return w


# ---- a rank context -----------------------------------------------------------------------------------------------------------
def test_a_rank_context_draws_lights_and_bounces_the_mover(vct, oracle, world):
    from voxel_cone_tracing_amd import scene as sc
    w, h, S = 96, 64, ddc.SHADOW
    spos, smat, salb = world["static"]
    static = (spos, smat, salb, np.full((salb.shape[0], 3), 0.25, np.float32), ddc.static_frames(spos))
    light = (0.0, 1.0, 0.25)
    cam = sc.default_camera(position=(25.0, -17.0, 85.0))               # a camera that sees the object at A and at B
    vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(light)
    for k in "AB":
        cat = ddc.concatenated(static, world[k], ms=MS, grid=G)
        depth, planes = ddc.reference(oracle, cat, w, h, vp, lvp, ms=MS)
        planes_static = oracle.render_gbuffer(ddc.mesh_of(oracle, static, MS), vp, w, h, depth, lvp)
        assert (bits(planes) != bits(planes_static)).any(0).sum() >= 80, k

    def ctx_of(flags):
        c = vct.Context(dc.config(vct, width=w, height=h, shadow_map_size=S, debug_outputs=0))
        upload_static(c, static)
        c.set_dynamic_mesh(*world["A"])
        c.set_dynamic_draw(flags, ddc.SPECULAR)
        c.set_dynamic_emission(de.EM)
        c.set_dynamic_bounce(True)
        c.set_camera_position(tuple(cam.position)); c.set_light_direction(light)
        return c
    with ctx_of(BOTH) as single, ctx_of(BOTH) as rank, ctx_of(0) as undrawn:
        rank.comm_init(vct.comm_unique_id(), 0, 1)
        seen = []
        for k in "AB":
            for c in (single, rank, undrawn):
                c.update_dynamic_positions(world[k][0])
                c.gi_pass(lvp, vp)
            rank.comm_sync()
            want, got = single.download_frame(), rank.comm_download_frame()
            differ = int((want != undrawn.download_frame()).any(axis=2).sum())
            print(f"at {k}: {differ} of {w * h} pixels differ from the frame with the draw flags off")
            assert differ >= 50, (k, differ)
            assert np.array_equal(got, want), k
            assert np.array_equal(rank.download_chain(), single.download_chain()), k
            assert not np.array_equal(rank.download_chain(), undrawn.download_chain()), k      # the layer under the drawn map
            for a, b in zip(rank.download_dynamic_voxels(), single.download_dynamic_voxels()):
                assert a.any() and np.array_equal(a, b), k
            depth = single.download_shadow_map()
            assert np.array_equal(bits(rank.download_shadow_map()), bits(depth)), k
            assert (bits(depth) != bits(undrawn.download_shadow_map())).sum() >= 20, k
            em = single.download_pixel_emission()
            assert np.array_equal(bits(rank.download_pixel_emission()), bits(em)), k
            assert (em > 0).any(0).sum() >= 50 and not undrawn.download_pixel_emission().any(), k
            assert np.array_equal(bits(rank.download_gbuffer()), bits(single.download_gbuffer())), k
            seen.append(want)
        assert (seen[0] != seen[1]).any(axis=2).sum() >= 50
        for c in (single, rank):
            c.bounce()
            c.trace_resident()
        assert single.last_step_count() == rank.last_step_count() > 0
        assert np.array_equal(rank.download_chain(), single.download_chain())
        bounced = single.download_frame()
        assert np.array_equal(rank.download_frame(), bounced)
        assert (bounced != seen[1]).any(axis=2).sum() >= 50                 # the bounce shows in the frame
        rank.comm_destroy()


# ---- pixel lights over dynamic pixels -------------------------------------------------------------------------------------------
def test_pixel_lights_over_dynamic_pixels(vct, oracle):
    """Specular colours 0 on both meshes: the lit planes hold no powf and are compared bit for bit."""
    pos, mat, alb, spec, frames = ddc.static_mesh()
    static = (pos, mat, alb, np.zeros_like(spec), frames)
    dyn = ddc.object_mesh("A")
    depth, planes = ddc.reference(oracle, ddc.concatenated(static, dyn, specular=None), W, H)
    own = ddc.owner_is_dynamic(planes)
    lights = ddc.object_lights()
    cam = (0.0, 0.0, 0.0)
    lit = lr.lit_planes(planes, lights, cam, 20.0)
    per_light = [(lr.lit_planes(planes, [l], cam, 20.0) > 0).any(0) for l in lights]
    assert (lit[:, own] > 0).any(0).sum() >= 100 and (lit[:, ~own] > 0).any(0).sum() >= 100
    reach = [int((p & own).sum()) for p in per_light]
    assert sum(r >= 10 for r in reach) >= 4 and len(set(reach)) >= 4        # several lights reach the object, each its own part
    with make_ctx(vct, static, voxel_attributes=1) as ctx:
        ctx.set_camera_position(cam); ctx.set_light_direction((0.0, 1.0, 0.6))
        ctx.set_lights(lights)
        ctx.set_dynamic_mesh(*dyn)
        ctx.set_dynamic_draw(BOTH)
        for rnd in range(2):
            draw(ctx)
            run_pass(ctx)
            ctx.trace_resident()
            assert_planes(ctx, planes, f"pass {rnd}")
            got = ctx.download_pixel_lights()
            bad = np.argwhere((bits(got) != bits(lit)).any(0))
            assert bad.shape[0] == 0, (rnd, bad.shape[0], bad[:4].tolist())
        # the flag off: the lit planes of the room alone
        _, planes_s = ddc.reference(oracle, static, W, H)
        lit_s = lr.lit_planes(planes_s, lights, cam, 20.0)
        assert (bits(lit_s) != bits(lit)).any(0).sum() >= 300
        ctx.set_dynamic_draw(0)
        draw(ctx)
        ctx.trace_resident()
        assert np.array_equal(bits(ctx.download_pixel_lights()), bits(lit_s))


# ---- the half-rate gather and the outputs ---------------------------------------------------------------------------------------
def test_half_rate_gather_and_outputs_over_dynamic_pixels(vct, oracle):
    Vd, Gd = 64, 64.0                                  # one world unit per voxel: the room is a few dozen voxels wide
    cam, light = (0.0, 0.0, 0.0), (0.0, 1.0, 0.6)
    static, dyn = ddc.static_mesh(), ddc.object_mesh("A")
    _, planes = ddc.reference(oracle, ddc.concatenated(static, dyn), W, H)
    own = ddc.owner_is_dynamic(planes)
    vs = np.float32(Gd) / np.float32(Vd)
    cls = dr.classify(planes, W, H, vs)
    interp = cls["alive"] & ~cls["marched"]
    assert (cls["fill"] & own).sum() >= 20, (cls["fill"] & own).sum()       # dynamic pixels that march their own cones
    assert (interp & own).sum() >= 300 and (cls["anchor"] & own).sum() >= 300 and (interp & ~own).sum() >= 1000
    with make_ctx(vct, static, V=Vd, grid_world_size=Gd, voxel_attributes=1, debug_outputs=1) as ctx:
        ctx.set_camera_position(cam); ctx.set_light_direction(light)
        ctx.set_dynamic_mesh(*dyn)
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        draw(ctx)
        run_pass(ctx)
        assert_planes(ctx, planes, "the drawn planes")
        chain = ctx.download_chain()
        assert (chain[:Vd ** 3, 3] > 0).sum() >= 1000
        p = oracle.default_params(Vd, G=Gd, camera_pos=cam, light_dir=light)
        ref = oracle.trace(p, chain, planes, nthreads=8, want_cones=True)
        s = dict(planes=planes, w=W, h=H)
        ctx.set_diffuse_rate(2)
        # rate 2 alone: the frame against the restatement
        want = dr.restate(planes, W, H, vs, ref, cam, light, p.ambient_factor, p.shininess)
        assert (want["steps"][cls["fill"] & own, :6].astype(np.int64).sum(1) > 0).sum() >= 20
        ctx.trace_resident()
        _check_against_restatement(vct, ctx, s, want, "rate 2 over the drawn planes")
        resident = ctx.download_frame()
        assert np.array_equal(ctx.trace(ctx.download_gbuffer()), resident)
        assert ctx.last_step_count() < ref["total_steps"]                   # fewer steps than the full-rate trace
        # ... and with all three outputs
        ctx.set_aov_outputs(ALL_AOV)
        want = dr.restate(planes, W, H, vs, ref, cam, light, p.ambient_factor, p.shininess, cr.SHOW_ALL, ALL_AOV)
        ctx.trace_resident()
        _check_against_restatement(vct, ctx, s, want, "rate 2 with the outputs")
        frame = ctx.download_frame()
        aovs = {bit: ctx.download_aov(bit) for bit in (vct.AOV_INDIRECT_DIFFUSE, vct.AOV_INDIRECT_SPECULAR, vct.AOV_DIRECT)}
        assert np.array_equal(frame, resident)                              # the outputs do not change the frame
        assert np.array_equal(ctx.trace(ctx.download_gbuffer()), frame)
        for bit, a in aovs.items():
            assert np.array_equal(ctx.download_aov(bit), a), bit
            assert (a.reshape(-1, 4)[own] != 0).any(1).sum() >= 100, bit    # each output holds dynamic pixels


# ---- directional chains and the voxel view --------------------------------------------------------------------------------------
def test_directional_chains_and_the_voxel_view_over_the_emitting_bounced_chain(vct, oracle, world):
    from voxel_cone_tracing_amd import scene as sc
    w, h = 40, 24
    S3, D3, Dp = world["S", NONE], world["A", NONE], world["A", "D'"]
    l0 = dc.merge(Dp, S3[0])
    l1, steps = db.expected(oracle, D3, S3, l0=l0)
    plain = dc.merge(D3[0], S3[0])
    assert db.differing(l1, l0).sum() >= 2000 and db.differing(l0, plain).sum() >= 300
    an0, an1 = oracle.build_mips_aniso(l0), oracle.build_mips_aniso(l1)
    assert (an0 != an1).any(-1).sum() >= 1000 and (an0 != oracle.build_mips_aniso(plain)).any(-1).sum() >= 100
    m = sc.invert_matrix(sc.camera_view_proj(sc.default_camera(position=(5.0, 4.0, -3.0), yaw=30.0, pitch=12.0), w, h))
    with static_ctx(vct, world, anisotropic_mips=1, width=w, height=h) as ctx:
        ctx.set_dynamic_bounce(True)
        ctx.set_dynamic_mesh(*world["A"])
        ctx.set_dynamic_emission(de.EM)
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, S3[0], "bounce 0")
        assert np.array_equal(ctx.download_aniso(), an0), "directional chains of merge(D', S)"
        ctx.bounce()
        assert_bounced(oracle, ctx, l1, steps, "the bounce")
        assert np.array_equal(ctx.download_aniso(), an1), "directional chains of the bounced chain"
        chains = {vct.VOXVIEW_RADIANCE: oracle.build_mips(l0), vct.VOXVIEW_CURRENT: oracle.build_mips(l1)}
        for level in (0, 1):
            frames = {}
            for source, chain in chains.items():
                want = vv.half_bits(vv.view(vv.level_of(chain, V, level), m, w, h, ctx.cfg.grid_world_size, ctx.cfg.max_alpha))
                ctx.render_voxels(m, source, level)
                got = ctx.download_frame()
                assert int((got != want).any(axis=2).sum()) == 0, (source, level)
                frames[source] = want
            assert (frames[vct.VOXVIEW_RADIANCE] != frames[vct.VOXVIEW_CURRENT]).any(axis=2).sum() >= 50, level
