"""GPU: the dynamic mesh's emission (include/vct.h "dynamic mesh", Emission; vct_set_dynamic_emission) -- a moving area
light in the chain and the frame -- bit-equal to the CPU oracle.  With D the layer as tests/test_gpu_dynamic.py holds it
and DEm = oracle.voxelize_conservative(dynamic mesh, pad4(table), no shadow map):

    D' = min(255, D + DEm) per byte, alpha D's        level 0 = where(D.a > 0, D', S)        download_dynamic_voxels[0] = D'

Scenes, table and their non-degeneracy in tests/dyncases.py and tests/dynemiscases.py (checked without a GPU by
tests/test_dynamic_emission_cases.py); the draw tests use tests/dyndrawcases.py's room and its two frame sizes.  Grid 64^3,
frames 8 x 8 except in the draw tests.  Every comparison is bit-equal: no tolerance is involved."""
import numpy as np
import pytest

import dyncases as dc
import dynbouncecases as db
import dyndrawcases as ddc
import dynemiscases as de
import emission_ref
import lights_ref as lr
import point_query_ref as pq
import synth
import vctpkg
from test_gpu_dynamic import ISSUE, NONE, RAISED, assert_chain, nbricks, run_pass, shadow_maps, static_ctx

pytestmark = pytest.mark.gpu
V, G, MS = dc.V, dc.G, dc.MS
EM = de.EM


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


@pytest.fixture(scope="module")
def world(oracle):
    """The static scene, the object at A and B, every layer under each shadow map, DEm (formed without a map) and D'."""
    w = dict(static=dc.static_scene(), A=dc.dynamic_mesh(dc.A), B=dc.dynamic_mesh(dc.B), maps=shadow_maps())
    for k in "AB":
        w[k, "DEm"] = de.dem(oracle, w[k][0], w[k][1])
    for sh, (depth, vp) in w["maps"].items():
        w["S", sh] = dc.layer(oracle, *w["static"], depth=depth, vp=vp)
        for k in "AB":
            w[k, sh] = dc.layer(oracle, *w[k], depth=depth, vp=vp)
            w[k, sh, "D'"] = de.add(w[k, sh][0], w[k, "DEm"])
    for k in "AB":
        de.assert_non_degenerate(w[k, NONE][0], w[k, "DEm"])
        dc.assert_non_degenerate(w[k, NONE, "D'"], w["S", NONE][0])
    return w


def assert_radiance(ctx, want, what):
    got = ctx.download_dynamic_voxels()[0]
    bad = np.argwhere((got != want).any(-1))
    assert bad.shape[0] == 0, (what, "layer radiance", bad.shape[0], bad[:4].tolist(),
                               got[tuple(bad[0])].tolist() if bad.shape[0] else None, want[tuple(bad[0])].tolist() if bad.shape[0] else None)


def assert_pass(oracle, ctx, Dp, S, what):
    assert_radiance(ctx, Dp, what)
    assert_chain(oracle, ctx, dc.merge(Dp, S), what)


def lit_ctx(vct, world, k="A", shadow=NONE, table=EM, **kw):
    """A context with the static scene, the object at k and the table attached."""
    ctx = static_ctx(vct, world, shadow, **kw)
    ctx.set_dynamic_mesh(*world[k])
    ctx.set_dynamic_emission(table)
    return ctx


def refused(vct, call, *a, **kw):
    with pytest.raises(vct.VctError) as e:
        call(*a, **kw)
    assert "(-1)" in str(e.value), str(e.value)               # VCT_ERR_INVALID
    return str(e.value)


# ---- 1. the layer and the chain -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", [1, 0])
@pytest.mark.parametrize("with_shadow", [NONE, ISSUE, RAISED])
def test_layer_and_chain(vct, oracle, world, with_shadow, attributes):
    S, D, Dp = world["S", with_shadow][0], world["A", with_shadow], world["A", with_shadow, "D'"]
    assert (Dp != D[0]).any(-1).sum() >= 300
    with lit_ctx(vct, world, "A", with_shadow, voxel_attributes=attributes) as ctx:
        assert np.array_equal(ctx.dynamic_emission(), EM)
        for rnd in range(2):                                      # the second pass starts from cleared sums
            run_pass(ctx)
            assert_pass(oracle, ctx, Dp, S, f"A, shadow={with_shadow}, attributes={attributes}, pass {rnd}")
            info = ctx.dynamic_info()
            assert info["bricks_used"] == nbricks(D[0]) and info["left_out"] == 0, info
        if attributes:                                            # albedo and normal are the layer's, untouched by the table
            got = ctx.download_dynamic_voxels()
            assert np.array_equal(got[1], D[1]) and np.array_equal(got[2], D[2])
        t_vox, t_merge = ctx.last_dynamic_ms()
        print(f"with the table: dynamic kernels {t_vox:.4f} ms, merge {t_merge:.4f} ms")
        # a table on one material only
        ctx.set_dynamic_emission(de.ONE)
        run_pass(ctx)
        one = de.add(D[0], de.dem(oracle, world["A"][0], world["A"][1], de.ONE))
        assert (one != Dp).any(-1).sum() >= 100 and (one != D[0]).any(-1).sum() >= 100
        assert_pass(oracle, ctx, one, S, "material 2 alone")


# ---- 2. accumulator hygiene ---------------------------------------------------------------------------------------------------
def test_moving_reuses_slots_with_clean_sums(vct, oracle, world):
    S = world["S", RAISED][0]
    with lit_ctx(vct, world, "A", RAISED) as ctx:
        for k in "ABA":
            ctx.update_dynamic_positions(world[k][0])
            run_pass(ctx)
            assert_pass(oracle, ctx, world[k, RAISED, "D'"], S, f"at {k}")


def test_a_discarded_pass_leaves_no_sums(vct, oracle, world):
    """vct_voxelize twice, one vct_inject_light: the first pass is discarded.  Sums it left would double DEm while the
    fragment count does not double."""
    S = world["S", NONE][0]
    with lit_ctx(vct, world, "A") as ctx:
        ctx.voxelize()
        run_pass(ctx)
        assert_pass(oracle, ctx, world["A", NONE, "D'"], S, "after a discarded pass")
        ctx.voxelize()                                              # discarded at B, resolved at A
        ctx.update_dynamic_positions(world["B"][0])
        ctx.voxelize()
        ctx.voxelize()
        ctx.update_dynamic_positions(world["A"][0])
        run_pass(ctx)
        assert_pass(oracle, ctx, world["A", NONE, "D'"], S, "after three discarded passes at two positions")


def test_a_pass_short_of_capacity_adds_nothing(vct, oracle, world):
    S, DA = world["S", NONE][0], world["A", NONE][0]
    need = nbricks(DA)
    pos, mat, alb = world["A"]
    # the same object at half its size around A: fewer bricks, so that it fits a layer one brick short of A's need
    small = (np.asarray(dc.A, np.float64)[None, None, :] + 0.5 * dc.offsets()).astype(np.float32).reshape(-1, 9)
    Ds = dc.layer(oracle, small, mat, alb)[0]
    Dsp = de.add(Ds, de.dem(oracle, small, mat))
    assert 1 <= nbricks(Ds) <= need - 1 and (Dsp != Ds).any(-1).sum() >= 50
    with static_ctx(vct, world) as ctx:
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=need - 1)
        ctx.set_dynamic_emission(EM)
        for rnd in range(2):
            run_pass(ctx)
            assert_chain(oracle, ctx, S, f"left out, pass {rnd}")
            assert_radiance(ctx, np.zeros_like(DA), f"left out, pass {rnd}")
            info = ctx.dynamic_info()
            assert (info["bricks_needed"], info["bricks_used"], info["left_out"]) == (need, 0, 1), info
        ctx.update_dynamic_positions(small)
        run_pass(ctx)
        assert_pass(oracle, ctx, Dsp, S, "within capacity after a pass that was left out")
        ctx.update_dynamic_positions(pos)                          # left out behind a resolved pass, and back
        run_pass(ctx)
        assert_chain(oracle, ctx, S, "left out again")
        ctx.update_dynamic_positions(small)
        run_pass(ctx)
        assert_pass(oracle, ctx, Dsp, S, "within capacity again")


def test_detach_and_the_table_between_voxelize_and_inject(vct, oracle, world):
    S, D, Dp = world["S", NONE][0], world["A", NONE][0], world["A", NONE, "D'"]
    one = de.add(D, de.dem(oracle, world["A"][0], world["A"][1], de.ONE))
    with lit_ctx(vct, world, "A") as ctx:
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, S, "attached")
        ctx.set_dynamic_emission(None)                             # a detach restores merge(D, S)
        assert ctx.dynamic_emission() is None
        run_pass(ctx)
        assert_pass(oracle, ctx, D, S, "detached")
        ctx.set_dynamic_emission(np.zeros((3, 3), np.float32))     # an all-zero table is a detach
        assert ctx.dynamic_emission() is None
        # attached between vct_voxelize and vct_inject_light: that pass has no dynamic emission, the next has
        ctx.voxelize()
        ctx.set_dynamic_emission(EM)
        ctx.inject_light(); ctx.build_mips()
        assert_pass(oracle, ctx, D, S, "attached behind the voxelize")
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, S, "the pass after the attach")
        # detached in between: none either; the sums of that pass are gone with the table
        ctx.voxelize()
        ctx.set_dynamic_emission(None)
        ctx.inject_light(); ctx.build_mips()
        assert_pass(oracle, ctx, D, S, "detached behind the voxelize")
        ctx.set_dynamic_emission(EM)
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, S, "attached again")
        # replaced in between: the pass resolves with the table it was voxelized under, the next with the new one
        ctx.voxelize()
        ctx.set_dynamic_emission(de.ONE)
        ctx.inject_light(); ctx.build_mips()
        assert_pass(oracle, ctx, Dp, S, "replaced behind the voxelize")
        run_pass(ctx)
        assert_pass(oracle, ctx, one, S, "the pass after the replacement")
        # detached, then attached, in between: fresh sums, no emission in that pass
        ctx.voxelize()
        ctx.set_dynamic_emission(None)
        ctx.set_dynamic_emission(EM)
        ctx.inject_light(); ctx.build_mips()
        assert_pass(oracle, ctx, D, S, "detached and attached behind the voxelize")
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, S, "and the pass after")


# ---- 3. many big triangles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", [1, 0])
def test_more_big_triangles_than_workgroups_with_the_table(vct, oracle, world, attributes):
    """k_dyn_big's EMIS form over more triangles than it has workgroups, all 512 bricks claimed."""
    S = world["S", NONE][0]
    pos, mat, alb = dc.big_triangles()
    assert int((dc.box_candidates(pos) > dc.VOX_BIG).sum()) > 512
    D = dc.layer(oracle, pos, mat, alb)[0]
    DEm = de.dem(oracle, pos, mat)
    n = de.non_degeneracy(D, DEm)
    assert n["saturating"] >= 100 and n["both"] >= 100 and n["mixed_values"] >= 5 and nbricks(D) == 512, n
    Dp = de.add(D, DEm)
    with static_ctx(vct, world, voxel_attributes=attributes) as ctx:
        ctx.set_dynamic_mesh(pos, mat, alb)
        ctx.set_dynamic_emission(EM)
        for rnd in range(2):
            run_pass(ctx)
            assert_pass(oracle, ctx, Dp, S, f"big triangles, attributes={attributes}, pass {rnd}")
        assert ctx.dynamic_info()["bricks_used"] == 512
        ctx.set_dynamic_emission(None)
        run_pass(ctx)
        assert_pass(oracle, ctx, D, S, "big triangles, detached")


# ---- 4. vct_gi_pass ------------------------------------------------------------------------------------------------------------
def test_gi_pass_equals_the_six_calls_with_the_table(vct, oracle, world):
    from voxel_cone_tracing_amd import scene as sc
    import geomcases
    pos, mat, alb = world["static"]
    frames = geomcases.Case.frames(type("M", (), dict(pos=pos))())
    spec = np.tile(np.array([0.25, 0.5, 0.125], np.float32), (alb.shape[0], 1))
    cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
    light = (0.0, 1.0, 0.25)
    vp, lvp = sc.camera_view_proj(cam, 8, 8), sc.light_view_proj(light)
    with vct.Context(dc.config(vct, shadow_map_size=256)) as fused, vct.Context(dc.config(vct, shadow_map_size=256)) as ref:
        for c in (fused, ref):
            c.upload_triangles(pos, mat, alb)
            c.upload_mesh_attributes(*frames, spec)
            c.set_camera_position(tuple(float(x) for x in cam.position))
            c.set_light_direction(light)
            c.set_dynamic_mesh(*world["A"])
            c.set_dynamic_emission(EM)
        for k in "AB":
            for c in (fused, ref):
                c.update_dynamic_positions(world[k][0])
            fused.gi_pass(lvp, vp)
            ref.render_shadow_map(lvp)
            ref.voxelize(); ref.inject_light(); ref.build_mips()
            ref.render_gbuffer(vp)
            ref.trace_resident()
            depth = ref.download_shadow_map()
            lvp_row = np.ascontiguousarray(np.asarray(lvp, np.float32).reshape(4, 4).T)
            S = dc.layer(oracle, pos, mat, alb, depth=depth, vp=lvp_row)[0]
            Dp = de.add(dc.layer(oracle, *world[k], depth=depth, vp=lvp_row)[0], world[k, "DEm"])
            assert_pass(oracle, ref, Dp, S, f"six calls at {k}")
            assert np.array_equal(fused.download_chain(), ref.download_chain()), k
            assert np.array_equal(fused.download_frame(), ref.download_frame()), k
            assert np.array_equal(fused.download_dynamic_voxels()[0], ref.download_dynamic_voxels()[0]), k
            assert np.array_equal(fused.download_pixel_emission(), ref.download_pixel_emission()), k
            assert fused.last_step_count() == ref.last_step_count() > 0


# ---- 5. with the neighbours ---------------------------------------------------------------------------------------------------
def test_static_emission_lies_under_the_glowing_mover(vct, oracle, world):
    pos, mat, alb = world["static"]
    D, Dp = world["A", NONE][0], world["A", NONE, "D'"]
    p = oracle.default_params(V, G=G)
    table = emission_ref.EMISSION.copy()
    table[mat[3]] = (0.3, 0.1, 0.6)                                  # the wall the object crosses glows too
    S1, L, Em = emission_ref.level0(oracle, p, pos, mat, alb, table)
    glows, d = (S1 != L).any(-1), D[..., 3] > 0
    assert (glows & d).sum() >= 10 and (glows & ~d).sum() >= 10
    with static_ctx(vct, world) as ctx:
        ctx.upload_emission(table)
        ctx.set_dynamic_mesh(*world["A"])
        ctx.set_dynamic_emission(EM)
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, S1, "both tables")
        ctx.upload_emission(None)                                    # the static detach leaves the dynamic table alone
        assert np.array_equal(ctx.dynamic_emission(), EM)
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, L, "the static table detached")
        ctx.upload_emission(table)
        ctx.set_dynamic_emission(None)
        run_pass(ctx)
        assert_pass(oracle, ctx, D, S1, "the dynamic table detached")
        # a new static mesh drops the static table, not the dynamic one
        ctx.set_dynamic_emission(EM)
        ctx.upload_triangles(pos, mat, alb)
        assert np.array_equal(ctx.dynamic_emission(), EM)
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, L, "behind a new static mesh")


def test_local_lights_light_the_emitting_layer(vct, oracle, world):
    (S, Sa, Sn), (D, Da, Dn), Dp = world["S", RAISED], world["A", RAISED], world["A", RAISED, "D'"]
    lights = lr.many_lights(8)
    lit_s, lit_d, lit_plain = lr.level0(S, Sa, Sn, lights, G), lr.level0(Dp, Da, Dn, lights, G), lr.level0(D, Da, Dn, lights, G)
    assert (lit_d != Dp).any(-1).sum() >= 50 and (lit_d != lit_plain).any(-1).sum() >= 100
    want = np.where((D[..., 3] > 0)[..., None], lit_d, lit_s)
    with lit_ctx(vct, world, "A", RAISED) as ctx:
        ctx.set_lights(lights)
        run_pass(ctx)
        assert_chain(oracle, ctx, want, "8 lights over D'")
        assert_radiance(ctx, Dp, "8 lights: the layer is D', before the lights")


def test_bounce_takes_the_emitting_texel_as_its_source(vct, oracle, world):
    S3, D3, Dp = world["S", NONE], world["A", NONE], world["A", NONE, "D'"]
    l0 = dc.merge(Dp, S3[0])
    l1, steps = db.expected(oracle, D3, S3, l0=l0)
    plain, plain_steps = db.expected(oracle, D3, S3)
    assert db.differing(l1, plain).sum() >= 300 and db.differing(l1, l0).sum() >= 2000
    with lit_ctx(vct, world, "A") as ctx:
        ctx.set_dynamic_bounce(True)
        run_pass(ctx)
        ctx.bounce()
        assert_chain(oracle, ctx, l1, "bounce over the chain holding D'")
        assert ctx.last_step_count() == steps
        assert_radiance(ctx, Dp, "the layer behind the bounce")


def test_a_gather_near_the_mover_sees_its_light(vct, oracle, world):
    S, D, Dp = world["S", NONE][0], world["A", NONE][0], world["A", NONE, "D'"]
    r = np.random.default_rng(4)
    P = np.asarray(dc.A) * MS + r.uniform(-20.0, 20.0, (64, 3))
    nn = r.normal(size=(64, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    h = np.where(np.abs(nn[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = np.cross(h, nn)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    pts = np.ascontiguousarray(np.concatenate([P, nn * MS, t * MS, np.cross(nn, t) * MS], 1), np.float32)
    p = oracle.default_params(V, G=G)
    ref = pq.gather(oracle, p, oracle.build_mips(dc.merge(Dp, S)), pts)
    ref_plain = pq.gather(oracle, p, oracle.build_mips(dc.merge(D, S)), pts)
    assert (pq.u32(ref["gather"]) != pq.u32(ref_plain["gather"])).any(-1).sum() >= 16      # the emission shows in the gathers
    with lit_ctx(vct, world, "A") as ctx:
        run_pass(ctx)
        pq.assert_floats_match(ctx.gather_points(pts), ref["gather"], "gather around the glowing A")


# ---- 6. two frame slots -------------------------------------------------------------------------------------------------------
def test_updates_and_passes_alternating_on_two_slots_with_the_table(vct, oracle, world):
    planes = synth.random_gbuffer(64, seed=42, discard_frac=0.05)
    S = world["S", RAISED][0]
    order = "ABABBA"

    def play(sync):
        out = []
        with static_ctx(vct, world, RAISED, debug_outputs=0) as ctx:
            ctx.set_frames_in_flight(2)
            ctx.set_dynamic_mesh(*world["A"])
            ctx.set_dynamic_emission(EM)
            for i, k in enumerate(order):
                ctx.select_frame_slot(i & 1)
                ctx.update_dynamic_positions(world[k][0])
                if sync:
                    ctx.synchronize()
                run_pass(ctx)
                if sync:
                    ctx.synchronize()
                frame = ctx.trace(planes)
                if sync:
                    ctx.synchronize()
                out.append((frame, ctx.download_chain()))
        return out
    got, want = play(False), play(True)
    for i, k in enumerate(order):
        assert np.array_equal(got[i][0], want[i][0]), (i, k, "frame")
        assert np.array_equal(got[i][1], want[i][1]), (i, k, "chain")
        assert np.array_equal(want[i][1], oracle.build_mips(dc.merge(world[k, RAISED, "D'"], S))), (i, k)
    assert not np.array_equal(want[0][0], want[1][0])


# ---- 7. drawing ---------------------------------------------------------------------------------------------------------------
BOTH = 3
DYN_EM = np.array([[1.5, 0.25, 0.0], [0.0, 0.0, 0.0], [0.125, 0.75, 3.0]], np.float32)       # of dyndrawcases' palette


def static_em(nmat):
    em = np.tile(np.array([0.5, 0.25, 2.0], np.float32), (nmat, 1)) * (np.arange(nmat)[:, None] + 1)
    em[1::3] = 0.0
    return em.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def draw_ctx(vct, static, w, h, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=16, width=w, height=h, shadow_map_size=ddc.SHADOW, model_scale=ddc.MS, **kw))
    pos, mat, alb, spec, frames = static
    ctx.upload_triangles(pos, mat, alb)
    ctx.upload_mesh_attributes(*frames, spec)
    return ctx


def draw(ctx, w, h, rows=None):
    ctx.render_shadow_map(ddc.light_vp())
    if rows is None:
        ctx.render_gbuffer(ddc.camera(w, h))
    else:
        ctx.render_gbuffer_rows(ddc.camera(w, h), *rows)


def assert_emission_planes(ctx, want, what, w, h, rows=None):
    got = ctx.download_pixel_emission().reshape(3, h, w)
    want = np.asarray(want, np.float32).reshape(3, h, w)
    if rows is not None:
        got, want = got[:, rows[0] * 8:min(rows[1] * 8, h)], want[:, rows[0] * 8:min(rows[1] * 8, h)]
    bad = np.argwhere((bits(got) != bits(want)).any(0))
    assert bad.shape[0] == 0, (what, "pixel emission", bad.shape[0], bad[:4].tolist())


@pytest.mark.parametrize("w,h", ddc.FRAMES)
def test_pixel_emission_of_the_drawn_mover(vct, oracle, w, h):
    static, dyn = ddc.static_mesh(), ddc.object_mesh("A")
    cat = ddc.concatenated(static, dyn)
    nstat = static[2].shape[0]
    assert len({tuple(a) for a in cat[2].view(np.uint32).tolist()}) == cat[2].shape[0]       # the albedos differ pairwise
    _, planes = ddc.reference(oracle, cat, w, h)
    _, planes_static = ddc.reference(oracle, static, w, h)
    is_dyn = ddc.owner_is_dynamic(planes)
    sem, zeros_s, zeros_d = static_em(nstat), np.zeros((nstat, 3), np.float32), np.zeros((3, 3), np.float32)
    E_both = emission_ref.pixel_emission(planes, cat[2], np.concatenate([sem, DYN_EM]))
    E_dyn = emission_ref.pixel_emission(planes, cat[2], np.concatenate([zeros_s, DYN_EM]))
    E_stat = emission_ref.pixel_emission(planes, cat[2], np.concatenate([sem, zeros_d]))
    E_off = emission_ref.pixel_emission(planes_static, static[2], sem)
    big = w == ddc.W
    assert is_dyn.sum() >= (300 if big else 5) and (E_both[:, is_dyn] > 0).any(0).sum() >= (150 if big else 2)
    assert (E_dyn[:, ~is_dyn] == 0).all() and (E_stat[:, is_dyn] == 0).all() and (E_stat > 0).any()
    assert (bits(E_off) != bits(E_both)).any(0).sum() >= (150 if big else 2)
    rows = (h + 7) // 8
    mid = (rows // 3, max(rows // 3 + 1, 2 * rows // 3))
    with draw_ctx(vct, static, w, h) as ctx:
        ctx.set_dynamic_mesh(*dyn)
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        # only the dynamic table: static pixels 0
        ctx.set_dynamic_emission(DYN_EM)
        assert (ctx.download_pixel_emission() == 0).all()          # attached zeroed
        draw(ctx, w, h)
        assert_emission_planes(ctx, E_dyn, "dynamic table alone", w, h)
        got = ctx.download_gbuffer()
        assert np.array_equal(bits(got).reshape(23, -1), bits(planes).reshape(23, -1)), "the 23 planes do not change with the table"
        # ... and with the flag off the planes hold 0
        ctx.set_dynamic_draw(0)
        draw(ctx, w, h)
        assert (ctx.download_pixel_emission() == 0).all(), "dynamic table alone, flag off"
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        # both tables
        ctx.upload_emission(sem)
        draw(ctx, w, h)
        assert_emission_planes(ctx, E_both, "both tables", w, h)
        # the rows form: the rows of a scissored pass, over planes another state wrote
        ctx.set_dynamic_emission(None)
        draw(ctx, w, h)
        assert_emission_planes(ctx, E_stat, "static table alone (dynamic pixels 0)", w, h)
        ctx.set_dynamic_emission(DYN_EM)
        draw(ctx, w, h, mid)
        assert_emission_planes(ctx, E_both, "rows form", w, h, mid)
        keep = np.ones(h, bool)
        keep[mid[0] * 8:min(mid[1] * 8, h)] = False
        got = ctx.download_pixel_emission().reshape(3, h, w)
        assert np.array_equal(bits(got[:, keep]), bits(E_stat.reshape(3, h, w)[:, keep])), "rows outside the scissor keep what they had"
        # the flag off: the static table's values over the static mesh alone
        ctx.set_dynamic_draw(0)
        draw(ctx, w, h)
        assert_emission_planes(ctx, E_off, "both tables, flag off", w, h)
        # the static detach keeps the planes while the dynamic table is attached, and the other way round
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        ctx.upload_emission(None)
        draw(ctx, w, h)
        assert_emission_planes(ctx, E_dyn, "static table detached", w, h)
        ctx.upload_emission(sem)
        ctx.set_dynamic_emission(None)
        draw(ctx, w, h)
        assert_emission_planes(ctx, E_stat, "dynamic table detached", w, h)
        ctx.upload_emission(None)
        refused(vct, ctx.download_pixel_emission)                  # neither table: no planes


def test_the_frame_adds_the_planes_the_table_wrote(vct, oracle):
    """The composite path is the reference: the frame traced with the tables equals the frame traced over the same resident
    G-buffer with the expected planes handed to vct_set_pixel_emission, and differs from the frame without planes."""
    w, h = ddc.FRAMES[0]
    static, dyn = ddc.static_mesh(), ddc.object_mesh("A")
    cat = ddc.concatenated(static, dyn)
    nstat = static[2].shape[0]
    _, planes = ddc.reference(oracle, cat, w, h)
    sem = static_em(nstat)
    E = emission_ref.pixel_emission(planes, cat[2], np.concatenate([sem, DYN_EM]))
    with draw_ctx(vct, static, w, h) as ctx:
        ctx.set_dynamic_mesh(*dyn)
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        ctx.upload_emission(sem)
        ctx.set_dynamic_emission(DYN_EM)
        draw(ctx, w, h)
        run_pass(ctx)
        ctx.trace_resident()
        with_tables = ctx.download_frame()
        assert_emission_planes(ctx, E, "before the trace", w, h)
        ctx.upload_emission(None)
        ctx.set_dynamic_emission(None)
        run_pass(ctx)                                              # the chain without either table
        ctx.trace_resident()
        dark = ctx.download_frame()
        ctx.upload_emission(sem)
        ctx.set_dynamic_emission(DYN_EM)
        run_pass(ctx)                                              # the chain of the first frame again
        ctx.upload_emission(None)
        ctx.set_dynamic_emission(None)
        refused(vct, ctx.download_pixel_emission)
        ctx.set_pixel_emission(E)
        ctx.trace_resident()
        by_hand = ctx.download_frame()
        assert np.array_equal(with_tables, by_hand)
        ctx.set_pixel_emission(None)
        ctx.trace_resident()
        no_planes = ctx.download_frame()
        assert (no_planes != with_tables).any(-1).sum() >= 50
        assert (dark != with_tables).any(-1).sum() >= 50


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(vct, oracle, world):
    S, D, Dp = world["S", NONE][0], world["A", NONE][0], world["A", NONE, "D'"]
    pos, mat, alb = world["A"]
    L = vct.lib()
    with static_ctx(vct, world) as ctx:
        msg = refused(vct, ctx.set_dynamic_emission, EM)           # no mesh
        assert "no dynamic mesh attached" in msg
        refused(vct, ctx.set_dynamic_emission, None)
        assert ctx.dynamic_emission() is None
        refused(vct, ctx.download_pixel_emission)                  # and no planes were attached
        ctx.set_dynamic_mesh(pos, mat, alb)
        ctx.set_dynamic_emission(EM)
        run_pass(ctx)
        chain, planes0 = ctx.download_chain(), ctx.download_pixel_emission()
        assert_pass(oracle, ctx, Dp, S, "before the refusals")

        def unchanged(what):
            assert np.array_equal(ctx.dynamic_emission(), EM), what
            assert np.array_equal(ctx.download_chain(), chain), what
            assert np.array_equal(ctx.download_pixel_emission(), planes0), what
        for value in (np.nan, np.inf, -np.inf, -0.25):
            for at in ((0, 0), (1, 2), (2, 1)):
                bad = EM.copy()
                bad[at] = value
                msg = refused(vct, ctx.set_dynamic_emission, bad)
                assert f"channel {at[1]} of material {at[0]}" in msg, msg
                unchanged((value, at))
        for variant in (1, 2, 3, 4):                               # the planes are attached (the table attached them)
            refused(vct, ctx.set_trace_variant, variant)
            unchanged(("variant", variant))
        assert L.vct_get_dynamic_emission(ctx._h, None, None) == -1
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, S, "after the refusals")
        # a replace of the mesh drops the table, and with it the planes
        ctx.set_dynamic_mesh(*world["B"])
        assert ctx.dynamic_emission() is None
        refused(vct, ctx.download_pixel_emission)
        run_pass(ctx)
        assert_pass(oracle, ctx, world["B", NONE][0], S, "replaced: no table")
        ctx.set_dynamic_emission(EM)
        ctx.set_dynamic_mesh(None)                                 # a detach of the mesh too
        assert ctx.dynamic_emission() is None
        refused(vct, ctx.download_pixel_emission)
        # without planes the variants are back, and under one the table is refused
        ctx.set_dynamic_mesh(pos, mat, alb)
        for variant in (1, 2, 3, 4):
            ctx.set_trace_variant(variant)
            refused(vct, ctx.set_dynamic_emission, EM)
            assert ctx.dynamic_emission() is None
        ctx.set_trace_variant(0)
        ctx.set_dynamic_emission(EM)
        run_pass(ctx)
        assert_pass(oracle, ctx, Dp, S, "attached after the refusals")
    with static_ctx(vct, world, trace_variant=1) as ctx:            # config.trace_variant 1 with the table
        ctx.set_dynamic_mesh(pos, mat, alb)
        run_pass(ctx)
        chain = ctx.download_chain()
        refused(vct, ctx.set_dynamic_emission, EM)
        assert ctx.dynamic_emission() is None
        refused(vct, ctx.download_pixel_emission)
        run_pass(ctx)
        assert np.array_equal(ctx.download_chain(), chain)
        assert_chain(oracle, ctx, dc.merge(D, S), "trace_variant 1: the plain layer")


# ---- the demo -----------------------------------------------------------------------------------------------------------------
def test_the_demo_carries_a_glowing_obj_through_the_scene(vct, tmp_path):
    """vct_demo --dynamic-emission: the facade's SetDynamicEmission behind SetDynamicMesh; the light shows in the cones."""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxel-cone-tracing_amd", "vct_demo")
    assert os.path.exists(exe), "build it with `make demo`"
    obj = tmp_path / "quad.obj"
    obj.write_text("v -100 -180 -100\nv 100 -180 -100\nv 100 -180 100\nv -100 -180 100\nf 1 2 3\nf 1 3 4\n")

    def run(*args):
        out = subprocess.run([exe, "--voxels", "64", "--size", "32x32", "--shadow", "256", "--frames", "3", "--dynamic-obj", str(obj),
                              "--dynamic-path", "-600,0,0;600,0,0", *args], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return re.search(r"fnv1a=([0-9a-f]{16})", out.stdout).group(1)
    dark, glowing = run(), run("--dynamic-emission", "0=2,1,0.5")
    assert glowing != dark
    assert run("--dynamic-emission", "0=0,0,0") == dark             # an all-zero table attaches nothing
