"""GPU: a skin on the dynamic mesh (include/vct.h "dynamic mesh", Skin) -- four bone influences per triangle corner, one
3 x 4 matrix per bone, blended and applied to the rest positions on the device.  Every comparison is bit-equality: the
positions against dynskincases.skin_ref (the definition in float32 NumPy, one rounding per product and sum; a fused form
would differ, tests/test_dynamic_skin_cases.py), layer and chain against the CPU oracle over those positions, and
everything downstream against the positions route -- vct_update_dynamic_positions of the same bits.  Cases and their
premises: tests/dynskincases.py and tests/test_dynamic_skin_cases.py.  All contexts: 64^3 and an 8 x 8 frame unless said."""
import numpy as np
import pytest

import dyncases as dc
import dynemiscases as de
import dynpartcases as dp
import dynskincases as ds
import geomcases
import vctpkg
from test_gpu_dynamic import ISSUE, NONE, RAISED, assert_chain, nbricks, run_pass, shadow_maps

pytestmark = pytest.mark.gpu
u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


@pytest.fixture(scope="module")
def world(oracle):
    """The static scene and its layer, the 150-triangle object with its influences, and the positions of every pose."""
    pos, mat, alb = ds.mesh(150)
    bone, weight = ds.influences(150)
    w = dict(static=dc.static_scene(), mesh=(pos, mat, alb), bone=bone, weight=weight, maps=shadow_maps())
    for name in ds.POSES + ("PX",):
        w[name] = ds.skin_ref(pos, bone, weight, ds.pose(name))
    for sh in (NONE, ISSUE, RAISED):
        depth, vp = w["maps"][sh]
        w["S", sh] = dc.layer(oracle, *w["static"], depth=depth, vp=vp)
    return w


def attach(ctx, w, max_bricks=ds.MAX_BRICKS):
    ctx.set_dynamic_mesh(*w["mesh"], max_bricks=max_bricks)
    ctx.set_dynamic_skin(w["bone"], w["weight"], ds.NBONES)


def static_ctx(vct, w, shadow=NONE, **kw):
    ctx = vct.Context(dc.config(vct, **kw))
    ctx.upload_triangles(*w["static"])
    if shadow != NONE:
        ctx.upload_shadow_map(*w["maps"][shadow])
    return ctx


def off_boundary(m):
    """The same matrices in a host array that starts 4 bytes off a 16-byte boundary."""
    buf = np.zeros(m.size + 8, np.float32)
    k = next(i for i in range(4) if (buf.ctypes.data + 4 * i) % 16 == 4)
    out = buf[k:k + m.size].reshape(m.shape)
    out[...] = m
    assert out.ctypes.data % 16 == 4 and out.flags["C_CONTIGUOUS"]
    return out


def assert_positions(ctx, want, what):
    got = ctx.download_dynamic_positions()
    bad = np.argwhere(u32(got) != u32(want))
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist())


def refused(vct, call, *a, **kw):
    with pytest.raises(vct.VctError) as e:
        call(*a, **kw)
    assert "(-1)" in str(e.value), str(e.value)               # VCT_ERR_INVALID
    return str(e.value)


# ---- 1. the kernels alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", [0, 3], ids=["k_dyn_skin", "skin_prepare"])
@pytest.mark.parametrize("ntri", ds.SIZES)
def test_positions_are_the_definition_s_bit_for_bit(vct, ntri, draw):
    import torch
    pos, mat, alb = ds.mesh(ntri)
    bone, weight = ds.influences(ntri)
    with vct.Context(dc.config(vct)) as ctx:
        ctx.set_dynamic_draw(draw)
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=ds.MAX_BRICKS)
        assert ctx.dynamic_skin() is None
        ctx.set_dynamic_skin(bone, weight, ds.NBONES)
        n, b, w = ctx.dynamic_skin()
        assert n == ds.NBONES and np.array_equal(b, bone) and np.array_equal(u32(w), u32(weight))
        assert ctx.dynamic_parts() is None
        assert_positions(ctx, pos, "skin attached: the current positions are left as they are")
        for name in ds.POSES + ("P1", "P0"):
            m = ds.pose(name)
            want = ds.skin_ref(pos, bone, weight, m)
            dev = torch.from_numpy(m).cuda()
            torch.cuda.synchronize()
            for src, given in (("host", m), ("host [n, 3, 4]", m.reshape(-1, 3, 4)), ("device", int(dev.data_ptr())),
                               ("host 4 bytes off", off_boundary(m))):
                ctx.update_dynamic_positions(pos)          # (rest = current = pos again: every source starts from the same state)
                ctx.update_dynamic_transforms(given)
                assert_positions(ctx, want, (name, src, ntri, draw))
        assert (u32(ds.skin_ref(pos, bone, weight, ds.pose("P1"))) != u32(pos)).any()


@pytest.mark.parametrize("draw", [0, 3], ids=["k_dyn_skin", "skin_prepare"])
def test_the_largest_bone_index(vct, draw):
    """nbones = VCT_DYNAMIC_BONES_MAX: every influence on bone 4 moved to bone 65535, the last index the packed uint16 holds
    and the last row of the table; the rows in between are zero matrices that no corner names."""
    pos, mat, alb = ds.mesh(150)
    bone, weight = ds.influences(150)
    top = vct.DYNAMIC_BONES_MAX - 1
    bone = np.where(bone == 4, top, bone).astype(np.int32)
    assert (bone == top).sum() >= 10 and top == 65535
    m = np.zeros((vct.DYNAMIC_BONES_MAX, 12), np.float32)
    m[:4] = ds.pose("P1")[:4]
    m[top] = ds.pose("P1")[4]
    with vct.Context(dc.config(vct)) as ctx:
        ctx.set_dynamic_draw(draw)
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=ds.MAX_BRICKS)
        ctx.set_dynamic_skin(bone, weight, vct.DYNAMIC_BONES_MAX)
        n, b, _ = ctx.dynamic_skin()
        assert n == vct.DYNAMIC_BONES_MAX and np.array_equal(b, bone)
        ctx.update_dynamic_transforms(m)
        assert_positions(ctx, ds.skin_ref(pos, *ds.influences(150), ds.pose("P1")), "bone 65535")
        refused(vct, ctx.set_dynamic_skin, bone, weight, vct.DYNAMIC_BONES_MAX + 1)
        refused(vct, ctx.set_dynamic_skin, bone, weight, top)                      # 65535 is out of range for 65535 bones


# ---- 2. layer and chain ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", [1, 0])
@pytest.mark.parametrize("shadow", [ISSUE, RAISED])
def test_layer_and_chain_follow_the_skinned_positions(vct, oracle, world, shadow, attributes):
    depth, vp = world["maps"][shadow]
    S = world["S", shadow][0]
    _, mat, alb = world["mesh"]
    with static_ctx(vct, world, shadow, voxel_attributes=attributes) as ctx:
        attach(ctx, world)
        for name in ("P0", "P1", "P2", "P1"):
            ctx.update_dynamic_transforms(ds.pose(name))
            run_pass(ctx)
            want = dc.layer(oracle, world[name], mat, alb, depth=depth, vp=vp)
            if not attributes:
                assert np.array_equal(dc.layer_plain(oracle, world[name], mat, alb, depth=depth, vp=vp), want[0])
            got = ctx.download_dynamic_voxels()
            for g, x, plane in zip(got, want, ("radiance", "albedo", "normal")):
                if attributes or plane == "radiance":
                    assert np.array_equal(g, x), (name, plane, int((g != x).any(-1).sum()))
                else:
                    assert g is None
            # the chain: the merge, the mips, and nothing left in the bricks the previous pose occupied
            assert_chain(oracle, ctx, dc.merge(want[0], S), (name, shadow, attributes))
            info = ctx.dynamic_info()
            assert info["bricks_needed"] == info["bricks_used"] == nbricks(want[0]) and info["skipped"] == info["left_out"] == 0, info


# ---- 3. the same bits as the positions route ------------------------------------------------------------------------------------
def test_everything_downstream_equals_the_positions_route(vct, world):
    """Both draw flags, an emission table and the second bounce: shadow-map words, all G-buffer planes, the pixel-emission
    planes, the chain, the frame and the bounce's chain are the same bytes by either route."""
    vctpkg.load()
    from voxel_cone_tracing_amd import scene as sc
    w, h = 203, 117
    spos, smat, salb = world["static"]
    pos = world["mesh"][0]
    frames = geomcases.Case.frames(type("M", (), dict(pos=spos))())
    spec = np.tile(np.array([0.25, 0.5, 0.125], np.float32), (salb.shape[0], 1))
    cam = sc.default_camera(**ds.VIEW)
    vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(ds.LIGHT)
    with vct.Context(dc.config(vct, width=w, height=h, shadow_map_size=256)) as ctx:
        ctx.upload_triangles(spos, smat, salb)
        ctx.upload_mesh_attributes(*frames, spec)
        ctx.set_camera_position(tuple(float(x) for x in cam.position))
        ctx.set_light_direction(ds.LIGHT)
        ctx.set_dynamic_draw(vct.DYNAMIC_DRAW_SHADOW | vct.DYNAMIC_DRAW_GBUFFER, (0.3, 0.6, 0.2))
        attach(ctx, world)
        ctx.set_dynamic_emission(de.EM)
        ctx.set_dynamic_bounce(True)

        def read():
            ctx.render_shadow_map(lvp)
            run_pass(ctx)
            ctx.render_gbuffer(vp)
            ctx.trace_resident()
            out = dict(shadow=u32(ctx.download_shadow_map()), planes=u32(ctx.download_gbuffer()),
                       emission=u32(ctx.download_pixel_emission()), chain=ctx.download_chain(), frame=ctx.download_frame(),
                       info=ctx.dynamic_info())
            ctx.bounce()
            out["bounce"] = ctx.download_chain()
            return out
        seen = []
        for name in ("P1", "P2", "P0"):
            ctx.update_dynamic_positions(pos)
            ctx.update_dynamic_transforms(ds.pose(name))          # drawn: the skin form of the prepare kernel
            a = read()
            ctx.update_dynamic_positions(world[name])            # the copy and the plain prepare
            b = read()
            for key in a:
                same = a[key] == b[key] if key == "info" else np.array_equal(a[key], b[key])
                assert same, (name, key)
            seen.append(a)
        for key in ("shadow", "planes", "chain", "bounce", "frame"):
            assert not np.array_equal(seen[0][key], seen[2][key]), key          # the pose shows in every output
        assert (seen[2]["emission"] != 0).any() and not np.array_equal(seen[0]["chain"], seen[0]["bounce"])


# ---- 4. unvalidated matrices ----------------------------------------------------------------------------------------------------
def test_bad_matrices_go_through_the_vertex_contract(vct, oracle, world):
    """A NaN in one bone's matrix and an infinity in another's: every triangle with a corner that names either bone is
    skipped by the contract and counted, the others are voxelized as in P1, and the next good pose is clean."""
    pos, mat, alb = world["mesh"]
    bone = world["bone"]
    S = world["S", NONE][0]
    gone = ds.names(bone, ds.NAN_BONE) | ds.names(bone, ds.INF_BONE)
    keep = ~gone
    bad = ds.bad_matrices()
    out = ds.skin_ref(pos, bone, world["weight"], bad)
    want = dc.layer(oracle, out[keep], mat[keep], alb)
    with static_ctx(vct, world) as ctx:
        attach(ctx, world)
        ctx.update_dynamic_transforms(bad)
        assert_positions(ctx, out, "NaN and infinity as the products give them")
        run_pass(ctx)
        info = ctx.dynamic_info()
        assert info["skipped"] == int(gone.sum()) and 0 < info["skipped"] < 150 and info["left_out"] == 0, info
        for g, x in zip(ctx.download_dynamic_voxels(), want):
            assert np.array_equal(g, x)
        assert_chain(oracle, ctx, dc.merge(want[0], S), "bad matrices")
        ctx.update_dynamic_transforms(ds.pose("P1"))          # good matrices afterwards: nothing stuck
        run_pass(ctx)
        assert ctx.dynamic_info()["skipped"] == 0
        assert np.array_equal(ctx.download_dynamic_voxels()[0], dc.layer(oracle, world["P1"], mat, alb)[0])


def test_a_zero_weight_does_not_skip_a_nan_bone(vct, oracle, world):
    """As defined: all four terms are evaluated and 0 * NaN is NaN, so the one triangle whose unused slot names the bone
    with the NaN matrix is skipped; every other triangle is where P1 puts it."""
    pos, mat, alb = world["mesh"]
    bone, weight, t, m = ds.zero_weight_case()
    keep = np.arange(150) != t
    with static_ctx(vct, world) as ctx:
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=ds.MAX_BRICKS)
        ctx.set_dynamic_skin(bone, weight, ds.NBONES)
        ctx.update_dynamic_transforms(m)
        got = ctx.download_dynamic_positions()
        assert np.array_equal(u32(got[keep]), u32(world["P1"][keep])) and np.isnan(got[t, 6])
        assert_positions(ctx, ds.skin_ref(pos, bone, weight, m), "0 * NaN")
        run_pass(ctx)
        info = ctx.dynamic_info()
        assert info["skipped"] == 1 and info["left_out"] == 0, info
        assert np.array_equal(ctx.download_dynamic_voxels()[0], dc.layer(oracle, world["P1"][keep], mat[keep], alb)[0])


def test_a_pose_beyond_capacity_leaves_the_layer_out(vct, oracle, world):
    _, mat, alb = world["mesh"]
    S = world["S", NONE][0]
    with static_ctx(vct, world) as ctx:
        attach(ctx, world, max_bricks=ds.SMALL_CAPACITY)
        ctx.update_dynamic_transforms(ds.pose("PX"))
        run_pass(ctx)
        info = ctx.dynamic_info()
        assert (info["max_bricks"], info["bricks_needed"], info["bricks_used"], info["left_out"]) == \
            (ds.SMALL_CAPACITY, ds.SMALL_CAPACITY + ds.OVER, 0, 1), info
        assert_chain(oracle, ctx, S, "left out: the static chain")
        ctx.update_dynamic_transforms(ds.pose("P0"))
        run_pass(ctx)
        D = dc.layer(oracle, world["P0"], mat, alb)[0]
        assert ctx.dynamic_info()["left_out"] == 0 and nbricks(D) <= ds.SMALL_CAPACITY
        assert_chain(oracle, ctx, dc.merge(D, S), "within capacity again")


# ---- 5. rules -------------------------------------------------------------------------------------------------------------------
def test_rest_ownership_and_detach(vct, oracle, world):
    pos, mat, alb = world["mesh"]
    bone, weight = world["bone"], world["weight"]
    B = dc.dynamic_mesh(dc.B)[0]
    S = world["S", NONE][0]
    with static_ctx(vct, world) as ctx:
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=ds.MAX_BRICKS)
        ctx.update_dynamic_positions(B)
        ctx.set_dynamic_skin(bone, weight, ds.NBONES)            # directly behind the update: B is the rest
        ctx.update_dynamic_transforms(ds.pose("P1"))
        assert_positions(ctx, ds.skin_ref(B, bone, weight, ds.pose("P1")), "rest = B")
        ctx.update_dynamic_transforms(ds.pose("P2"))             # the matrices move the rest, not the current positions
        assert_positions(ctx, ds.skin_ref(B, bone, weight, ds.pose("P2")), "rest = B, second update")
        ctx.update_dynamic_positions(pos)                        # positions with a skin attached: new rest and new current
        assert_positions(ctx, pos, "positions with a skin attached")
        ctx.update_dynamic_transforms(ds.pose("P1"))
        assert_positions(ctx, world["P1"], "the next update moves the new rest")
        run_pass(ctx)
        chain = ctx.download_chain()
        assert_chain(oracle, ctx, dc.merge(dc.layer(oracle, world["P1"], mat, alb)[0], S), "P1")
        ctx.set_dynamic_skin(None, None)                         # detached: the current positions stay
        assert ctx.dynamic_skin() is None
        assert_positions(ctx, world["P1"], "skin detached")
        run_pass(ctx)
        assert np.array_equal(ctx.download_chain(), chain)
        refused(vct, ctx.update_dynamic_transforms, ds.pose("P1"))
        ctx.set_dynamic_skin(None, None)                         # nothing to detach: fine
        attach(ctx, world)                                       # replace and detach of the mesh drop the skin
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=ds.MAX_BRICKS)
        assert ctx.dynamic_skin() is None
        refused(vct, ctx.update_dynamic_transforms, ds.pose("P1"))
        attach(ctx, world)
        ctx.set_dynamic_mesh(None)
        assert ctx.dynamic_skin() is None
        refused(vct, ctx.set_dynamic_skin, bone, weight, ds.NBONES)
        run_pass(ctx)
        assert_chain(oracle, ctx, S, "mesh detached")


def test_parts_and_skin_refuse_each_other(vct, world):
    pos, mat, alb = world["mesh"]
    bone, weight = world["bone"], world["weight"]
    part = dp.parts(150)
    with vct.Context(dc.config(vct)) as ctx:
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=ds.MAX_BRICKS)
        ctx.set_dynamic_skin(bone, weight, ds.NBONES)
        ctx.update_dynamic_transforms(ds.pose("P1"))
        assert "do not go together" in refused(vct, ctx.set_dynamic_parts, part, dp.NPARTS)
        assert ctx.dynamic_parts() is None and ctx.dynamic_skin()[0] == ds.NBONES
        ctx.update_dynamic_transforms(ds.pose("P2"))             # the skin is untouched: it still takes six matrices
        assert_positions(ctx, world["P2"], "skin after the refused parts")
        ctx.set_dynamic_parts(None)                              # no parts to detach: fine, and the skin stays
        assert ctx.dynamic_skin()[0] == ds.NBONES
        ctx.set_dynamic_skin(None, None)
        ctx.update_dynamic_positions(pos)
        ctx.set_dynamic_parts(part, dp.NPARTS)
        ctx.update_dynamic_transforms(dp.pose("P1"))
        want = dp.transform_ref(pos, part, dp.pose("P1"))
        assert "do not go together" in refused(vct, ctx.set_dynamic_skin, bone, weight, ds.NBONES)
        assert ctx.dynamic_skin() is None and ctx.dynamic_parts()[0] == dp.NPARTS
        assert_positions(ctx, want, "parts after the refused skin")
        ctx.update_dynamic_transforms(dp.pose("P2"))
        assert_positions(ctx, dp.transform_ref(pos, part, dp.pose("P2")), "parts still move")
        ctx.set_dynamic_skin(None, None)                         # no skin to detach: the parts stay
        assert ctx.dynamic_parts()[0] == dp.NPARTS


@pytest.mark.parametrize("draw", [0, 3], ids=["plain", "prepare"])
def test_table_and_timer_are_fresh_across_a_change_of_kind(vct, world, draw):
    """The movers share one rest buffer, one matrix table and one timer: every attach -- of the other kind behind a detach,
    or of the same kind again -- starts with a fresh rest snapshot and a timer that has not run."""
    pos, mat, alb = world["mesh"]
    bone, weight = world["bone"], world["weight"]
    part = dp.parts(150)
    with vct.Context(dc.config(vct)) as ctx:
        ctx.set_trace_timing(True)
        ctx.set_dynamic_draw(draw)
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=ds.MAX_BRICKS)
        ctx.set_dynamic_skin(bone, weight, ds.NBONES)
        ctx.update_dynamic_transforms(ds.pose("P1"))
        assert ctx.last_dynamic_transform_ms() > 0.0
        ctx.set_dynamic_skin(None, None)
        refused(vct, ctx.last_dynamic_transform_ms)
        ctx.update_dynamic_positions(pos)
        ctx.set_dynamic_parts(part, dp.NPARTS)
        refused(vct, ctx.last_dynamic_transform_ms)              # the skin's timer did not carry over
        ctx.update_dynamic_transforms(dp.pose("P1"))
        moved = dp.transform_ref(pos, part, dp.pose("P1"))
        assert_positions(ctx, moved, "parts behind a skin")      # ... and neither did its table or its rest positions
        assert ctx.last_dynamic_transform_ms() > 0.0
        ctx.set_dynamic_parts(part, dp.NPARTS)                   # the same kind again: the moved positions are the rest
        refused(vct, ctx.last_dynamic_transform_ms)
        ctx.update_dynamic_transforms(dp.pose("P1"))
        moved = dp.transform_ref(moved, part, dp.pose("P1"))
        assert_positions(ctx, moved, "parts re-attached")
        ctx.set_dynamic_parts(None)
        ctx.set_dynamic_skin(bone, weight, ds.NBONES)
        ctx.update_dynamic_transforms(ds.pose("P2"))
        assert_positions(ctx, ds.skin_ref(moved, bone, weight, ds.pose("P2")), "a skin behind parts")


def test_refusals_leave_everything_as_it_was(vct, world):
    pos, mat, alb = world["mesh"]
    bone, weight = world["bone"], world["weight"]
    L = vct.lib()
    m = ds.pose("P1")
    with static_ctx(vct, world) as ctx:
        refused(vct, ctx.set_dynamic_skin, bone, weight, ds.NBONES)               # no dynamic mesh attached
        refused(vct, ctx._ck, L.vct_set_dynamic_skin(ctx._h, None, None, 0), "vct_set_dynamic_skin")
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=ds.MAX_BRICKS)
        refused(vct, ctx.update_dynamic_transforms, m)                            # no skin attached
        refused(vct, ctx.last_dynamic_transform_ms)
        attach(ctx, world)
        ctx.set_trace_timing(True)
        ctx.update_dynamic_transforms(m)
        run_pass(ctx)
        before = (ctx.download_dynamic_positions(), ctx.download_chain(), ctx.dynamic_info(), ctx.dynamic_skin())
        ms = ctx.last_dynamic_transform_ms()
        print(f"skin kernel {ms:.4f} ms")
        assert ms > 0.0
        for n in (0, -1, vct.DYNAMIC_BONES_MAX + 1):
            refused(vct, ctx.set_dynamic_skin, bone, weight, n)
        b, w = bone.ctypes.data, weight.ctypes.data
        refused(vct, ctx._ck, L.vct_set_dynamic_skin(ctx._h, None, w, ds.NBONES), "vct_set_dynamic_skin")
        refused(vct, ctx._ck, L.vct_set_dynamic_skin(ctx._h, b, None, ds.NBONES), "vct_set_dynamic_skin")
        refused(vct, ctx._ck, L.vct_set_dynamic_skin(ctx._h, None, None, 3), "vct_set_dynamic_skin")
        for (t, c, s), v in (((0, 0, 0), ds.NBONES), ((149, 2, 3), -1), ((77, 1, 2), 1 << 20)):
            wrong = bone.copy()
            wrong[t, c, s] = v
            msg = refused(vct, ctx.set_dynamic_skin, wrong, weight, ds.NBONES)
            assert f"triangle {t}, corner {c}, slot {s}" in msg and "bone index" in msg, msg
        for (t, c, s), v in (((0, 0, 0), np.nan), ((149, 2, 3), np.inf), ((77, 1, 2), -np.inf)):
            wrong = weight.copy()
            wrong[t, c, s] = v
            msg = refused(vct, ctx.set_dynamic_skin, bone, wrong, ds.NBONES)
            assert f"triangle {t}, corner {c}, slot {s}" in msg and "weight" in msg, msg
        refused(vct, ctx._ck, L.vct_update_dynamic_transforms(ctx._h, None, vct.MEM_HOST), "vct_update_dynamic_transforms")
        refused(vct, ctx._ck, L.vct_update_dynamic_transforms(ctx._h, m.ctypes.data, 7), "vct_update_dynamic_transforms")
        refused(vct, ctx._ck, L.vct_update_dynamic_transforms(ctx._h, m.ctypes.data + 2, vct.MEM_HOST), "vct_update_dynamic_transforms")
        for shape in ((ds.NBONES, 11), (ds.NBONES + 1, 12), (ds.NBONES, 4, 3), (ds.NBONES * 12,)):
            with pytest.raises(vct.VctError) as e:
                ctx.update_dynamic_transforms(np.zeros(shape, np.float32))
            assert "bones" in str(e.value)
        with pytest.raises(vct.VctError):
            ctx.set_dynamic_skin(bone[:-1], weight[:-1], ds.NBONES)
        assert L.vct_get_dynamic_skin(ctx._h, None, None, None) != 0
        assert L.vct_set_dynamic_skin(None, b, w, ds.NBONES) != 0 and L.vct_get_dynamic_skin(None, None, None, None) != 0
        run_pass(ctx)
        after = (ctx.download_dynamic_positions(), ctx.download_chain(), ctx.dynamic_info(), ctx.dynamic_skin())
        assert np.array_equal(u32(before[0]), u32(after[0])) and np.array_equal(before[1], after[1]) and before[2] == after[2]
        assert before[3][0] == after[3][0] and np.array_equal(before[3][1], after[3][1]) and np.array_equal(u32(before[3][2]), u32(after[3][2]))
        assert ctx.last_dynamic_transform_ms() == ms                             # no kernel ran in between
        ctx.set_trace_timing(False)
        ctx.update_dynamic_transforms(m)
        refused(vct, ctx.last_dynamic_transform_ms)
        ctx.set_trace_timing(True)
        ctx.update_dynamic_transforms(m)
        assert ctx.last_dynamic_transform_ms() > 0.0
        assert_positions(ctx, world["P1"], "after the refusals")


# ---- 6. two frame slots ---------------------------------------------------------------------------------------------------------
def test_updates_and_passes_alternating_on_two_slots(vct):
    """dyncases.crowd() (200 k small triangles) at 128^3 skinned to 8 bones; per frame: select slot k & 1,
    vct_update_dynamic_transforms(pose k), vct_gi_pass -- frames and the final chain against a one-slot replay of the same
    calls with a vct_synchronize behind each.  The other slot's pass may still be reading the positions when the next
    update is issued; vct_update_dynamic_transforms does vct_pipeline_join for that, for a skin as for parts (what
    tests/test_gpu_dynamic_parts.py says about the join being a guarantee, not an observable, holds here too)."""
    vctpkg.load()
    from voxel_cone_tracing_amd import scene as sc
    V, w, h, nbones = 128, 64, 36, 8
    off, mat, alb = dc.crowd()
    rest = dc.placed(off, dc.A)
    ntri = rest.shape[0]
    r = np.random.default_rng(8)
    home = (np.arange(ntri) * nbones // ntri).astype(np.int32)                    # a triangle's main bone: an eighth of the mesh each
    bone = r.integers(0, nbones, (ntri, 3, 4)).astype(np.int32)
    bone[..., 0] = home[:, None]
    weight = r.uniform(0.0, 0.1, (ntri, 3, 4))
    weight[..., 0] = 1.0 - weight[..., 1:].sum(-1)
    weight = np.ascontiguousarray(weight.astype(np.float32))
    spos, smat, salb = dc.static_scene()
    frames = geomcases.Case.frames(type("M", (), dict(pos=spos))())
    spec = np.tile(np.array([0.25, 0.5, 0.125], np.float32), (salb.shape[0], 1))
    cam = sc.default_camera(**ds.VIEW)
    vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(ds.LIGHT)
    poses = []
    for k in range(6):
        m = np.stack([dp.about(dp.rotation(r.normal(size=3), float(r.uniform(-180, 180))), r.uniform(-400, 400, 3)) for _ in range(nbones)])
        poses.append(np.ascontiguousarray(m.astype(np.float32).reshape(nbones, 12)))

    def play(slots):
        out = []
        with vct.Context(dc.config(vct, V=V, width=w, height=h, shadow_map_size=256, debug_outputs=0)) as ctx:
            ctx.upload_triangles(spos, smat, salb)
            ctx.upload_mesh_attributes(*frames, spec)
            ctx.set_camera_position(tuple(float(x) for x in cam.position))
            ctx.set_light_direction(ds.LIGHT)
            if slots == 2:
                ctx.set_frames_in_flight(2)
            ctx.set_dynamic_mesh(rest, mat, alb, max_bricks=(V // 8) ** 3)
            ctx.set_dynamic_skin(bone, weight, nbones)
            for k, m in enumerate(poses):
                if slots == 2:
                    ctx.select_frame_slot(k & 1)
                ctx.update_dynamic_transforms(m)
                if slots == 1:
                    ctx.synchronize()
                ctx.gi_pass(lvp, vp)
                if slots == 1:
                    ctx.synchronize()
                out.append(ctx.download_frame())
            if slots == 2:
                ctx.synchronize()
            out.append(ctx.download_chain())
            out.append(ctx.download_dynamic_positions())
            out.append(ctx.dynamic_info())
        return out
    got, want = play(2), play(1)
    for k in range(len(poses)):
        assert np.array_equal(got[k], want[k]), (k, "frame")
    assert np.array_equal(got[-3], want[-3]), "chain"
    assert np.array_equal(u32(got[-2]), u32(ds.skin_ref(rest, bone, weight, poses[-1]))) and got[-1] == want[-1]
    assert want[-1]["left_out"] == 0 and want[-1]["bricks_used"] >= 100
    assert not np.array_equal(want[0], want[1])
