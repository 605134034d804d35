"""GPU: rigid parts of the dynamic mesh (include/vct.h "dynamic mesh", Parts) -- one 3 x 4 matrix per part, applied to
the rest positions on the device.  Every comparison is bit-equality: the positions against dynpartcases.transform_ref (the
definition in float32 NumPy, one rounding per product and sum; a fused form would differ, tests/test_dynamic_parts_cases.py),
layer and chain against the CPU oracle over those positions, and everything downstream against the positions route --
vct_update_dynamic_positions of the same bits.  Cases and their premises: tests/dynpartcases.py and
tests/test_dynamic_parts_cases.py.  All contexts: 64^3 and an 8 x 8 frame unless said."""
import numpy as np
import pytest

import dyncases as dc
import dynemiscases as de
import dynpartcases as dp
import geomcases
import lights_ref as lr
import vctpkg
from test_gpu_dynamic import NONE, RAISED, assert_chain, nbricks, run_pass, shadow_maps

pytestmark = pytest.mark.gpu
u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


@pytest.fixture(scope="module")
def world(oracle):
    """The static scene and its layer, the 150-triangle object with its parts, and the positions of every pose."""
    pos, mat, alb = dp.mesh(150)
    part = dp.parts(150)
    w = dict(static=dc.static_scene(), mesh=(pos, mat, alb), part=part, maps=shadow_maps())
    for name in dp.POSES:
        w[name] = dp.transform_ref(pos, part, dp.pose(name))
    for sh in (NONE, RAISED):
        depth, vp = w["maps"][sh]
        w["S", sh] = dc.layer(oracle, *w["static"], depth=depth, vp=vp)
    return w


def attach(ctx, w, max_bricks=dp.MAX_BRICKS):
    ctx.set_dynamic_mesh(*w["mesh"], max_bricks=max_bricks)
    ctx.set_dynamic_parts(w["part"], dp.NPARTS)


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


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", [0, 3], ids=["k_dyn_transform", "parts_prepare"])
@pytest.mark.parametrize("ntri", dp.SIZES)
def test_positions_are_the_definition_s_bit_for_bit(vct, ntri, draw):
    import torch
    pos, mat, alb = dp.mesh(ntri)
    part = dp.parts(ntri)
    with vct.Context(dc.config(vct)) as ctx:
        ctx.set_dynamic_draw(draw)
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=dp.MAX_BRICKS)
        assert ctx.dynamic_parts() is None
        assert_positions(ctx, pos, "attached, no parts")
        ctx.set_dynamic_parts(part, dp.NPARTS)
        n, back = ctx.dynamic_parts()
        assert n == dp.NPARTS and np.array_equal(back, part)
        assert_positions(ctx, pos, "parts attached: the current positions are left as they are")
        for name in dp.POSES + ("P1", "P0"):
            m = dp.pose(name)
            want = dp.transform_ref(pos, part, m)
            dev = torch.from_numpy(m).cuda()
            torch.cuda.synchronize()
            for src, given in (("host", m), ("host [n, 3, 4]", m.reshape(-1, 3, 4)), ("device", int(dev.data_ptr())),
                               ("host 4 bytes off", off_boundary(m))):
                ctx.update_dynamic_positions(pos)          # (rest = current = pos again: every source starts from the same state)
                ctx.update_dynamic_transforms(given)
                assert_positions(ctx, want, (name, src, ntri, draw))
        assert (u32(dp.transform_ref(pos, part, dp.pose("P1"))) != u32(pos)).any()


# ---- 2. layer and chain ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", [1, 0])
@pytest.mark.parametrize("shadow", [NONE, RAISED])
def test_layer_and_chain_follow_the_transformed_positions(vct, oracle, world, shadow, attributes):
    depth, vp = world["maps"][shadow]
    S = world["S", shadow][0]
    _, mat, alb = world["mesh"]
    with static_ctx(vct, world, shadow, voxel_attributes=attributes) as ctx:
        attach(ctx, world)
        for name in ("P0", "P1", "P2", "P1"):
            ctx.update_dynamic_transforms(dp.pose(name))
            run_pass(ctx)
            want = dc.layer(oracle, world[name], mat, alb, depth=depth, vp=vp)
            dc.assert_non_degenerate(want[0], S)
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
def test_base_condition_equals_the_positions_route(vct, world):
    pos = world["mesh"][0]
    with static_ctx(vct, world, RAISED) as ctx:
        attach(ctx, world)

        def read():
            run_pass(ctx)
            return ctx.download_dynamic_voxels(), ctx.download_chain(), ctx.dynamic_info()
        seen = []
        for name in ("P1", "P2", "P0", "P1"):
            ctx.update_dynamic_positions(pos)                  # the rest positions again (the positions route below replaced them)
            ctx.update_dynamic_transforms(dp.pose(name))
            a = read()
            ctx.update_dynamic_positions(world[name])
            b = read()
            for x, y in zip(a[0], b[0]):
                assert np.array_equal(x, y), name
            assert np.array_equal(a[1], b[1]) and a[2] == b[2], (name, a[2], b[2])
            seen.append(a[1])
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


@pytest.mark.parametrize("fused", [False, True], ids=["six_calls", "gi_pass"])
@pytest.mark.parametrize("w,h", [(17, 9), (203, 117)])
def test_everything_on_equals_the_positions_route(vct, world, w, h, fused):
    """Both draw flags, an emission table, 8 local lights and the second bounce: shadow-map words, all 23 planes, the
    pixel-emission planes, the chain, the frame and the bounce's chain are the same bytes by either route."""
    vctpkg.load()
    from voxel_cone_tracing_amd import scene as sc
    spos, smat, salb = world["static"]
    pos = world["mesh"][0]
    frames = geomcases.Case.frames(type("M", (), dict(pos=spos))())
    spec = np.tile(np.array([0.25, 0.5, 0.125], np.float32), (salb.shape[0], 1))
    cam = sc.default_camera(**dp.VIEW)
    vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(dp.LIGHT)
    with vct.Context(dc.config(vct, width=w, height=h, shadow_map_size=256)) as ctx:
        ctx.upload_triangles(spos, smat, salb)
        ctx.upload_mesh_attributes(*frames, spec)
        ctx.set_camera_position(tuple(float(x) for x in cam.position))
        ctx.set_light_direction(dp.LIGHT)
        ctx.set_dynamic_draw(vct.DYNAMIC_DRAW_SHADOW | vct.DYNAMIC_DRAW_GBUFFER, (0.3, 0.6, 0.2))
        attach(ctx, world)
        ctx.set_dynamic_emission(de.EM)
        ctx.set_lights(lr.many_lights(8))
        ctx.set_dynamic_bounce(True)

        def read():
            if fused:
                ctx.gi_pass(lvp, vp)
            else:
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
            ctx.update_dynamic_transforms(dp.pose(name))          # drawn: the PARTS prepare
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
    """Parts drawn from all five indices here (dynpartcases.parts_all), so that four bad matrices leave a fifth part to
    compare: NaN, infinity and the huge scale are skipped by the contract and counted; the all-zero part is in contract,
    has no area and adds no fragment."""
    pos, mat, alb = world["mesh"]
    part = dp.parts_all(150)
    S = world["S", NONE][0]
    keep = part == 4
    bad = dp.bad_matrices()
    out = dp.transform_ref(pos, part, bad)
    want = dc.layer(oracle, out[keep], mat[keep], alb)
    with static_ctx(vct, world) as ctx:
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=dp.MAX_BRICKS)
        ctx.set_dynamic_parts(part)
        ctx.update_dynamic_transforms(bad)
        assert_positions(ctx, out, "NaN, infinity and overflow as the products give them")
        run_pass(ctx)
        info = ctx.dynamic_info()
        assert info["skipped"] == int((part <= 2).sum()) and info["left_out"] == 0, info
        for g, x in zip(ctx.download_dynamic_voxels(), want):
            assert np.array_equal(g, x)
        assert_chain(oracle, ctx, dc.merge(want[0], S), "bad matrices")
        # the zero part removed by the contract as well: the same layer and the same fragment count -- it added none
        worse = bad.copy()
        worse[3, 0] = np.float32(np.nan)
        ctx.update_dynamic_transforms(worse)
        run_pass(ctx)
        again = ctx.dynamic_info()
        assert again["skipped"] == int((part <= 3).sum()) and again["fragments"] == info["fragments"] > 0, (info, again)
        assert np.array_equal(ctx.download_dynamic_voxels()[0], want[0])
        # and good matrices afterwards: nothing stuck
        ctx.update_dynamic_transforms(dp.pose("P1"))
        run_pass(ctx)
        assert ctx.dynamic_info()["skipped"] == 0
        assert np.array_equal(ctx.download_dynamic_voxels()[0], dc.layer(oracle, dp.transform_ref(pos, part, dp.pose("P1")), mat, alb)[0])


# ---- 5. state -------------------------------------------------------------------------------------------------------------------
def test_rest_snapshot(vct, world):
    pos, mat, alb = world["mesh"]
    part = world["part"]
    B = dc.dynamic_mesh(dc.B)[0]
    with vct.Context(dc.config(vct)) as ctx:
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=dp.MAX_BRICKS)
        ctx.update_dynamic_positions(B)
        ctx.set_dynamic_parts(part, dp.NPARTS)            # directly behind the update: B is the rest
        ctx.update_dynamic_transforms(dp.pose("P1"))
        assert_positions(ctx, dp.transform_ref(B, part, dp.pose("P1")), "rest = B")
        ctx.update_dynamic_transforms(dp.pose("P2"))       # transforms move the rest, not the current positions
        assert_positions(ctx, dp.transform_ref(B, part, dp.pose("P2")), "rest = B, second transform")
        # positions while parts are attached: new rest and new current
        ctx.update_dynamic_positions(pos)
        assert_positions(ctx, pos, "positions with parts attached")
        ctx.update_dynamic_transforms(dp.pose("P1"))
        assert_positions(ctx, world["P1"], "the next transform moves the new rest")
        # parts set again behind a transform: the transformed positions are the rest
        ctx.set_dynamic_parts(part, dp.NPARTS)
        ctx.update_dynamic_transforms(dp.pose("P2"))
        assert_positions(ctx, dp.transform_ref(world["P1"], part, dp.pose("P2")), "rest = P1's positions")


def test_lifetime_of_the_parts(vct, oracle, world):
    pos, mat, alb = world["mesh"]
    S = world["S", NONE][0]
    with static_ctx(vct, world) as ctx:
        attach(ctx, world)
        ctx.update_dynamic_transforms(dp.pose("P1"))
        run_pass(ctx)
        chain = ctx.download_chain()
        assert_chain(oracle, ctx, dc.merge(dc.layer(oracle, world["P1"], mat, alb)[0], S), "P1")
        ctx.set_dynamic_parts(None)                        # detached: the current positions stay
        assert ctx.dynamic_parts() is None
        assert_positions(ctx, world["P1"], "parts detached")
        run_pass(ctx)
        assert np.array_equal(ctx.download_chain(), chain)
        refused(vct, ctx.update_dynamic_transforms, dp.pose("P1"))
        ctx.set_dynamic_parts(None)                        # nothing to detach: fine
        # replace and detach of the mesh drop the parts
        attach(ctx, world)
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=dp.MAX_BRICKS)
        assert ctx.dynamic_parts() is None
        refused(vct, ctx.update_dynamic_transforms, dp.pose("P1"))
        attach(ctx, world)
        ctx.set_dynamic_mesh(None)
        assert ctx.dynamic_parts() is None
        refused(vct, ctx.update_dynamic_transforms, dp.pose("P1"))
        refused(vct, ctx.set_dynamic_parts, world["part"], dp.NPARTS)
        run_pass(ctx)
        assert_chain(oracle, ctx, S, "mesh detached")


def test_draw_going_on_after_a_transform_draws_the_transformed_positions(vct, world):
    vctpkg.load()
    from voxel_cone_tracing_amd import scene as sc
    spos, smat, salb = world["static"]
    w, h = 203, 117
    frames = geomcases.Case.frames(type("M", (), dict(pos=spos))())
    spec = np.tile(np.array([0.25, 0.5, 0.125], np.float32), (salb.shape[0], 1))
    cam = sc.default_camera(**dp.VIEW)
    vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(dp.LIGHT)
    with vct.Context(dc.config(vct, width=w, height=h, shadow_map_size=256)) as ctx:
        ctx.upload_triangles(spos, smat, salb)
        ctx.upload_mesh_attributes(*frames, spec)
        attach(ctx, world)

        def drawn():
            ctx.render_shadow_map(lvp)
            ctx.render_gbuffer(vp)
            return u32(ctx.download_shadow_map()), u32(ctx.download_gbuffer())
        ctx.update_dynamic_transforms(dp.pose("P1"))      # flags off: k_dyn_move, no draw copy yet
        ctx.set_dynamic_draw(3)
        a = drawn()
        ctx.update_dynamic_positions(world["P1"])
        b = drawn()
        ctx.update_dynamic_positions(world["P0"])
        c = drawn()
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and not np.array_equal(x, z)


def test_a_pose_beyond_capacity_leaves_the_layer_out(vct, oracle, world):
    _, mat, alb = world["mesh"]
    S = world["S", NONE][0]
    with static_ctx(vct, world) as ctx:
        attach(ctx, world, max_bricks=dp.SMALL_CAPACITY)
        ctx.update_dynamic_transforms(dp.pose("P1"))
        run_pass(ctx)
        info = ctx.dynamic_info()
        assert (info["max_bricks"], info["bricks_needed"], info["bricks_used"], info["left_out"]) == \
            (dp.SMALL_CAPACITY, dp.SMALL_CAPACITY + 18, 0, 1), info
        assert_chain(oracle, ctx, S, "left out")
        ctx.update_dynamic_transforms(dp.pose("P0"))
        run_pass(ctx)
        D = dc.layer(oracle, world["P0"], mat, alb)[0]
        assert ctx.dynamic_info()["left_out"] == 0 and nbricks(D) <= dp.SMALL_CAPACITY
        assert_chain(oracle, ctx, dc.merge(D, S), "within capacity again")


def test_refusals_leave_everything_as_it_was(vct, world):
    import ctypes as C
    pos, mat, alb = world["mesh"]
    part = world["part"]
    L = vct.lib()
    m = dp.pose("P1")
    with static_ctx(vct, world) as ctx:
        refused(vct, ctx.set_dynamic_parts, part, dp.NPARTS)                      # no dynamic mesh attached
        refused(vct, ctx.update_dynamic_transforms, m)
        refused(vct, ctx._ck, L.vct_download_dynamic_positions(ctx._h, pos.ctypes.data), "vct_download_dynamic_positions")
        ctx.set_dynamic_mesh(pos, mat, alb, max_bricks=dp.MAX_BRICKS)
        refused(vct, ctx.update_dynamic_transforms, m)                            # no parts attached
        refused(vct, ctx.last_dynamic_transform_ms)
        attach(ctx, world)
        ctx.set_trace_timing(True)
        ctx.update_dynamic_transforms(m)
        run_pass(ctx)
        before = (ctx.download_dynamic_positions(), ctx.download_chain(), ctx.dynamic_info(), ctx.dynamic_parts())
        ms = ctx.last_dynamic_transform_ms()
        print(f"transform kernel {ms:.4f} ms")
        assert ms > 0.0
        for n in (0, -1, vct.DYNAMIC_PARTS_MAX + 1):
            refused(vct, ctx.set_dynamic_parts, part, n)
        refused(vct, ctx._ck, L.vct_set_dynamic_parts(ctx._h, None, 3), "vct_set_dynamic_parts")       # NULL with nparts > 0
        for i, v in ((0, dp.NPARTS), (149, -1), (77, 1 << 20)):
            wrong = part.copy()
            wrong[i] = v
            assert f"triangle {i}" in refused(vct, ctx.set_dynamic_parts, wrong, dp.NPARTS)
        refused(vct, ctx._ck, L.vct_update_dynamic_transforms(ctx._h, None, vct.MEM_HOST), "vct_update_dynamic_transforms")
        refused(vct, ctx._ck, L.vct_update_dynamic_transforms(ctx._h, m.ctypes.data, 7), "vct_update_dynamic_transforms")
        refused(vct, ctx._ck, L.vct_update_dynamic_transforms(ctx._h, m.ctypes.data + 2, vct.MEM_HOST), "vct_update_dynamic_transforms")
        refused(vct, ctx._ck, L.vct_download_dynamic_positions(ctx._h, None), "vct_download_dynamic_positions")
        for shape in ((dp.NPARTS, 11), (dp.NPARTS + 1, 12), (dp.NPARTS, 4, 3), (dp.NPARTS * 12,)):
            with pytest.raises(vct.VctError):
                ctx.update_dynamic_transforms(np.zeros(shape, np.float32))
        with pytest.raises(vct.VctError):
            ctx.set_dynamic_parts(part[:-1], dp.NPARTS)
        assert L.vct_get_dynamic_parts(ctx._h, None, None) != 0 and L.vct_last_dynamic_transform_ms(ctx._h, None) != 0
        run_pass(ctx)
        after = (ctx.download_dynamic_positions(), ctx.download_chain(), ctx.dynamic_info(), ctx.dynamic_parts())
        assert np.array_equal(u32(before[0]), u32(after[0])) and np.array_equal(before[1], after[1]) and before[2] == after[2]
        assert before[3][0] == after[3][0] and np.array_equal(before[3][1], after[3][1])
        assert ctx.last_dynamic_transform_ms() == ms                             # no transform ran in between
        ctx.set_trace_timing(False)
        ctx.update_dynamic_transforms(m)
        refused(vct, ctx.last_dynamic_transform_ms)
        ctx.set_trace_timing(True)
        ctx.update_dynamic_transforms(m)
        assert ctx.last_dynamic_transform_ms() > 0.0
        assert_positions(ctx, world["P1"], "after the refusals")


# ---- 6. two frame slots ---------------------------------------------------------------------------------------------------------
def test_transforms_and_passes_alternating_on_two_slots(vct):
    """dyncases.crowd() (200 k small triangles) at 128^3, one part per eighth of its triangles; per frame: select slot k & 1,
    vct_update_dynamic_transforms(pose k), vct_gi_pass -- frames and the final chain against a one-slot replay of the same
    calls with a vct_synchronize behind each.  The other slot's k_dyn_tris may still be reading the positions when the next
    update is issued; vct_update_dynamic_transforms does vct_pipeline_join for that.

    A scratch build without that join (never committed) PASSES this test, as tests/test_gpu_pipeline_features.py found for
    vct_update_dynamic_positions: the only readers of the position buffer are the kernels of vct_voxelize / vct_gi_pass,
    those calls are producers, and vct_select_frame_slot puts the stream selected next behind a producer, so the table copy
    and the kernel of an update issued on the other slot already follow the pass.  The join in the update is a guarantee,
    not an observable; what this test pins is the result of the two-slot order."""
    vctpkg.load()
    from voxel_cone_tracing_amd import scene as sc
    V, w, h, nparts = 128, 64, 36, 8
    off, mat, alb = dc.crowd()
    rest = dc.placed(off, dc.A)
    ntri = rest.shape[0]
    part = (np.arange(ntri) * nparts // ntri).astype(np.int32)
    spos, smat, salb = dc.static_scene()
    frames = geomcases.Case.frames(type("M", (), dict(pos=spos))())
    spec = np.tile(np.array([0.25, 0.5, 0.125], np.float32), (salb.shape[0], 1))
    cam = sc.default_camera(**dp.VIEW)
    vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(dp.LIGHT)
    r = np.random.default_rng(8)
    poses = []
    for k in range(6):
        m = np.stack([dp.about(dp.rotation(r.normal(size=3), float(r.uniform(-180, 180))), r.uniform(-400, 400, 3)) for _ in range(nparts)])
        poses.append(np.ascontiguousarray(m.astype(np.float32).reshape(nparts, 12)))

    def play(slots):
        out = []
        with vct.Context(dc.config(vct, V=V, width=w, height=h, shadow_map_size=256, debug_outputs=0)) as ctx:
            ctx.upload_triangles(spos, smat, salb)
            ctx.upload_mesh_attributes(*frames, spec)
            ctx.set_camera_position(tuple(float(x) for x in cam.position))
            ctx.set_light_direction(dp.LIGHT)
            if slots == 2:
                ctx.set_frames_in_flight(2)
            ctx.set_dynamic_mesh(rest, mat, alb, max_bricks=(V // 8) ** 3)
            ctx.set_dynamic_parts(part, nparts)
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
    assert np.array_equal(u32(got[-2]), u32(dp.transform_ref(rest, part, poses[-1]))) and got[-1] == want[-1]
    assert want[-1]["left_out"] == 0 and want[-1]["bricks_used"] >= 100
    assert not np.array_equal(want[0], want[1])
