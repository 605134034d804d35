"""GPU: corner normals of the dynamic mesh (include/vct.h "dynamic mesh", Normals; vct_set_dynamic_normals).  Every
comparison is bit-equality: the frames vct_download_dynamic_frames returns against tests/dynamic_normals_ref.py (the
definition in float32 NumPy, one rounding per operation), the positions the NRM prepare kernels store against the parts'
and the skin's restatements, and the drawn stages against the CPU checker over the ONE static mesh whose appended triangles
carry the per-corner frames.  Cases: tests/dynnormalcases.py; their premises: tests/test_dynamic_normals_cases.py.
Frames 203 x 117 and 17 x 9 and a 128^2 map in dyndrawcases' room; the voxel tests run in dyncases' 64^3 world."""
import os
import re
import subprocess

import numpy as np
import pytest

import dynamic_normals_ref as nr
import dyncases as dc
import dyndrawcases as ddc
import dynnormalcases as nc
import dynpartcases as dp
import dynskincases as ds
import emission_ref
import vctpkg
from test_gpu_dynamic import run_pass
from test_gpu_dynamic_draw import BOTH, GBUFFER_FLAG, SHADOW_FLAG, assert_map, assert_planes, bits, draw, make_ctx, upload_static

pytestmark = pytest.mark.gpu
W, H = ddc.W, ddc.H
SOURCES = ("positions", "parts", "skin")
DYN_EM = np.array([[0.5, 0.25, 2.0], [0.0, 0.0, 0.0], [1.5, 0.125, 0.25]], np.float32)


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    v = vctpkg.load()
    assert hasattr(v.lib(), "vct_set_dynamic_normals") and hasattr(v.Context, "download_dynamic_frames")
    return v


@pytest.fixture(scope="module")
def world(oracle):
    """The room, the sphere, and the checker's map and planes of the concatenated mesh with face and with corner frames."""
    static = ddc.static_mesh()
    pos, nrm, mat, pal = nc.sphere()
    w = dict(static=static, sphere=(pos, mat, pal), nrm=nrm)
    w["faceted"] = ddc.reference(oracle, ddc.concatenated(static, (pos, mat, pal)), W, H)
    w["smooth"] = ddc.reference(oracle, nr.concatenated(static, (pos, mat, pal), nrm), W, H)
    return w


def refused(vct, call, *a, **kw):
    with pytest.raises(vct.VctError) as e:
        call(*a, **kw)
    assert "(-1)" in str(e.value), str(e.value)               # VCT_ERR_INVALID
    return str(e.value)


def assert_frames(ctx, want, what):
    got = ctx.download_dynamic_frames()
    for g, x, name in zip(got, want, ("normal", "tangent", "bitangent")):
        bad = np.argwhere(bits(g) != bits(x))
        assert bad.shape[0] == 0, (what, name, bad.shape[0], bad[:4].tolist(), g[tuple(bad[0])], x[tuple(bad[0])])


def assert_positions(ctx, want, what):
    got = ctx.download_dynamic_positions()
    bad = np.argwhere(bits(got) != bits(np.ascontiguousarray(want, np.float32)))
    assert bad.shape[0] == 0, (what, "positions", bad.shape[0], bad[:4].tolist())


def movers(ntri):
    """source -> (attach(ctx), [(name, matrices, moved positions of `pos`, mover keywords of the restatement)])"""
    part = nc.parts(ntri)
    bone, weight = ds.influences(ntri)
    tables = [(f"table {s}", nc.table(s)) for s in range(len(nc.MATRICES))]
    bones = [(f"bones {s}", nc.bone_table(s)) for s in range(len(nc.MATRICES))] + [(p, nc.skin_pose(p)) for p in ds.POSES]
    return dict(
        parts=(lambda ctx: ctx.set_dynamic_parts(part, len(nc.MATRICES)), tables,
               lambda pos, m: dp.transform_ref(pos, part, m), lambda m: dict(part=part, m=m)),
        skin=(lambda ctx: ctx.set_dynamic_skin(bone, weight, ds.NBONES), bones,
              lambda pos, m: ds.skin_ref(pos, bone, weight, m), lambda m: dict(bone=bone, weight=weight, m=m)))


def check_kernel_output(vct, mesh, source, what):
    """download_dynamic_frames and the stored positions against the restatement, normals and matrices through host and
    device pointers, for one mesh (pos, nrm, mat, pal) and one source of the prepare kernel."""
    import torch
    pos, nrm, mat, pal = mesh
    ntri = pos.shape[0]
    with vct.Context(vct.default_config(voxel_dim=16, width=8, height=8, shadow_map_size=128, model_scale=ddc.MS)) as ctx:
        ctx.set_dynamic_draw(BOTH)
        ctx.set_dynamic_mesh(pos, mat, pal)
        assert ctx.dynamic_normals() is None
        assert_frames(ctx, ddc.dynamic_frames(nr.draw_copy(pos)), (what, "no normals: the face frames"))
        ctx.set_dynamic_normals(nrm)
        assert np.array_equal(bits(ctx.dynamic_normals()), bits(nrm))
        assert_frames(ctx, nr.frames(pos, nrm), (what, "normals as given"))
        if source == "positions":
            other = np.ascontiguousarray(nrm[:, ::-1])          # the corners' normals in another order: an update shows
            dev = torch.from_numpy(other).cuda()
            torch.cuda.synchronize()
            for given, src in ((other, "host"), (nrm, "host"), (int(dev.data_ptr()), "device"), (nrm.reshape(-1, 9), "host [n, 9]")):
                ctx.update_dynamic_normals(given)
                want = other if isinstance(given, int) or given is other else nrm
                assert_frames(ctx, nr.frames(pos, want), (what, "update", src))
            moved = (pos.reshape(-1, 3, 3) + np.float32(3.0)).reshape(-1, 9)
            ctx.update_dynamic_positions(moved)
            assert_frames(ctx, nr.frames(moved, nrm), (what, "positions updated"))
            return
        attach, poses, move, kw = movers(ntri)[source]
        attach(ctx)
        assert_frames(ctx, nr.frames(pos, nrm), (what, "mover attached, nothing moved yet: as given"))
        assert np.array_equal(bits(ctx.dynamic_normals()), bits(nrm))                   # the normals survived the attach
        other = np.ascontiguousarray(nrm[:, ::-1])
        dev_other = torch.from_numpy(other).cuda()
        torch.cuda.synchronize()
        for k, (name, m) in enumerate(poses):
            given = m
            if k % 2:
                dev = torch.from_numpy(m).cuda()
                torch.cuda.synchronize()
                given = int(dev.data_ptr())
            ctx.update_dynamic_transforms(given)
            p = move(pos, m)
            assert_positions(ctx, p, (what, name))
            assert_frames(ctx, nr.frames(p, nrm, **kw(m)), (what, name))
            if k in (1, 2):          # new normals under the moved mover, through a device and a host pointer: the mover's kernel again
                ctx.update_dynamic_normals(int(dev_other.data_ptr()) if k == 1 else other)
                assert_positions(ctx, p, (what, name, "normals updated"))
                assert_frames(ctx, nr.frames(p, other, **kw(m)), (what, name, "normals updated"))
                ctx.update_dynamic_normals(nrm)


# ---- 1. the kernels alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntri", nc.SIZES + (nc.NTRI,))
@pytest.mark.parametrize("source", SOURCES)
def test_frames_are_the_definition_s_bit_for_bit(vct, source, ntri):
    check_kernel_output(vct, nc.padded(ntri), source, (source, ntri))


@pytest.mark.parametrize("source", SOURCES)
def test_adversarial_corners_and_matrices(vct, source):
    check_kernel_output(vct, nc.adversarial(), source, (source, "adversarial"))


# ---- 2. the drawn stages ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", ddc.FRAMES)
@pytest.mark.parametrize("path", ["direct", "binned"])
def test_drawn_stages_positions_only(vct, oracle, world, path, w, h):
    """All 23 planes, the pixel-emission planes and the pixel-gloss plane; a scissored pass between two whole ones; the
    shadow map is the map without normals."""
    static, sphere, nrm = world["static"], world["sphere"], world["nrm"]
    cat = nr.concatenated(static, sphere, nrm)
    depth, planes = ddc.reference(oracle, cat, w, h)
    depth_faceted, planes_faceted = ddc.reference(oracle, ddc.concatenated(static, sphere), w, h)
    assert np.array_equal(bits(depth), bits(depth_faceted))
    own = ddc.owner_is_dynamic(planes)
    assert (bits(planes) != bits(planes_faceted)).any(0).sum() * 2 >= own.sum() >= (800 if w == W else 8)
    nstat = static[2].shape[0]
    E = emission_ref.pixel_emission(planes, cat[2], np.concatenate([np.zeros((nstat, 3), np.float32), DYN_EM]))
    assert (E[:, own] > 0).any()
    rows = (h + 7) // 8
    mid = (rows // 3, max(rows // 3 + 1, 2 * rows // 3))
    with make_ctx(vct, static, w, h, path=path) as ctx:
        ctx.set_gloss_classes([(0.07, 20.0), (0.2, 8.0), (0.03, 60.0)])
        ctx.upload_material_gloss((1 + np.arange(nstat) % 2).astype(np.uint8))
        ctx.set_dynamic_mesh(*sphere)
        ctx.set_dynamic_emission(DYN_EM)
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        draw(ctx, w, h)
        assert_planes(ctx, planes_faceted, f"{path} {w}x{h} before the normals", None, w, h)
        gloss_faceted = ctx.download_pixel_gloss()
        ctx.set_dynamic_normals(nrm)
        for r in (None, mid, None):
            draw(ctx, w, h, r)
            assert_map(ctx, depth, f"{path} {w}x{h} rows {r}")
            assert_planes(ctx, planes, f"{path} {w}x{h} rows {r}", r, w, h)
        assert np.array_equal(bits(ctx.download_pixel_emission()), bits(E)), "pixel emission"
        gloss = ctx.download_pixel_gloss()
        assert np.array_equal(gloss, gloss_faceted) and (gloss.reshape(-1)[own] == 0).all() and (gloss > 0).any()
        ctx.set_dynamic_normals(None)                           # detached: the face frames return
        assert ctx.dynamic_normals() is None
        draw(ctx, w, h)
        assert_planes(ctx, planes_faceted, f"{path} {w}x{h} normals detached", None, w, h)


@pytest.mark.parametrize("w,h", ddc.FRAMES)
@pytest.mark.parametrize("path", ["direct", "binned"])
@pytest.mark.parametrize("name", ["rotation", "mirror"])
def test_drawn_stages_parts(vct, oracle, world, name, path, w, h):
    static, (pos, mat, pal), nrm = world["static"], world["sphere"], world["nrm"]
    part, m = nc.one_part(nc.NTRI), nc.matrix(name)[None]
    moved = dp.transform_ref(pos, part, m)
    depth, planes = ddc.reference(oracle, nr.concatenated(static, (moved, mat, pal), nrm, part=part, m=m), w, h)
    _, rest_planes = ddc.reference(oracle, nr.concatenated(static, (pos, mat, pal), nrm), w, h)
    big = w == W
    assert ddc.owner_is_dynamic(planes).sum() >= (800 if big else 8)
    assert (bits(planes) != bits(rest_planes)).any(0).sum() >= (300 if big else 3)
    with make_ctx(vct, static, w, h, path=path) as ctx:
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        ctx.set_dynamic_mesh(pos, mat, pal)
        ctx.set_dynamic_normals(nrm)
        ctx.set_dynamic_parts(part, 1)
        draw(ctx, w, h)
        assert_planes(ctx, rest_planes, f"{name}: parts attached, not moved yet", None, w, h)
        for rnd in range(2):
            ctx.update_dynamic_transforms(m)
            draw(ctx, w, h)
            assert_map(ctx, depth, f"{name} {path} {w}x{h} {rnd}")
            assert_planes(ctx, planes, f"{name} {path} {w}x{h} {rnd}", None, w, h)


@pytest.mark.parametrize("path", ["direct", "binned"])
def test_drawn_stages_skin(vct, oracle, world, path):
    static, (pos, mat, pal), nrm = world["static"], world["sphere"], world["nrm"]
    bone, weight = nc.smooth_influences()
    seen = []
    with make_ctx(vct, static, path=path) as ctx:
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        ctx.set_dynamic_mesh(pos, mat, pal)
        ctx.set_dynamic_skin(bone, weight, ds.NBONES)
        ctx.set_dynamic_normals(nrm)                            # behind the mover: the order does not matter
        for pose in ds.POSES:
            m = nc.skin_pose(pose)
            moved = ds.skin_ref(pos, bone, weight, m)
            depth, planes = ddc.reference(oracle, nr.concatenated(static, (moved, mat, pal), nrm, bone=bone, weight=weight, m=m), W, H)
            assert ddc.owner_is_dynamic(planes).sum() >= 300, pose
            ctx.update_dynamic_transforms(m)
            draw(ctx)
            assert_map(ctx, depth, pose)
            assert_planes(ctx, planes, pose)
            seen.append(planes)
    assert (bits(seen[0]) != bits(seen[1])).any() and (bits(seen[1]) != bits(seen[2])).any()


# ---- 3. the voxel layer does not see the normals ------------------------------------------------------------------------------
def test_voxels_are_those_without_normals(vct):
    pos, mat, alb = dc.dynamic_mesh(dc.A)
    r = np.random.default_rng(5)
    nrm = r.normal(size=(pos.shape[0], 3, 3)).astype(np.float32)
    out = []
    for given in (None, nrm):
        with vct.Context(dc.config(vct)) as ctx:
            ctx.upload_triangles(*dc.static_scene())
            ctx.set_dynamic_draw(BOTH)
            ctx.set_dynamic_mesh(pos, mat, alb)
            ctx.set_dynamic_normals(given)
            run_pass(ctx)
            out.append((ctx.download_chain(),) + ctx.download_dynamic_voxels() + (ctx.dynamic_info(),))
    for a, b in zip(*out):
        assert a == b if isinstance(a, dict) else np.array_equal(a, b)
    assert (out[0][1][..., 3] > 0).sum() >= 100 and (out[0][3] != 0).any()


# ---- 4. life cycle ------------------------------------------------------------------------------------------------------------
def test_life_cycle_and_ordering(vct, world):
    static, (pos, mat, pal), nrm = world["static"], world["sphere"], world["nrm"]
    face, smooth = ddc.dynamic_frames(pos), nr.frames(pos, nrm)
    other = np.ascontiguousarray(nrm[:, ::-1])
    part, m = nc.one_part(nc.NTRI), nc.matrix("rotation")[None]
    moved = dp.transform_ref(pos, part, m)
    with make_ctx(vct, static) as ctx:
        ctx.set_dynamic_mesh(pos, mat, pal)
        ctx.set_dynamic_normals(nrm)                            # no flag on: stored, nothing launched, no arrays
        refused(vct, ctx.download_dynamic_frames)
        assert np.array_equal(bits(ctx.dynamic_normals()), bits(nrm))
        ctx.set_dynamic_draw(GBUFFER_FLAG)                      # the flag goes on behind the normals: the frames appear
        assert_frames(ctx, smooth, "flag on after the normals")
        ctx.update_dynamic_normals(other)
        assert_frames(ctx, nr.frames(pos, other), "update")
        ctx.set_dynamic_normals(None)
        assert ctx.dynamic_normals() is None
        assert_frames(ctx, face, "detached")
        refused(vct, ctx.update_dynamic_normals, nrm)
        ctx.set_dynamic_normals(nrm)
        assert_frames(ctx, smooth, "attached again")
        # either order of the two updates gives the same frames
        shifted = (pos.reshape(-1, 3, 3) + np.float32(2.0)).reshape(-1, 9)
        ctx.update_dynamic_normals(other); ctx.update_dynamic_positions(shifted)
        a = ctx.download_dynamic_frames()
        ctx.update_dynamic_positions(pos); ctx.update_dynamic_normals(nrm)
        ctx.update_dynamic_positions(shifted); ctx.update_dynamic_normals(other)
        assert_frames(ctx, a, "positions then normals")
        assert_frames(ctx, nr.frames(shifted, other), "both updated")
        ctx.update_dynamic_positions(pos); ctx.update_dynamic_normals(nrm)
        # a mover attached, replaced and detached leaves the normals
        ctx.set_dynamic_parts(part, 1)
        ctx.update_dynamic_transforms(m)
        assert_frames(ctx, nr.frames(moved, nrm, part=part, m=m), "parts")
        ctx.set_dynamic_parts(part, 1)                          # replaced in the moved pose: the moved positions are the rest
        assert_frames(ctx, nr.frames(moved, nrm), "parts replaced: as given on the new rest")
        ctx.set_dynamic_parts(None)
        assert np.array_equal(bits(ctx.dynamic_normals()), bits(nrm))
        assert_frames(ctx, nr.frames(moved, nrm), "parts detached: as given")
        bone, weight = nc.smooth_influences()
        ctx.update_dynamic_positions(pos)
        ctx.set_dynamic_skin(bone, weight, ds.NBONES)
        ctx.update_dynamic_transforms(nc.skin_pose("P1"))
        assert_frames(ctx, nr.frames(ds.skin_ref(pos, bone, weight, nc.skin_pose("P1")), nrm, bone=bone, weight=weight,
                                     m=nc.skin_pose("P1")), "skin")
        ctx.update_dynamic_positions(pos)                       # positions with a mover attached: new rest, nothing moved
        assert_frames(ctx, smooth, "positions under a skin")
        ctx.set_dynamic_draw(0)
        ctx.set_dynamic_draw(BOTH)                              # the flag goes on again over mover and normals
        assert_frames(ctx, smooth, "flag on again")
        ctx.update_dynamic_transforms(nc.skin_pose("P2"))
        ctx.set_dynamic_draw(0); ctx.set_dynamic_draw(SHADOW_FLAG)
        assert_frames(ctx, nr.frames(ds.skin_ref(pos, bone, weight, nc.skin_pose("P2")), nrm, bone=bone, weight=weight,
                                     m=nc.skin_pose("P2")), "flag on again in a moved pose")
        assert_positions(ctx, ds.skin_ref(pos, bone, weight, nc.skin_pose("P2")), "flag on again in a moved pose")
        # the mesh drops them: replace and detach
        ctx.set_dynamic_mesh(pos, mat, pal)
        assert ctx.dynamic_normals() is None
        assert_frames(ctx, face, "mesh replaced")
        ctx.set_dynamic_normals(nrm)
        ctx.set_dynamic_mesh(None)
        refused(vct, ctx.set_dynamic_normals, nrm)
        ctx.set_dynamic_mesh(pos, mat, pal)
        assert ctx.dynamic_normals() is None
        assert_frames(ctx, face, "attached again")


def test_refusals_leave_everything_as_it_was(vct, world):
    static, (pos, mat, pal), nrm = world["static"], world["sphere"], world["nrm"]
    L = vct.lib()
    p = nrm.ctypes.data
    with make_ctx(vct, static) as ctx:
        refused(vct, ctx._ck, L.vct_set_dynamic_normals(ctx._h, p), "vct_set_dynamic_normals")          # no mesh
        refused(vct, ctx._ck, L.vct_update_dynamic_normals(ctx._h, p, vct.MEM_HOST), "vct_update_dynamic_normals")
        refused(vct, ctx._ck, L.vct_download_dynamic_frames(ctx._h, None, None, None), "vct_download_dynamic_frames")
        ctx.set_dynamic_draw(BOTH)
        ctx.set_dynamic_mesh(pos, mat, pal)
        refused(vct, ctx._ck, L.vct_update_dynamic_normals(ctx._h, p, vct.MEM_HOST), "vct_update_dynamic_normals")   # none attached
        ctx.set_dynamic_normals(nrm)
        before = ctx.download_dynamic_frames()
        refused(vct, ctx._ck, L.vct_update_dynamic_normals(ctx._h, None, vct.MEM_HOST), "vct_update_dynamic_normals")
        refused(vct, ctx._ck, L.vct_update_dynamic_normals(ctx._h, p, 7), "vct_update_dynamic_normals")
        refused(vct, ctx._ck, L.vct_update_dynamic_normals(ctx._h, p + 2, vct.MEM_HOST), "vct_update_dynamic_normals")
        for shape in ((nc.NTRI, 3, 2), (nc.NTRI + 1, 3, 3), (nc.NTRI - 1, 9), (nc.NTRI * 9,)):
            for call in (ctx.set_dynamic_normals, ctx.update_dynamic_normals):
                with pytest.raises(vct.VctError) as e:
                    call(np.zeros(shape, np.float32))
                assert "triangles" in str(e.value)
        assert L.vct_set_dynamic_normals(None, p) != 0 and L.vct_update_dynamic_normals(None, p, 0) != 0
        assert L.vct_get_dynamic_normals(None, None, None) != 0 and L.vct_get_dynamic_normals(ctx._h, None, None) != 0
        assert L.vct_download_dynamic_frames(None, None, None, None) != 0
        assert np.array_equal(bits(ctx.dynamic_normals()), bits(nrm))
        assert_frames(ctx, before, "after the refusals")
        ctx.set_dynamic_draw(0)
        refused(vct, ctx.download_dynamic_frames)               # no flag on: the arrays are not handed out


def test_two_frame_slots_against_a_single_slot_replay(vct, world):
    static, (pos, mat, pal), nrm = world["static"], world["sphere"], world["nrm"]
    other = np.ascontiguousarray(nrm[:, ::-1])
    seq = [nrm, other, nrm, nrm, other, other, nrm]
    with make_ctx(vct, static) as two, make_ctx(vct, static) as one:
        for c in (two, one):
            c.set_dynamic_mesh(pos, mat, pal)
            c.set_dynamic_draw(BOTH, ddc.SPECULAR)
            c.set_dynamic_normals(nrm)
        two.set_frames_in_flight(2)
        for k, n in enumerate(seq):            # nothing is read back in between: the slots' work stays in flight
            two.select_frame_slot(k & 1)
            two.update_dynamic_normals(n)
            draw(two)
        got = []
        for slot in (0, 1):
            two.select_frame_slot(slot)
            got.append(two.download_gbuffer())
        for slot, n in ((0, seq[6]), (1, seq[5])):
            one.update_dynamic_normals(n)
            draw(one)
            assert np.array_equal(bits(got[slot]), bits(one.download_gbuffer())), slot
        assert np.array_equal(bits(got[0]), bits(world["smooth"][1])) and (bits(got[0]) != bits(got[1])).any()


def test_gi_pass_against_the_separate_calls_and_the_traced_frame(vct, world):
    """vct_gi_pass against the separate calls, and the library's frame over the smooth G-buffer against the frame traced
    from the checker's planes (the pattern of tests/test_gpu_dynamic_draw.py)."""
    static, sphere, nrm = world["static"], world["sphere"], world["nrm"]

    def ctx_of():
        c = make_ctx(vct, static, V=64, grid_world_size=64.0, voxel_attributes=1)
        c.set_camera_position((0.0, 0.0, 0.0)); c.set_light_direction((0.0, 1.0, 0.6))
        c.set_dynamic_mesh(*sphere)
        c.set_dynamic_draw(BOTH, ddc.SPECULAR)
        c.set_dynamic_normals(nrm)
        return c
    with ctx_of() as fused, ctx_of() as ref:
        for rnd in range(2):
            fused.gi_pass(ddc.light_vp(), ddc.camera(W, H))
            ref.render_shadow_map(ddc.light_vp())
            run_pass(ref)
            ref.render_gbuffer(ddc.camera(W, H))
            ref.trace_resident()
            for c, what in ((fused, "gi_pass"), (ref, "separate calls")):
                assert_map(c, world["smooth"][0], f"{what} {rnd}")
                assert_planes(c, world["smooth"][1], f"{what} {rnd}")
            assert np.array_equal(fused.download_chain(), ref.download_chain())
            assert np.array_equal(fused.download_frame(), ref.download_frame())
        frame = ref.download_frame()
        assert np.array_equal(frame, ref.trace(world["smooth"][1]))
        assert (frame != ref.trace(world["faceted"][1])).any(-1).sum() >= 300


# ---- 5. readers ---------------------------------------------------------------------------------------------------------------
def test_the_half_rate_gather_marches_fewer_pixels_over_smooth_normals(vct, world):
    """vct_set_diffuse_rate(ctx, 2): the normal test of the gather rejects neighbours across every facet edge, so faceted
    the sphere's pixels march their own cones more often.  Only the sphere's pixels differ between the two G-buffers
    (tests/test_dynamic_normals_cases.py), so the difference of the frame's counts is the difference on the sphere."""
    static, sphere, nrm = world["static"], world["sphere"], world["nrm"]
    own = int(ddc.owner_is_dynamic(world["smooth"][1]).sum())
    with make_ctx(vct, static, V=64, grid_world_size=64.0, voxel_attributes=1) as ctx:
        ctx.set_camera_position((0.0, 0.0, 0.0)); ctx.set_light_direction((0.0, 1.0, 0.6))
        ctx.set_dynamic_mesh(*sphere)
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        ctx.set_diffuse_rate(2)
        marched = []
        for given in (None, nrm):
            ctx.set_dynamic_normals(given)
            draw(ctx)
            run_pass(ctx)
            ctx.trace_resident()
            rate, n = ctx.diffuse_rate()
            assert rate == 2
            marched.append(n)
        print(f"pixels that marched their diffuse cones: faceted {marched[0]}, smooth {marched[1]}; the sphere owns {own}")
        assert marched[1] < marched[0]


# ---- 6. the demo --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mover", ["alone", "path", "spin", "bend"])
def test_the_demo_draws_smooth(vct, tmp_path, mover):
    """vct_demo --dynamic-obj FILE --dynamic-draw both [--dynamic-path | --dynamic-spin | --dynamic-bend] with and without
    --dynamic-smooth: the frame of the last Render() differs (a sphere with vn records in the middle of the hall)."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxel-cone-tracing_amd", "vct_demo")
    assert os.path.exists(exe), "build it with `make demo`"
    pos, nrm, _, _ = nc.sphere()
    v = (pos.reshape(-1, 3).astype(np.float64) - nc.CENTRE_MODEL) * 4.0            # a sphere of 150 model units in the hall
    n = nrm.reshape(-1, 3)
    obj = tmp_path / "sphere.obj"
    obj.write_text("".join(f"v {x:.6f} {y:.6f} {z:.6f}\n" for x, y, z in v) + "".join(f"vn {x:.6f} {y:.6f} {z:.6f}\n" for x, y, z in n) +
                   "".join(f"f {3 * t + 1}//{3 * t + 1} {3 * t + 2}//{3 * t + 2} {3 * t + 3}//{3 * t + 3}\n" for t in range(nc.NTRI)))
    args = {"alone": (), "path": ("--dynamic-path", "0,0,0;60,0,0"), "spin": ("--dynamic-spin", "0,1,0;20"),
            "bend": ("--dynamic-bend", "0,0,1;15")}[mover]

    def frame(*more):
        out = subprocess.run([exe, "--voxels", "64", "--size", "64x64", "--shadow", "256", "--frames", "2", "--dynamic-obj", str(obj),
                              "--dynamic-draw", "both", *args, *more], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert f"dynamic mesh: triangles={nc.NTRI}" in out.stdout, out.stdout[-1000:]
        return re.search(r"fnv1a=([0-9a-f]{16})", out.stdout).group(1)
    faceted = frame()
    assert faceted != frame("--dynamic-smooth")
    assert faceted == frame()          # without the option nothing of it runs: the same frame again
