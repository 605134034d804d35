"""GPU: the dynamic mesh (include/vct.h "dynamic mesh") -- a second mesh voxelized by itself in every pass and merged
into level 0 behind the static resolve -- bit-equal to the CPU oracle: the layer alone is voxelize_conservative_attr of
the dynamic mesh, the chain is build_mips(where(D.a > 0, D, S)).  Scenes and their non-degeneracy in tests/dyncases.py
(checked without a GPU by tests/test_dynamic_cases.py); every test asserts the non-degeneracy of what it compares.

All contexts: voxel_dim 64 (the edge cases: their own grid), an 8 x 8 frame, voxel attributes.  The two-slot test runs
without config.debug_outputs, which two frames in flight do not take."""
import ctypes as C

import numpy as np
import pytest

import dyncases as dc
import emission_ref
import lights_ref as lr
import point_query_ref as pq
import synth
import vctpkg
import voxcases
from test_gpu_parity import light_setup

pytestmark = pytest.mark.gpu
V, G, MS = dc.V, dc.G, dc.MS


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


NONE, ISSUE, RAISED = "none", "issue", "raised"


def shadow_maps():
    """No shadow map; light_setup(128, 9); and the same map 0.1 further from the light.  Under the second the wall the
    object at A crosses lies in full shadow where the two meshes meet (both texels black: 3 voxels differ, at B none), so
    that map alone would make "the dynamic mesh wins" nearly vacuous; the third leaves the meeting voxels partly lit."""
    depth, vp = light_setup(128, 9)
    raised = (np.round((depth + 0.1) * (2 ** 24 - 1)) / (2 ** 24 - 1)).astype(np.float32)
    return {NONE: (None, None), ISSUE: (depth.astype(np.float32), vp), RAISED: (raised, vp)}


@pytest.fixture(scope="module")
def world(oracle):
    """The static scene, the object at A and B, and every layer the tests compare with, under each shadow map.  The
    non-degeneracy conditions hold without a map and under the raised one; under light_setup's own map the geometric
    three hold and at least 100 voxels of the layer are partly shadowed."""
    w = dict(static=dc.static_scene(), A=dc.dynamic_mesh(dc.A), B=dc.dynamic_mesh(dc.B), maps=shadow_maps())
    for sh, (depth, vp) in w["maps"].items():
        w["S", sh] = dc.layer(oracle, *w["static"], depth=depth, vp=vp)
        for k in "AB":
            w[k, sh] = dc.layer(oracle, *w[k], depth=depth, vp=vp)
            if sh != ISSUE:
                dc.assert_non_degenerate(w[k, sh][0], w["S", sh][0])
    for k in "AB":
        n = dc.non_degeneracy(w[k, ISSUE][0], w["S", ISSUE][0])
        assert n["dynamic_only_bricks"] >= 1 and n["shared_bricks"] >= 1 and n["static_only_in_shared"] >= 1, n
    D, Dn = w["A", ISSUE][0], w["A", NONE][0]
    assert ((D != Dn).any(-1) & (D[..., :3] > 0).any(-1)).sum() >= 100
    return w


def run_pass(ctx):
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()


def nbricks(D):
    return int(dc.bricks(D[..., 3] > 0).sum())


def assert_layer(ctx, want, what):
    got = ctx.download_dynamic_voxels()
    for g, w, name in zip(got, want, ("radiance", "albedo", "normal")):
        bad = np.argwhere((g != w).any(-1))
        assert bad.shape[0] == 0, (what, name, bad.shape[0], bad[:4].tolist())


def assert_chain(oracle, ctx, l0, what):
    want = oracle.build_mips(l0)
    got = ctx.download_chain()
    n = l0.shape[0] ** 3
    bad = np.argwhere((got[:n] != want[:n]).any(-1).reshape(l0.shape[:3]))
    assert bad.shape[0] == 0, (what, "level 0", bad.shape[0], bad[:4].tolist())
    assert np.array_equal(got, want), (what, "mips")


def static_ctx(vct, w, shadow=NONE, **kw):
    ctx = vct.Context(dc.config(vct, **kw))
    ctx.upload_triangles(*w["static"])
    if shadow != NONE:
        ctx.upload_shadow_map(*w["maps"][shadow])
    return ctx


# ---- 1. the layer and the merge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_shadow", [NONE, ISSUE, RAISED])
def test_layer_and_merge(vct, oracle, world, with_shadow):
    S, (D, Da, Dn) = world["S", with_shadow][0], world["A", with_shadow]
    with static_ctx(vct, world, with_shadow) as ctx:
        ctx.set_dynamic_mesh(*world["A"])
        info = ctx.dynamic_info()
        assert (info["ntri"], info["nmat"], info["max_bricks"]) == (dc.NTRI, dc.NMAT, max(64, 2 * nbricks(D)))
        assert info["bricks_needed"] == info["fragments"] == 0                   # no pass resolved yet
        for rnd in range(2):                                                     # the second pass starts from cleared accumulators
            run_pass(ctx)
            assert_layer(ctx, (D, Da, Dn), f"A, shadow={with_shadow}, pass {rnd}")
            assert_chain(oracle, ctx, dc.merge(D, S), f"A, shadow={with_shadow}, pass {rnd}")
            info = ctx.dynamic_info()
            assert info["bricks_needed"] == info["bricks_used"] == nbricks(D), info
            assert info["fragments"] >= int((D[..., 3] > 0).sum()) and info["skipped"] == 0 and info["left_out"] == 0, info
        t_vox, t_merge = ctx.last_dynamic_ms()
        print(f"dynamic kernels {t_vox:.4f} ms, merge {t_merge:.4f} ms")
        assert t_vox > 0.0 and t_merge > 0.0
        # the static pools are the static mesh's: the dynamic layer has its own
        alb, nrm = ctx.voxel_attributes()
        assert np.array_equal(alb, world["S", with_shadow][1]) and np.array_equal(nrm, world["S", with_shadow][2])
        # a voxelize that follows an unresolved one discards it
        ctx.voxelize()
        run_pass(ctx)
        assert_layer(ctx, (D, Da, Dn), "after a discarded pass")
        assert_chain(oracle, ctx, dc.merge(D, S), "after a discarded pass")


# ---- 2. moving ----------------------------------------------------------------------------------------------------------------
def test_moving_object_leaves_clean_bricks(vct, oracle, world):
    S = world["S", RAISED][0]
    with static_ctx(vct, world, RAISED) as ctx:
        ctx.set_dynamic_mesh(*world["A"])
        for k in "ABA":
            ctx.update_dynamic_positions(world[k][0])
            run_pass(ctx)
            assert_layer(ctx, world[k, RAISED], f"at {k}")
            assert_chain(oracle, ctx, dc.merge(world[k, RAISED][0], S), f"at {k}")
        ctx.set_dynamic_mesh(None)
        run_pass(ctx)
        assert_chain(oracle, ctx, S, "detached")
        assert ctx.dynamic_info()["ntri"] == 0
        # the layer survives a new static mesh
        ctx.set_dynamic_mesh(*world["B"])
        pos2, mat2, alb2 = voxcases.random_scene(200, seed=12)
        ctx.upload_triangles(pos2, mat2, alb2)
        S2 = dc.layer(oracle, pos2, mat2, alb2, depth=world["maps"][RAISED][0], vp=world["maps"][RAISED][1])[0]
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(world["B", RAISED][0], S2), "B over a new static mesh")


def test_gi_pass_equals_the_six_calls(vct, oracle, world):
    """vct_gi_pass against shadow map, voxelize, inject, mips, G-buffer, trace -- the object at A, then at B -- and the six
    calls' chain against the oracle under the shadow map they rendered."""
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
            D = dc.layer(oracle, *world[k], depth=depth, vp=lvp_row)
            n = dc.non_degeneracy(D[0], S)            # (the four conditions hold for the unlit layers: `world`)
            assert n["dynamic_only_bricks"] >= 1 and n["shared_bricks"] >= 1 and n["static_only_in_shared"] >= 1, n
            assert (D[0][..., :3] > 0).any(-1).sum() >= 50 and (D[0] != world[k, NONE][0]).any(-1).sum() >= 1, k
            assert_layer(ref, D, f"six calls at {k}")
            assert_chain(oracle, ref, dc.merge(D[0], S), f"six calls at {k}")
            assert np.array_equal(fused.download_chain(), ref.download_chain()), k
            assert np.array_equal(fused.download_frame(), ref.download_frame()), k
            for a, b in zip(fused.download_dynamic_voxels(), ref.download_dynamic_voxels()):
                assert np.array_equal(a, b), k
            assert fused.last_step_count() == ref.last_step_count() > 0


# ---- 3. adversarial dynamic meshes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(voxcases.EDGE_CASES))
def test_edge_case_meshes_as_the_dynamic_mesh(vct, oracle, name):
    pos, mat, alb, ms, g, v = voxcases.EDGE_CASES[name]()
    depth, vp = light_setup(128, 9)
    spos, smat, salb = voxcases.random_scene(40, seed=12)
    spos = voxcases.rescale(spos, ms, g)
    S = dc.layer(oracle, spos, smat, salb, ms, g, v, depth, vp)[0]
    D = dc.layer(oracle, pos, mat, alb, ms, g, v, depth, vp)
    assert (D[0][..., 3] > 0).any() and (S[..., 3] > 0).any()
    apos, amat, aalb = dc.dynamic_mesh(dc.A)
    apos = voxcases.rescale(apos, ms, g)
    DA = dc.layer(oracle, apos, amat, aalb, ms, g, v, depth, vp)
    assert (DA[0][..., 3] > 0).sum() >= 50
    with vct.Context(dc.config(vct, v, g, ms)) as ctx:
        ctx.upload_triangles(spos, smat, salb)
        ctx.upload_shadow_map(depth, vp)
        ctx.set_dynamic_mesh(pos, mat, alb)
        run_pass(ctx)
        info = ctx.dynamic_info()
        assert info["left_out"] == 0 and info["skipped"] == 0 and info["bricks_used"] == nbricks(D[0]), info
        assert_layer(ctx, D, name)
        assert_chain(oracle, ctx, dc.merge(D[0], S), name)
        ctx.set_dynamic_mesh(apos, amat, aalb)                     # an ordinary object on the same context
        run_pass(ctx)
        assert_layer(ctx, DA, name + ", then A")
        assert_chain(oracle, ctx, dc.merge(DA[0], S), name + ", then A")


# ---- 4. the vertex contract, on the device ---------------------------------------------------------------------------------
def test_out_of_contract_triangles_are_skipped(vct, oracle, world):
    import torch
    S = world["S", NONE][0]
    pos, mat, alb = world["A"]
    beyond, inside = voxcases.at_the_bound(MS, G, inside=False), voxcases.at_the_bound(MS, G, inside=True)
    assert np.nextafter(inside, np.float32(np.inf)) == beyond
    bad = pos.copy()
    poison = {3: np.nan, 17: np.inf, 40: -np.inf, 64: beyond, 65: -beyond, 149: np.nan}      # triangle -> value
    for i, (t, value) in enumerate(poison.items()):
        bad[t, (4 * i) % 9] = value
    keep = np.ones(pos.shape[0], bool)
    keep[list(poison)] = False
    D = dc.layer(oracle, pos[keep], mat[keep], alb)
    assert (D[0] != world["A", NONE][0]).any()                    # the skipped triangles had fragments
    dc.assert_non_degenerate(D[0], S)
    edge = pos.copy()
    edge[7, 2] = inside                                             # the last value inside the bound is a vertex like any other
    edge[8, 3] = -inside
    De = dc.layer(oracle, edge, mat, alb)
    with static_ctx(vct, world) as ctx:
        ctx.set_dynamic_mesh(pos, mat, alb)
        for arr, want, skipped, what in ((bad, D, len(poison), "poisoned"), (edge, De, 0, "at the bound"), (pos, world["A", NONE], 0, "clean")):
            dev = torch.from_numpy(arr).cuda()
            torch.cuda.synchronize()
            ctx.update_dynamic_positions(dev.data_ptr())
            run_pass(ctx)
            assert_layer(ctx, want, what)
            assert_chain(oracle, ctx, dc.merge(want[0], S), what)
            info = ctx.dynamic_info()
            assert info["skipped"] == skipped and info["left_out"] == 0, (what, info)
        # the same rule for host positions, also at the attach
        ctx.set_dynamic_mesh(bad, mat, alb)
        run_pass(ctx)
        assert_layer(ctx, D, "poisoned, attached from the host")
        assert ctx.dynamic_info()["skipped"] == len(poison)


# ---- 5. capacity ------------------------------------------------------------------------------------------------------------
def test_a_pass_beyond_the_capacity_is_the_static_chain(vct, oracle, world):
    S, DA, DB = world["S", NONE][0], world["A", NONE], world["B", NONE]
    need_a, need_b = nbricks(DA[0]), nbricks(DB[0])
    empty = tuple(np.zeros_like(x) for x in DA)
    with static_ctx(vct, world) as ctx:
        ctx.set_dynamic_mesh(*world["A"], max_bricks=need_a - 1)
        for _ in range(2):
            run_pass(ctx)                                           # no error
            assert_chain(oracle, ctx, S, "left out")
            assert_layer(ctx, empty, "left out")
            info = ctx.dynamic_info()
            assert (info["max_bricks"], info["bricks_needed"], info["bricks_used"], info["left_out"]) == (need_a - 1, need_a, 0, 1), info
        ctx.set_dynamic_mesh(*world["A"], max_bricks=need_a)        # exactly enough
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(DA[0], S), "exact capacity")
        assert ctx.dynamic_info()["left_out"] == 0
        cap = 0 if need_b <= max(64, 2 * need_a) else need_b        # the default, unless B would not fit it
        ctx.set_dynamic_mesh(*world["A"], max_bricks=cap)
        run_pass(ctx)
        assert_layer(ctx, DA, "default capacity")
        assert_chain(oracle, ctx, dc.merge(DA[0], S), "default capacity")
        ctx.update_dynamic_positions(world["B"][0])
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(DB[0], S), "B on that capacity")
        info = ctx.dynamic_info()
        assert info["bricks_used"] == need_b and info["left_out"] == 0, info
        # left out after a resolved pass: the layer of that pass is gone from the chain and from the downloads
        ctx.set_dynamic_mesh(*world["B"], max_bricks=need_b)
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(DB[0], S), "B, exact")
        both = np.concatenate([world["A"][0], world["B"][0]])[: dc.NTRI * 2: 2]
        Dboth = dc.layer(oracle, both, world["A"][1], world["A"][2])
        assert nbricks(Dboth[0]) > need_b
        ctx.update_dynamic_positions(both)
        run_pass(ctx)
        assert_chain(oracle, ctx, S, "left out after a resolved pass")
        assert_layer(ctx, empty, "left out after a resolved pass")
        ctx.update_dynamic_positions(world["B"][0])
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(DB[0], S), "B again")


# ---- 6. with the neighbours ----------------------------------------------------------------------------------------------------
def test_local_lights_light_both_layers(vct, oracle, world):
    (S, Sa, Sn), (D, Da, Dn) = world["S", RAISED], world["A", RAISED]
    lights = lr.many_lights(8)
    lit_s, lit_d = lr.level0(S, Sa, Sn, lights, G), lr.level0(D, Da, Dn, lights, G)
    assert (lit_d != D).any(-1).sum() >= 50 and (lit_s != S).any(-1).sum() >= 50
    want = np.where((D[..., 3] > 0)[..., None], lit_d, lit_s)
    with static_ctx(vct, world, RAISED) as ctx:
        ctx.set_lights(lights)
        ctx.set_dynamic_mesh(*world["A"])
        run_pass(ctx)
        assert_chain(oracle, ctx, want, "8 lights")
        assert_layer(ctx, (D, Da, Dn), "8 lights: the layer is the unlit one")
        # moved: the slots the object left hold no attributes a light could find
        (DB, DBa, DBn) = world["B", RAISED]
        ctx.update_dynamic_positions(world["B"][0])
        run_pass(ctx)
        assert_chain(oracle, ctx, np.where((DB[..., 3] > 0)[..., None], lr.level0(DB, DBa, DBn, lights, G), lit_s), "8 lights at B")
        ctx.set_lights(None)
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(DB, S), "lights detached")


def test_static_emission_lies_under_the_dynamic_layer(vct, oracle, world):
    pos, mat, alb = world["static"]
    D = world["A", NONE][0]
    p = oracle.default_params(V, G=G)
    table = emission_ref.EMISSION.copy()
    table[mat[3]] = (0.3, 0.1, 0.6)                                  # the wall the object crosses glows too
    S1, L, Em = emission_ref.level0(oracle, p, pos, mat, alb, table)
    glows, d = (S1 != L).any(-1), D[..., 3] > 0
    inside = np.repeat(np.repeat(np.repeat(dc.bricks(d), 8, 0), 8, 1), 8, 2)
    assert (glows & d).sum() >= 10 and (glows & ~d & inside).sum() >= 10      # emission under the object, and beside it in its bricks
    with static_ctx(vct, world) as ctx:
        ctx.upload_emission(table)
        ctx.set_dynamic_mesh(*world["A"])
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(D, S1), "emission")


def test_footprint_records_and_point_queries_read_the_merged_chain(vct, oracle, world):
    S, D = world["S", NONE][0], world["A", NONE][0]
    planes = synth.random_gbuffer(64, seed=42, discard_frac=0.05)
    r = np.random.default_rng(4)
    P = np.asarray(dc.A) * MS + r.uniform(-20.0, 20.0, (64, 3))
    nn = r.normal(size=(64, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    h = np.where(np.abs(nn[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = np.cross(h, nn)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    pts = np.ascontiguousarray(np.concatenate([P, nn * MS, t * MS, np.cross(nn, t) * MS], 1), np.float32)
    merged = oracle.build_mips(dc.merge(D, S))
    p = oracle.default_params(V, G=G)
    ref, ref_static = pq.gather(oracle, p, merged, pts), pq.gather(oracle, p, oracle.build_mips(S), pts)
    assert (pq.u32(ref["gather"]) != pq.u32(ref_static["gather"])).any(-1).sum() >= 16      # the object shows in the gathers
    with static_ctx(vct, world) as ctx:
        ctx.set_dynamic_mesh(*world["A"])
        run_pass(ctx)
        plain = ctx.trace(planes)
        pq.assert_floats_match(ctx.gather_points(pts), ref["gather"], "gather around A")
        ctx.set_footprint_records(True)
        run_pass(ctx)
        assert np.array_equal(ctx.trace(planes), plain)
        ctx.update_dynamic_positions(world["B"][0])
        run_pass(ctx)
        with_records = ctx.trace(planes)
        ctx.set_footprint_records(False)
        assert np.array_equal(ctx.trace(planes), with_records)
        assert not np.array_equal(with_records, plain)


# ---- 7. two frame slots --------------------------------------------------------------------------------------------------------
def test_updates_and_passes_alternating_on_two_slots(vct, oracle, world):
    planes = synth.random_gbuffer(64, seed=42, discard_frac=0.05)
    S = world["S", RAISED][0]
    order = "ABABBA"

    def play(sync):
        out = []
        with static_ctx(vct, world, RAISED, debug_outputs=0) as ctx:
            ctx.set_frames_in_flight(2)
            ctx.set_dynamic_mesh(*world["A"])
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
        assert np.array_equal(want[i][1], oracle.build_mips(dc.merge(world[k, RAISED][0], S))), (i, k)
    assert not np.array_equal(want[0][0], want[1][0])


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(vct, oracle, world):
    S, D = world["S", NONE][0], world["A", NONE][0]
    pos, mat, alb = world["A"]
    L = vct.lib()
    with static_ctx(vct, world) as ctx:
        def refused(call, *a, **kw):
            with pytest.raises(vct.VctError) as e:
                call(*a, **kw)
            assert "(-1)" in str(e.value), str(e.value)               # VCT_ERR_INVALID

        refused(ctx.update_dynamic_positions, pos)                     # nothing attached
        ctx.set_dynamic_mesh(pos, mat, alb)
        run_pass(ctx)
        info, chain = ctx.dynamic_info(), ctx.download_chain()
        assert_chain(oracle, ctx, dc.merge(D, S), "before the refusals")

        def unchanged(what):
            assert ctx.dynamic_info() == info, what
            assert np.array_equal(ctx.download_chain(), chain), what
        refused(ctx.voxelize, vct.VOX_REFERENCE); unchanged("reference mode")
        refused(ctx.bounce); unchanged("bounce")
        bad_mat = mat.copy(); bad_mat[5] = dc.NMAT
        refused(ctx.set_dynamic_mesh, pos, bad_mat, alb); unchanged("material out of range")
        bad_mat[5] = -1
        refused(ctx.set_dynamic_mesh, pos, bad_mat, alb); unchanged("negative material")
        refused(ctx.set_dynamic_mesh, pos, mat, alb, max_bricks=-1); unchanged("max_bricks < 0")
        p = pos.ctypes.data_as(C.c_void_p)
        m = mat.ctypes.data_as(C.c_void_p)
        a = alb.ctypes.data_as(C.c_void_p)
        for args in ((p, None, dc.NTRI, a, dc.NMAT, 0), (p, m, dc.NTRI, None, dc.NMAT, 0), (p, m, -1, a, dc.NMAT, 0),
                     (p, m, (1 << 20) + 1, a, dc.NMAT, 0), (p, m, dc.NTRI, a, 0, 0)):
            assert L.vct_set_dynamic_mesh(ctx._h, *args) == -1, args[2:]
            unchanged(args[2:])
        assert L.vct_update_dynamic_positions(ctx._h, p, 2) == -1; unchanged("unknown location")
        assert L.vct_update_dynamic_positions(ctx._h, None, 0) == -1; unchanged("null positions")
        run_pass(ctx)                                                  # and the context still works
        assert_chain(oracle, ctx, dc.merge(D, S), "after the refusals")
        # detached: reference mode and the bounce are back
        ctx.set_dynamic_mesh(None)
        run_pass(ctx)
        ctx.bounce()
        ctx.voxelize(vct.VOX_REFERENCE); ctx.inject_light(); ctx.build_mips()


# ---- the demo -----------------------------------------------------------------------------------------------------------------
def test_the_demo_moves_an_obj_through_the_scene(vct, tmp_path):
    """vct_demo --dynamic-obj / --dynamic-path: the facade's SetDynamicMesh / UpdateDynamicMesh, a whole GI pass per frame."""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxel-cone-tracing_amd", "vct_demo")
    assert os.path.exists(exe), "build it with `make demo`"
    obj = tmp_path / "quad.obj"
    obj.write_text("v -100 -180 -100\nv 100 -180 -100\nv 100 -180 100\nv -100 -180 100\nf 1 2 3\nf 1 3 4\n")

    def run(*args):
        out = subprocess.run([exe, "--voxels", "64", "--size", "32x32", "--shadow", "256", "--frames", "3", *args],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout
    moved = run("--dynamic-obj", str(obj), "--dynamic-path", "-600,0,0;600,0,0")
    m = re.search(r"dynamic mesh: triangles=2 bricks=(\d+) of (\d+) fragments=(\d+) skipped=0 left_out=0 voxelize_ms=([0-9.]+) "
                  r"merge_ms=([0-9.]+)", moved)
    assert m, moved
    assert int(m.group(1)) >= 1 and int(m.group(3)) >= 20 and float(m.group(4)) > 0.0 and float(m.group(5)) > 0.0
    frame = lambda text: re.search(r"fnv1a=([0-9a-f]{16})", text).group(1)
    plain = run("--dynamic-light")
    assert "dynamic mesh" not in plain
    assert frame(moved) != frame(plain)                       # the object shows in the cones
