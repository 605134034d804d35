"""GPU: the forms of the dynamic mesh (include/vct.h "dynamic mesh") that tests/test_gpu_dynamic.py does not run, bit-equal
to the CPU oracle like that file and with its helpers:

  A  contexts without voxel attributes: k_dyn_tris<true,false>, k_dyn_big<true,false>, k_dyn_merge<false>; the expected
     layer is oracle.voxelize_conservative of the dynamic mesh alone
  B  dc.big_triangles(): more big triangles than k_dyn_big has workgroups (its grid-stride loop takes a second trip), every
     brick of the grid claimed by hundreds of workgroups at once, a layer whose capacity is the whole grid
  C  grids of 8^3 (one brick), 16^3, 128^3 and 256^3 (brick indices beyond 9 bits, Morton codes beyond 18)
  D  the readers include/vct.h names and no test ran with a mesh attached -- directional chains, the voxel view, a rank's
     frame step -- a pass over an uploaded volume, emission and lights together, the layer replaced or detached between
     vct_voxelize and vct_inject_light, and vct_last_dynamic_ms with timing off

The premises (non-degeneracy of every scene, the big-triangle count by the library's box rule, the equality of the two oracle
voxelizers' level 0) are checked without a GPU by tests/test_dynamic_cases.py; every test here asserts, on the oracle's
output, the non-degeneracy of what it compares."""
import ctypes as C

import numpy as np
import pytest

import dyncases as dc
import emission_ref
import lights_ref as lr
import voxcases
import voxel_view_ref as vv
from test_gpu_dynamic import NONE, RAISED, assert_chain, assert_layer, nbricks, run_pass, shadow_maps, static_ctx, vct, world  # noqa: F401

pytestmark = pytest.mark.gpu
V, G, MS = dc.V, dc.G, dc.MS
INFO_KEYS = ("ntri", "nmat", "max_bricks", "bricks_needed", "bricks_used", "fragments", "skipped", "left_out")


def refused(vct, call, *a, **kw):
    with pytest.raises(vct.VctError) as e:
        call(*a, **kw)
    assert "(-1)" in str(e.value), str(e.value)                       # VCT_ERR_INVALID


def occupied(D):
    return int((D[..., 3] > 0).sum())


def resolved(ctx, D, what):
    """dynamic_info() of a pass that resolved layer D within its capacity."""
    info = ctx.dynamic_info()
    assert info["bricks_needed"] == info["bricks_used"] == nbricks(D) and info["fragments"] >= occupied(D), (what, info)
    assert info["skipped"] == 0 and info["left_out"] == 0, (what, info)
    return info


# ---- A. no voxel attributes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_shadow", [NONE, RAISED])
def test_no_attributes_layer_and_merge(vct, oracle, world, with_shadow):
    """Two passes at A, then A -> B -> A, then detached; vct_get_dynamic as on a context with attributes."""
    S = world["S", with_shadow][0]
    depth, vp = world["maps"][with_shadow]
    for k in "AB":      # the layer of this form is the plain voxelizer's (equal to the other's level 0: test_dynamic_cases.py)
        assert np.array_equal(dc.layer_plain(oracle, *world[k], depth=depth, vp=vp), world[k, with_shadow][0])
    with static_ctx(vct, world, with_shadow, voxel_attributes=0) as ctx, static_ctx(vct, world, with_shadow) as full:
        for c in (ctx, full):
            c.set_dynamic_mesh(*world["A"])
        assert ctx.dynamic_info() == full.dynamic_info()
        assert ctx.dynamic_info()["max_bricks"] == max(64, 2 * nbricks(world["A", with_shadow][0]))
        for rnd, k in enumerate("AABA"):
            D = world[k, with_shadow][0]
            for c in (ctx, full):
                c.update_dynamic_positions(world[k][0])
                run_pass(c)
            got = ctx.download_dynamic_voxels()
            assert got[1] is None and got[2] is None
            assert_layer(ctx, (D,), f"no attributes, {k}, shadow={with_shadow}, pass {rnd}")
            assert_chain(oracle, ctx, dc.merge(D, S), f"no attributes, {k}, shadow={with_shadow}, pass {rnd}")
            assert resolved(ctx, D, k) == full.dynamic_info()
        ctx.set_dynamic_mesh(None)
        run_pass(ctx)
        assert_chain(oracle, ctx, S, "no attributes, detached")
        assert ctx.dynamic_info() == dict.fromkeys(INFO_KEYS, 0)


def test_no_attributes_downloads(vct, oracle, world):
    """Radiance alone is downloaded; an albedo or normal pointer is refused and leaves chain and statistics alone."""
    S, D = world["S", NONE][0], world["A", NONE][0]
    L = vct.lib()
    with static_ctx(vct, world, voxel_attributes=0) as ctx:
        ctx.set_dynamic_mesh(*world["A"])
        run_pass(ctx)
        info, chain = ctx.dynamic_info(), ctx.download_chain()
        bufs = [np.zeros((V, V, V, 4), np.uint8) for _ in range(3)]
        p = [b.ctypes.data_as(C.c_void_p) for b in bufs]
        assert L.vct_download_dynamic_voxels(ctx._h, p[0], None, None) == 0
        assert occupied(D) >= 400 and np.array_equal(bufs[0], D)
        for args in ((p[0], p[1], None), (p[0], None, p[2]), (None, p[1], p[2]), (None, None, p[2])):
            assert L.vct_download_dynamic_voxels(ctx._h, *args) == -1
            assert b"voxel_attributes" in L.vct_last_error(ctx._h)
            assert ctx.dynamic_info() == info and np.array_equal(ctx.download_chain(), chain)
        assert not bufs[1].any() and not bufs[2].any()
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(D, S), "after the refused downloads")


def test_no_attributes_lights_are_refused(vct, oracle, world):
    """vct_set_lights needs the voxels' albedo and normal and refuses a context without them: neither layer can be lit.  The
    refusal leaves no lights attached and a context whose passes are merge(D, S)."""
    S, D = world["S", RAISED][0], world["A", RAISED][0]
    with static_ctx(vct, world, RAISED, voxel_attributes=0) as ctx:
        ctx.set_dynamic_mesh(*world["A"])
        run_pass(ctx)
        refused(vct, ctx.set_lights, lr.many_lights(8))
        assert ctx.lights() == []
        assert_chain(oracle, ctx, dc.merge(D, S), "lights refused, the chain as it was")
        run_pass(ctx)
        assert_layer(ctx, (D,), "after the refused lights")
        assert_chain(oracle, ctx, dc.merge(D, S), "after the refused lights")
        resolved(ctx, D, "after the refused lights")


def test_no_attributes_capacity(vct, oracle, world):
    S, DA, DB = world["S", NONE][0], world["A", NONE][0], world["B", NONE][0]
    need_a, need_b = nbricks(DA), nbricks(DB)
    empty = (np.zeros_like(DA),)
    with static_ctx(vct, world, voxel_attributes=0) as ctx:
        ctx.set_dynamic_mesh(*world["A"], max_bricks=need_a - 1)
        for _ in range(2):
            run_pass(ctx)
            assert_chain(oracle, ctx, S, "left out")
            assert_layer(ctx, empty, "left out")
            info = ctx.dynamic_info()
            assert (info["max_bricks"], info["bricks_needed"], info["bricks_used"], info["left_out"]) == (need_a - 1, need_a, 0, 1), info
        ctx.set_dynamic_mesh(*world["A"], max_bricks=need_a)
        run_pass(ctx)
        assert_layer(ctx, (DA,), "exact capacity")
        assert_chain(oracle, ctx, dc.merge(DA, S), "exact capacity")
        assert ctx.dynamic_info()["left_out"] == 0
        # left out after a resolved pass: that pass's layer is gone from the chain and from the download
        ctx.set_dynamic_mesh(*world["B"], max_bricks=need_b)
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(DB, S), "B, exact")
        both = np.concatenate([world["A"][0], world["B"][0]])[: dc.NTRI * 2: 2]
        assert nbricks(dc.layer_plain(oracle, both, world["A"][1], world["A"][2])) > need_b
        ctx.update_dynamic_positions(both)
        run_pass(ctx)
        assert_chain(oracle, ctx, S, "left out after a resolved pass")
        assert_layer(ctx, empty, "left out after a resolved pass")
        assert ctx.dynamic_info()["left_out"] == 1
        ctx.update_dynamic_positions(world["B"][0])
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(DB, S), "B again")


@pytest.mark.parametrize("name", ["whole_grid_and_a_crowded_brick", "degenerate_triangles"])
def test_no_attributes_edge_case_meshes(vct, oracle, name):
    """The two edge-case meshes with a triangle for k_dyn_big / without a normal, as the dynamic mesh of this form."""
    from test_gpu_parity import light_setup
    pos, mat, alb, ms, g, v = voxcases.EDGE_CASES[name]()
    depth, vp = light_setup(128, 9)
    spos, smat, salb = voxcases.random_scene(40, seed=12)
    spos = voxcases.rescale(spos, ms, g)
    S = dc.layer_plain(oracle, spos, smat, salb, ms, g, v, depth, vp)
    D = dc.layer_plain(oracle, pos, mat, alb, ms, g, v, depth, vp)
    assert (D[..., 3] > 0).any() and (S[..., 3] > 0).any()
    if name.startswith("whole_grid"):
        assert int((dc.box_candidates(pos, ms, g, v) > dc.VOX_BIG).sum()) >= 1
    with vct.Context(dc.config(vct, v, g, ms, voxel_attributes=0)) as ctx:
        ctx.upload_triangles(spos, smat, salb)
        ctx.upload_shadow_map(depth, vp)
        ctx.set_dynamic_mesh(pos, mat, alb)
        for rnd in range(2):
            run_pass(ctx)
            resolved(ctx, D, name)
            assert_layer(ctx, (D,), name)
            assert_chain(oracle, ctx, dc.merge(D, S), name)


# ---- B. many big triangles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", [1, 0])
def test_more_big_triangles_than_workgroups(vct, oracle, world, attributes):
    S = world["S", NONE][0]
    pos, mat, alb = dc.big_triangles()
    moved = pos.reshape(-1, 3, 3).copy()
    moved[..., 0] += np.float32(300.0)
    moved = moved.reshape(-1, 9)
    layer = (lambda p: dc.layer(oracle, p, mat, alb)) if attributes else (lambda p: (dc.layer_plain(oracle, p, mat, alb),))
    D, Dm = layer(pos), layer(moved)
    for p in (pos, moved):
        assert int((dc.box_candidates(p) > dc.VOX_BIG).sum()) >= 530          # k_dyn_big's grid is capped at 512 workgroups
    n = dc.non_degeneracy(D[0], S)
    assert n["dynamic_bricks"] == 512 and n["both_differ"] >= 2000 and n["static_only_in_shared"] >= 300, n
    assert (Dm[0] != D[0]).any(-1).sum() >= 100000 and dc.non_degeneracy(Dm[0], S)["both_differ"] >= 2000
    with static_ctx(vct, world, voxel_attributes=attributes) as ctx:
        ctx.set_dynamic_mesh(pos, mat, alb)                     # max_bricks = 0: counted by the slots-only launch, clamped to the grid
        info = ctx.dynamic_info()
        assert (info["ntri"], info["max_bricks"]) == (600, 512), info
        for what, p, want in (("first pass", pos, D), ("second pass", pos, D), ("moved", moved, Dm), ("back", pos, D)):
            ctx.update_dynamic_positions(p)
            run_pass(ctx)
            assert_layer(ctx, want, what)
            assert_chain(oracle, ctx, dc.merge(want[0], S), what)
            info = resolved(ctx, want[0], what)
            if want is D:
                assert info["bricks_used"] == 512, info


# ---- C. grid sizes ------------------------------------------------------------------------------------------------------------
_GRID = {}


def grid_world(oracle, v, shadow=NONE):
    """The scenes of dyncases on a grid of v^3, computed once per (v, shadow map)."""
    if (v, shadow) not in _GRID:
        depth, vp = shadow_maps()[shadow]
        w = dict(static=dc.static_scene(), A=dc.dynamic_mesh(dc.A), B=dc.dynamic_mesh(dc.B), depth=depth, vp=vp)
        w["S"] = dc.layer(oracle, *w["static"], V=v, depth=depth, vp=vp)
        for k in "AB":
            w["D", k] = dc.layer(oracle, *w[k], V=v, depth=depth, vp=vp)
            if v >= 128:
                dc.assert_non_degenerate(w["D", k][0], w["S"][0])
            else:           # one brick, or eight: no brick can be dynamic-only
                n = dc.non_degeneracy(w["D", k][0], w["S"][0])
                assert n["both_differ"] >= 5 and n["static_only_in_shared"] >= 50, (v, k, n)
        assert (w["D", "A"][0] != w["D", "B"][0]).any()
        _GRID[v, shadow] = w
    return _GRID[v, shadow]


def grid_ctx(vct, w, v, attributes, shadow=NONE):
    ctx = vct.Context(dc.config(vct, V=v, voxel_attributes=attributes))
    ctx.upload_triangles(*w["static"])
    if shadow != NONE:
        ctx.upload_shadow_map(w["depth"], w["vp"])
    return ctx


@pytest.mark.parametrize("attributes", [1, 0])
@pytest.mark.parametrize("v", [8, 16, 128, 256])
def test_grid_sizes(vct, oracle, v, attributes):
    w = grid_world(oracle, v)
    S, grid = w["S"][0], (v // 8) ** 3
    want = lambda k: w["D", k] if attributes else w["D", k][:1]
    with grid_ctx(vct, w, v, attributes) as ctx:
        ctx.set_dynamic_mesh(*w["A"])
        assert ctx.dynamic_info()["max_bricks"] == min(max(64, 2 * nbricks(w["D", "A"][0])), grid)
        if v == 8:
            ctx.set_dynamic_mesh(*w["A"], max_bricks=5)
            assert ctx.dynamic_info()["max_bricks"] == 1
        for k in "ABA":
            ctx.update_dynamic_positions(w[k][0])
            run_pass(ctx)
            assert_layer(ctx, want(k), f"{v}^3 at {k}")
            assert_chain(oracle, ctx, dc.merge(w["D", k][0], S), f"{v}^3 at {k}")
            resolved(ctx, w["D", k][0], f"{v}^3 at {k}")
        ctx.set_dynamic_mesh(None)
        run_pass(ctx)
        assert_chain(oracle, ctx, S, f"{v}^3 detached")


def test_capacity_and_shadow_map_at_128(vct, oracle):
    v = 128
    w = grid_world(oracle, v)
    S, DA = w["S"][0], w["D", "A"]
    need = nbricks(DA[0])
    empty = tuple(np.zeros_like(x) for x in DA)
    with grid_ctx(vct, w, v, 1) as ctx:
        ctx.set_dynamic_mesh(*w["A"], max_bricks=need - 1)
        run_pass(ctx)
        assert_chain(oracle, ctx, S, "128^3 left out")
        assert_layer(ctx, empty, "128^3 left out")
        info = ctx.dynamic_info()
        assert (info["max_bricks"], info["bricks_needed"], info["bricks_used"], info["left_out"]) == (need - 1, need, 0, 1), info
        ctx.set_dynamic_mesh(*w["A"], max_bricks=need)
        run_pass(ctx)
        assert_layer(ctx, DA, "128^3 exact capacity")
        assert_chain(oracle, ctx, dc.merge(DA[0], S), "128^3 exact capacity")
        assert ctx.dynamic_info()["left_out"] == 0
    r = grid_world(oracle, v, RAISED)
    assert (r["D", "A"][0] != DA[0]).any(-1).sum() >= 100              # the map shows in the layer
    with grid_ctx(vct, r, v, 1, RAISED) as ctx:
        ctx.set_dynamic_mesh(*r["A"])
        run_pass(ctx)
        assert_layer(ctx, r["D", "A"], "128^3 under the raised map")
        assert_chain(oracle, ctx, dc.merge(r["D", "A"][0], r["S"][0]), "128^3 under the raised map")


# ---- D. the readers vct.h names, and the neighbours together ----------------------------------------------------------------
def test_directional_chains_follow_the_merged_chain(vct, oracle, world):
    S = world["S", NONE][0]
    want = {k: oracle.build_mips_aniso(dc.merge(world[k, NONE][0], S)) for k in "AB"}
    want["S"] = oracle.build_mips_aniso(S)
    for a, b in (("A", "B"), ("A", "S"), ("B", "S")):
        assert (want[a] != want[b]).any(-1).sum() >= 1000, (a, b)
    with static_ctx(vct, world, anisotropic_mips=1) as ctx:
        ctx.set_dynamic_mesh(*world["A"])
        for k in "ABA":
            ctx.update_dynamic_positions(world[k][0])
            run_pass(ctx)
            assert_chain(oracle, ctx, dc.merge(world[k, NONE][0], S), f"aniso context at {k}")
            assert np.array_equal(ctx.download_aniso(), want[k]), k
        ctx.set_dynamic_mesh(None)
        run_pass(ctx)
        assert np.array_equal(ctx.download_aniso(), want["S"]), "detached"


def test_voxel_view_shows_the_merged_chain_and_the_static_pools(vct, oracle, world):
    """The radiance source at levels 0 and 1 against tests/voxel_view_ref.py on the merged chain, from a camera beside the
    object; the albedo and normal sources byte for byte what a context without a dynamic mesh shows."""
    from voxel_cone_tracing_amd import scene as sc
    w, h = 40, 24
    S, D = world["S", NONE][0], world["A", NONE][0]
    m = sc.invert_matrix(sc.camera_view_proj(sc.default_camera(position=(5.0, 4.0, -3.0), yaw=30.0, pitch=12.0), w, h))
    merged, static = oracle.build_mips(dc.merge(D, S)), oracle.build_mips(S)

    def view(ctx, source, level=0):
        ctx.render_voxels(m, source, level)
        return ctx.download_frame()
    with static_ctx(vct, world, width=w, height=h) as ctx, static_ctx(vct, world, width=w, height=h) as plain:
        ctx.set_dynamic_mesh(*world["A"])
        run_pass(ctx)
        run_pass(plain)
        for level in (0, 1):
            ref = lambda chain: vv.half_bits(vv.view(vv.level_of(chain, V, level), m, w, h, ctx.cfg.grid_world_size, ctx.cfg.max_alpha))
            want = ref(merged)
            assert (want != ref(static)).any(axis=2).sum() >= 50, level             # the object changes this camera's frame
            for source in (vct.VOXVIEW_RADIANCE, vct.VOXVIEW_CURRENT):
                got = view(ctx, source, level)
                assert int((got != want).any(axis=2).sum()) == 0, (source, level)
        alb, nrm = plain.voxel_attributes()
        assert np.array_equal(alb, world["S", NONE][1]) and np.array_equal(nrm, world["S", NONE][2])
        for source, vol in ((vct.VOXVIEW_ALBEDO, alb), (vct.VOXVIEW_NORMAL, nrm)):
            got = view(ctx, source)
            assert (got[..., :3] != 0).any(axis=2).sum() >= 50
            assert np.array_equal(got, view(plain, source)), source
            assert np.array_equal(got, vv.half_bits(vv.view(vol, m, w, h, ctx.cfg.grid_world_size, ctx.cfg.max_alpha))), source


def test_a_pass_over_an_uploaded_volume(vct, oracle, world):
    """vct_upload_volume_rgba8 + vct_build_mips is the upload's chain, mesh attached or not; the pass behind it resolves
    densely (every brick) and merges; the pass after that is sparse again."""
    S, D = world["S", NONE][0], world["A", NONE][0]
    r = np.random.default_rng(8)
    vol = r.integers(0, 256, (V, V, V, 4), dtype=np.uint8)
    vol[r.uniform(size=(V, V, V)) >= 0.2] = 0
    d, s = D[..., 3] > 0, S[..., 3] > 0
    assert (vol.any(-1) & ~d & ~s).sum() >= 10000 and (vol.any(-1) & d).sum() >= 50        # residue would show, beside and under the object
    with static_ctx(vct, world) as ctx:
        for attached in (False, True):
            if attached:
                ctx.set_dynamic_mesh(*world["A"])
            ctx.upload_volume(vol)
            ctx.build_mips()
            assert_chain(oracle, ctx, vol, f"the upload, attached={attached}")
            for what in ("dense", "sparse"):
                run_pass(ctx)
                assert_chain(oracle, ctx, dc.merge(D, S) if attached else S, f"{what} pass behind the upload, attached={attached}")
            if attached:
                assert_layer(ctx, world["A", NONE], "behind the upload")
        # the upload between a resolved pass and the next: the bricks of that pass's layer are the upload's, then clean
        ctx.update_dynamic_positions(world["B"][0])
        ctx.upload_volume(vol)
        ctx.build_mips()
        assert_chain(oracle, ctx, vol, "the upload over a resolved layer")
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(world["B", NONE][0], S), "B behind the upload")


def test_emission_and_lights_together(vct, oracle, world):
    """level0 = D.a > 0 ? lit(D, Da, Dn) : lit(S', Sa, Sn), S' the static level 0 with its emission added."""
    pos, mat, alb = world["static"]
    (S, Sa, Sn), (D, Da, Dn) = world["S", NONE], world["A", NONE]
    table = emission_ref.EMISSION.copy()
    table[mat[3]] = (0.3, 0.1, 0.6)                                  # the wall the object crosses glows too
    S1, L, _ = emission_ref.level0(oracle, oracle.default_params(V, G=G), pos, mat, alb, table)
    assert np.array_equal(L, S)
    lights = lr.many_lights(8)
    lit_s, lit_d = lr.level0(S1, Sa, Sn, lights, G), lr.level0(D, Da, Dn, lights, G)
    glows, lit, d = (S1 != S).any(-1), (lit_s != S1).any(-1), D[..., 3] > 0
    inside = np.repeat(np.repeat(np.repeat(dc.bricks(d), 8, 0), 8, 1), 8, 2)
    assert (glows & lit & d).sum() >= 10 and (glows & lit & ~d & inside).sum() >= 10      # glowing and lit: under the object, and beside it
    assert (lit_d != D).any(-1).sum() >= 50
    want = np.where(d[..., None], lit_d, lit_s)
    with static_ctx(vct, world) as ctx:
        ctx.upload_emission(table)
        ctx.set_lights(lights)
        ctx.set_dynamic_mesh(*world["A"])
        for rnd in range(2):
            run_pass(ctx)
            assert_chain(oracle, ctx, want, f"emission and 8 lights, pass {rnd}")
            assert_layer(ctx, (D, Da, Dn), "the layer is the unlit one")
        ctx.set_dynamic_mesh(None)
        run_pass(ctx)
        assert_chain(oracle, ctx, lit_s, "detached: the static chain with emission and lights")


def test_gi_pass_on_a_rank_context_carries_the_dynamic_mesh(vct, world):
    """vct_gi_pass after vct_comm_init(…, 0, 1) with the object at A, then B: the gathered frame is the single-GPU pass's
    with the same mesh, and not the frame without it."""
    from voxel_cone_tracing_amd import scene as sc
    import geomcases
    pos, mat, alb = world["static"]
    frames = geomcases.Case.frames(type("M", (), dict(pos=pos))())
    spec = np.tile(np.array([0.25, 0.5, 0.125], np.float32), (alb.shape[0], 1))
    cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
    light = (0.0, 1.0, 0.25)
    w, h = 64, 40
    vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(light)

    def ctx_with(mesh):
        c = vct.Context(dc.config(vct, width=w, height=h, shadow_map_size=256, debug_outputs=0))
        c.upload_triangles(pos, mat, alb)
        c.upload_mesh_attributes(*frames, spec)
        c.set_camera_position(tuple(float(x) for x in cam.position))
        c.set_light_direction(light)
        if mesh:
            c.set_dynamic_mesh(*world["A"])
        return c
    with ctx_with(True) as single, ctx_with(True) as rank, ctx_with(False) as bare:
        bare.gi_pass(lvp, vp)
        without = bare.download_frame()
        rank.comm_init(vct.comm_unique_id(), 0, 1)
        seen = []
        for k in "AB":
            for c in (single, rank):
                c.update_dynamic_positions(world[k][0])
                c.gi_pass(lvp, vp)
            rank.comm_sync()
            want, got = single.download_frame(), rank.comm_download_frame()
            print(f"at {k}: {int((want != without).any(axis=2).sum())} of {w * h} pixels differ from the frame without the object")
            assert not np.array_equal(want, without), k                     # the object shows in the single-GPU frame ...
            assert np.array_equal(got, want), k                             # ... and the rank's frame is that frame
            assert np.array_equal(rank.download_chain(), single.download_chain()), k
            for a, b in zip(rank.download_dynamic_voxels(), single.download_dynamic_voxels()):
                assert a.any() and np.array_equal(a, b), k
            seen.append(want)
        assert not np.array_equal(seen[0], seen[1])
        rank.comm_destroy()


@pytest.mark.parametrize("change", ["replace", "detach"])
def test_layer_replaced_or_detached_between_voxelize_and_inject(vct, oracle, world, change):
    """vct_set_dynamic_mesh between vct_voxelize and vct_inject_light: the fresh (or no) layer has no pass to resolve, so
    that pass is the static chain -- the bricks the previous pass's layer occupied clean, mips included -- and the next
    full pass is merge(D_new, S), or S."""
    S, DA, DB = world["S", NONE][0], world["A", NONE], world["B", NONE]
    assert not (dc.bricks(DA[0][..., 3] > 0) & dc.bricks(DB[0][..., 3] > 0)).any()
    with static_ctx(vct, world) as ctx:
        ctx.set_dynamic_mesh(*world["A"])
        run_pass(ctx)
        assert_chain(oracle, ctx, dc.merge(DA[0], S), "A resolved")
        ctx.voxelize()                                                  # A's fragments are in the old layer's accumulators
        if change == "replace":
            ctx.set_dynamic_mesh(*world["B"])
            info = ctx.dynamic_info()
            assert (info["ntri"], info["max_bricks"]) == (dc.NTRI, max(64, 2 * nbricks(DB[0]))), info
            assert [info[k] for k in INFO_KEYS[3:]] == [0] * 5, info    # no resolved pass
        else:
            ctx.set_dynamic_mesh(None)
            assert ctx.dynamic_info() == dict.fromkeys(INFO_KEYS, 0)
        ctx.inject_light(); ctx.build_mips()
        assert_chain(oracle, ctx, S, f"{change}: the pass in between is the static chain")
        if change == "replace":
            assert_layer(ctx, tuple(np.zeros_like(x) for x in DB), "the fresh layer has resolved nothing")
            assert [ctx.dynamic_info()[k] for k in INFO_KEYS[3:]] == [0] * 5
            for rnd in range(2):
                run_pass(ctx)
                assert_layer(ctx, DB, f"B, pass {rnd}")
                assert_chain(oracle, ctx, dc.merge(DB[0], S), f"B, pass {rnd}")
                resolved(ctx, DB[0], "B")
        else:
            run_pass(ctx)
            assert_chain(oracle, ctx, S, "detached, the next pass")
            ctx.set_dynamic_mesh(*world["A"])
            run_pass(ctx)
            assert_chain(oracle, ctx, dc.merge(DA[0], S), "attached again")


def test_dynamic_times_need_timing_on(vct, oracle, world):
    S, D = world["S", NONE][0], world["A", NONE][0]
    with static_ctx(vct, world) as ctx:
        ctx.set_dynamic_mesh(*world["A"])
        refused(vct, ctx.last_dynamic_ms)                               # before both ran
        run_pass(ctx)
        t = ctx.last_dynamic_ms()
        assert t[0] > 0.0 and t[1] > 0.0
        ctx.set_trace_timing(False)
        run_pass(ctx)
        refused(vct, ctx.last_dynamic_ms)
        assert b"timing off" in vct.lib().vct_last_error(ctx._h)
        assert_chain(oracle, ctx, dc.merge(D, S), "timing off")
        ctx.set_trace_timing(True)
        refused(vct, ctx.last_dynamic_ms)                               # the last kernels are still the untimed ones
        run_pass(ctx)
        t = ctx.last_dynamic_ms()
        assert t[0] > 0.0 and t[1] > 0.0
        assert_chain(oracle, ctx, dc.merge(D, S), "timing on again")
