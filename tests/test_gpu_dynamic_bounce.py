"""GPU: the second bounce over the dynamic mesh (include/vct.h "dynamic mesh", vct_set_dynamic_bounce) -- vct_bounce with
a mesh attached and the switch on, bit-equal to the CPU oracle's vcto_bounce over the merged chain with the owner's
attributes, where(D.a > 0, Da, Sa) and where(D.a > 0, Dn, Sn) (tests/dynbouncecases.py), mips behind it, and the same
step count.  Scenes: tests/dyncases.py; their premises are held without a GPU by tests/test_dynamic_bounce_cases.py.

All contexts: voxel_dim 64 (the dense scene: 16), an 8 x 8 frame, voxel attributes.  Every chain comparison covers all
levels; every bounce compares last_step_count() with the oracle's steps."""
import os
import re
import subprocess

import numpy as np
import pytest

import dynbouncecases as db
import dyncases as dc
import emission_ref
import lights_ref as lr
import point_query_ref as pq
import synth
import vctpkg
from test_gpu_dynamic import ISSUE, NONE, RAISED, nbricks, run_pass, shadow_maps, static_ctx

pytestmark = pytest.mark.gpu
V, G, MS = dc.V, dc.G, dc.MS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


@pytest.fixture(scope="module")
def world(oracle):
    """The static scene, the object at A and B and their layers; expected bounces are computed once each (`want`)."""
    w = dict(static=dc.static_scene(), A=dc.dynamic_mesh(dc.A), B=dc.dynamic_mesh(dc.B), maps=shadow_maps(), cache={})
    for sh, (depth, vp) in w["maps"].items():
        w["S", sh] = dc.layer(oracle, *w["static"], depth=depth, vp=vp)
        for k in ("A",) if sh != NONE else "AB":
            w[k, sh] = dc.layer(oracle, *w[k], depth=depth, vp=vp)
    return w


def want(oracle, world, k, sh=NONE):
    """(level 0 after the bounce, steps) with the object at k ("S": no object) under shadow map sh."""
    c = world["cache"]
    if (k, sh) not in c:
        c[k, sh] = db.detached(oracle, world["S", sh]) if k == "S" else db.expected(oracle, world[k, sh], world["S", sh])
    return c[k, sh]


def assert_bounced(oracle, ctx, l1, steps, what):
    got, mips = ctx.download_chain(), oracle.build_mips(l1)
    n = l1.shape[0] ** 3
    bad = np.argwhere((got[:n] != mips[:n]).any(-1).reshape(l1.shape[:3]))
    print(what, "steps", ctx.last_step_count(), "want", steps, "level-0 voxels off", bad.shape[0])
    assert bad.shape[0] == 0, (what, "level 0", bad.shape[0], bad[:4].tolist())
    assert np.array_equal(got, mips), (what, "mips")
    assert ctx.last_step_count() == steps, (what, ctx.last_step_count(), steps)


def assert_merged(oracle, ctx, D, S, what):
    assert np.array_equal(ctx.download_chain(), oracle.build_mips(dc.merge(D, S))), what


def dyn_ctx(vct, world, k="A", shadow=NONE, **kw):
    ctx = static_ctx(vct, world, shadow, **kw)
    ctx.set_dynamic_bounce(True)
    if k:
        ctx.set_dynamic_mesh(*world[k])
    return ctx


def refused(vct, call, *a):
    with pytest.raises(vct.VctError) as e:
        call(*a)
    assert "(-1)" in str(e.value), str(e.value)               # VCT_ERR_INVALID
    return str(e.value)


# ---- 1. the three shadow maps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_shadow", [NONE, ISSUE, RAISED])
def test_bounce_over_the_merged_chain(vct, oracle, world, with_shadow):
    S3, D3 = world["S", with_shadow], world["A", with_shadow]
    l1, steps = want(oracle, world, "A", with_shadow)
    wrong, wrong_steps = db.static_attributes(oracle, D3, S3)
    d = D3[0][..., 3] > 0
    # the comparison can fail: the bounce changes voxels, and which attributes shade the layer's voxels shows
    # (the oracle: 3,319 / 2,860 / 3,310 voxels changed by the bounce, 540 / 383 / 538 by whose attributes shade the layer)
    assert db.differing(l1, dc.merge(D3[0], S3[0])).sum() >= 2000 and steps > want(oracle, world, "S", with_shadow)[1] + 10_000
    assert (db.differing(l1, wrong) & d).sum() >= 300 and not (db.differing(l1, wrong) & ~d).any() and steps != wrong_steps
    with dyn_ctx(vct, world, "A", with_shadow) as ctx:
        run_pass(ctx)
        ctx.bounce()
        assert_bounced(oracle, ctx, l1, steps, f"A, shadow={with_shadow}")


# ---- 2. two bounces back to back ------------------------------------------------------------------------------------
def test_two_bounces_back_to_back(vct, oracle, world):
    l1, steps = want(oracle, world, "A")
    with dyn_ctx(vct, world) as ctx:
        run_pass(ctx)
        for rnd in range(2):
            ctx.bounce()
            assert_bounced(oracle, ctx, l1, steps, f"bounce {rnd}")


# ---- 3. A -> B -> A, detach, attach ---------------------------------------------------------------------------------
def test_a_bounce_after_every_pass_of_a_moving_object(vct, oracle, world):
    S = world["S", NONE][0]
    own = {k: dc.non_degeneracy(world[k, NONE][0], S)["dynamic_only_bricks"] for k in "AB"}
    assert own["A"] >= 3 and own["B"] >= 6                      # bricks the object leaves behind when it moves on
    assert db.differing(want(oracle, world, "A")[0], want(oracle, world, "B")[0]).sum() >= 2000
    with dyn_ctx(vct, world) as ctx:
        for k in "ABA":
            ctx.update_dynamic_positions(world[k][0])
            run_pass(ctx)
            assert_merged(oracle, ctx, world[k, NONE][0], S, f"bounce 0 at {k}")      # a new inject returns to bounce 0
            ctx.bounce()
            assert_bounced(oracle, ctx, *want(oracle, world, k), f"at {k}")
        ctx.set_dynamic_mesh(None)
        run_pass(ctx)
        ctx.bounce()
        l1, steps = want(oracle, world, "S")
        assert steps == 84_359
        assert_bounced(oracle, ctx, l1, steps, "detached")
        ctx.set_dynamic_mesh(*world["B"])
        run_pass(ctx)
        ctx.bounce()
        assert_bounced(oracle, ctx, *want(oracle, world, "B"), "attached again, at B")


# ---- 4. the switch as state -----------------------------------------------------------------------------------------
def test_the_switch_is_context_state(vct, oracle, world):
    S = world["S", NONE][0]
    with static_ctx(vct, world) as ctx:
        assert ctx.dynamic_bounce is False
        ctx.set_dynamic_bounce(True)
        assert ctx.dynamic_bounce is True
        run_pass(ctx)                                          # on with nothing attached: the static bounce
        ctx.bounce()
        assert_bounced(oracle, ctx, *want(oracle, world, "S"), "on, nothing attached")
        ctx.set_dynamic_mesh(*world["A"]); assert ctx.dynamic_bounce is True
        ctx.set_dynamic_mesh(*world["B"]); assert ctx.dynamic_bounce is True
        ctx.set_dynamic_mesh(None); assert ctx.dynamic_bounce is True
        ctx.upload_triangles(*world["static"]); assert ctx.dynamic_bounce is True
        for bad in (-1, 2):
            refused(vct, ctx.set_dynamic_bounce, bad)
            assert ctx.dynamic_bounce is True
        ctx.set_dynamic_mesh(*world["A"])
        run_pass(ctx)
        ctx.bounce()
        assert_bounced(oracle, ctx, *want(oracle, world, "A"), "attached, on")
        run_pass(ctx)
        chain = ctx.download_chain()
        ctx.set_dynamic_bounce(False)                          # on -> off: the refusal is back, the chain untouched
        assert ctx.dynamic_bounce is False
        assert "a dynamic mesh is attached" in refused(vct, ctx.bounce)
        assert np.array_equal(ctx.download_chain(), chain)
        assert_merged(oracle, ctx, world["A", NONE][0], S, "after the refusal")
        ctx.set_dynamic_bounce(True)
        ctx.bounce()
        assert_bounced(oracle, ctx, *want(oracle, world, "A"), "on again")


# ---- 5. capacity and stale layers -----------------------------------------------------------------------------------
def test_a_pass_without_the_layer_bounces_as_the_static_chain(vct, oracle, world):
    S = world["S", NONE][0]
    need = nbricks(world["A", NONE][0])
    static_l1, static_steps = want(oracle, world, "S")
    l1, steps = want(oracle, world, "A")
    assert steps != static_steps and db.differing(l1, static_l1).sum() >= 1000
    with dyn_ctx(vct, world, None) as ctx:
        ctx.set_dynamic_mesh(*world["A"], max_bricks=need - 1)         # one short: the whole layer is left out
        run_pass(ctx)
        assert ctx.dynamic_info()["left_out"] == 1
        ctx.bounce()
        assert_bounced(oracle, ctx, static_l1, static_steps, "left out for capacity")
        ctx.set_dynamic_mesh(*world["A"], max_bricks=need)             # exactly enough
        run_pass(ctx)
        assert ctx.dynamic_info()["left_out"] == 0
        ctx.bounce()
        assert_bounced(oracle, ctx, l1, steps, "exact capacity")
        ctx.voxelize()                                                 # replaced between voxelize and inject: no pass to resolve
        ctx.set_dynamic_mesh(*world["B"])
        ctx.inject_light(); ctx.build_mips()
        assert_merged(oracle, ctx, np.zeros_like(S), S, "the fresh layer has no pass")
        ctx.bounce()
        assert_bounced(oracle, ctx, static_l1, static_steps, "replaced between voxelize and inject")
        run_pass(ctx)                                                  # and the next full pass merges and bounces it
        ctx.bounce()
        assert_bounced(oracle, ctx, *want(oracle, world, "B"), "the pass after")


# ---- 6. the big object ----------------------------------------------------------------------------------------------
def test_the_big_object_overflows_the_list(vct, oracle, world):
    """Every brick of the grid is dynamic, 229 of them without a static slot, brick 0 among the layer's, one dynamic voxel
    with a zero normal, and more occupied voxels than the list holds: k_bounce_bricks<.., DYN> at 64^3."""
    S3 = world["S", NONE]
    big = dc.big_triangles()
    D3 = dc.layer(oracle, *big)
    d = D3[0][..., 3] > 0
    n = dc.non_degeneracy(D3[0], S3[0])
    assert n["dynamic_bricks"] == 512 and n["dynamic_only_bricks"] >= 200 and dc.bricks(d)[0, 0, 0]
    assert (dc.merge(D3[0], S3[0])[..., 3] > 0).sum() > V ** 3 // 8
    assert (d & db.zero_normal(D3[2])).sum() >= 1
    l1, steps = db.expected(oracle, D3, S3)
    assert steps > db.static_attributes(oracle, D3, S3)[1] + 100_000
    with dyn_ctx(vct, world, None) as ctx:
        ctx.set_dynamic_mesh(*big)
        run_pass(ctx)
        assert ctx.dynamic_info()["bricks_used"] == 512
        for rnd in range(2):
            ctx.bounce()
            assert_bounced(oracle, ctx, l1, steps, f"big triangles, bounce {rnd}")
        ctx.set_dynamic_mesh(*world["A"])                      # the small object behind it: 500 bricks of the layer come out clean
        run_pass(ctx)
        ctx.bounce()
        assert_bounced(oracle, ctx, *want(oracle, world, "A"), "A behind the big object")


# ---- 7. dense 16^3, both WRAP forms ---------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [1, 0])
def test_dense_grid_overflow_in_both_wrap_forms(vct, oracle, wrap):
    v = 16
    static, mesh = db.dense16_static(), dc.dynamic_mesh(dc.A)
    p = oracle.default_params(v, G=G, wrap_repeat=wrap)
    S3, D3 = dc.layer(oracle, *static, V=v), dc.layer(oracle, *mesh, V=v)
    d = D3[0][..., 3] > 0
    assert (dc.merge(D3[0], S3[0])[..., 3] > 0).sum() > v ** 3 // 8 and d.sum() >= 50 and dc.bricks(d).sum() == 8
    l1, steps = db.expected(oracle, D3, S3, p=p)
    wrong, wrong_steps = db.static_attributes(oracle, D3, S3, p=p)
    assert steps != wrong_steps and db.differing(l1, wrong).sum() >= 10
    other, _ = db.expected(oracle, D3, S3, p=oracle.default_params(v, G=G, wrap_repeat=1 - wrap))
    assert db.differing(l1, other).sum() >= 1                      # clamp and REPEAT differ here
    with vct.Context(dc.config(vct, v, wrap_repeat=wrap)) as ctx:
        ctx.upload_triangles(*static)
        ctx.set_dynamic_bounce(True)
        ctx.set_dynamic_mesh(*mesh)
        run_pass(ctx)
        for rnd in range(2):
            ctx.bounce()
            assert_bounced(oracle, ctx, l1, steps, f"dense 16^3, wrap_repeat={wrap}, bounce {rnd}")


# ---- 8. local lights and static emission together -------------------------------------------------------------------
def test_lights_and_emission_under_the_bounce(vct, oracle, world):
    """level0, the bounce's src, is the lit merged texel; ownership is the layer's own radiance, stored before lights."""
    pos, mat, alb = world["static"]
    (S, Sa, Sn), (D, Da, Dn) = world["S", NONE], world["A", NONE]
    table = emission_ref.EMISSION.copy()
    table[mat[3]] = (0.3, 0.1, 0.6)                                  # the wall the object crosses glows too
    S1, L, _ = emission_ref.level0(oracle, oracle.default_params(V, G=G), pos, mat, alb, table)
    assert np.array_equal(L, S)
    lights = lr.many_lights(8)
    lit_s, lit_d = lr.level0(S1, Sa, Sn, lights, G), lr.level0(D, Da, Dn, lights, G)
    d = D[..., 3] > 0
    l0 = np.where(d[..., None], lit_d, lit_s)
    assert db.differing(l0, dc.merge(D, S)).sum() >= 100 and (db.differing(lit_d, D) & d).sum() >= 50
    l1, steps = db.expected(oracle, (D, Da, Dn), (S, Sa, Sn), l0=l0)
    assert db.differing(l1, want(oracle, world, "A")[0]).sum() >= 100
    with dyn_ctx(vct, world, None) as ctx:
        ctx.upload_emission(table)
        ctx.set_lights(lights)
        ctx.set_dynamic_mesh(*world["A"])
        run_pass(ctx)
        assert np.array_equal(ctx.download_chain(), oracle.build_mips(l0))
        ctx.bounce()
        assert_bounced(oracle, ctx, l1, steps, "8 lights and emission")


# ---- 9. readers after the bounce ------------------------------------------------------------------------------------
def test_point_queries_and_the_trace_read_the_bounce_chain(vct, oracle, world):
    l1, steps = want(oracle, world, "A")
    chain, chain0 = oracle.build_mips(l1), oracle.build_mips(dc.merge(world["A", NONE][0], world["S", NONE][0]))
    planes = synth.random_gbuffer(64, seed=42, discard_frac=0.05)
    r = np.random.default_rng(4)
    P = np.asarray(dc.A) * MS + r.uniform(-20.0, 20.0, (64, 3))
    nn = r.normal(size=(64, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    h = np.where(np.abs(nn[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = np.cross(h, nn)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    pts = np.ascontiguousarray(np.concatenate([P, nn * MS, t * MS, np.cross(nn, t) * MS], 1), np.float32)
    p = oracle.default_params(V, G=G)
    ref, ref0 = pq.gather(oracle, p, chain, pts), pq.gather(oracle, p, chain0, pts)
    assert (pq.u32(ref["gather"]) != pq.u32(ref0["gather"])).any(-1).sum() >= 16      # the bounce shows in the gathers
    frame_ref = oracle.trace(p, chain, planes, nthreads=4)["rgba32f"]
    assert synth.rel_l2(oracle.trace(p, chain0, planes, nthreads=4)["rgba32f"], frame_ref) > 1e-3      # and in the frame
    with dyn_ctx(vct, world) as ctx:
        run_pass(ctx)
        ctx.bounce()
        assert_bounced(oracle, ctx, l1, steps, "before the readers")
        pq.assert_floats_match(ctx.gather_points(pts), ref["gather"], "gather around A on the bounce chain")
        err = synth.rel_l2(vct.half_to_float(ctx.trace(planes).reshape(-1, 4)), frame_ref)
        print("traced frame rel_l2", err)
        assert err <= 1e-3, err


# ---- 10. two frame slots --------------------------------------------------------------------------------------------
def test_bounce_on_one_slot_while_the_other_traces(vct, oracle, world):
    planes = synth.random_gbuffer(64, seed=42, discard_frac=0.05)
    order = "ABBA"

    def play(two):
        out = []
        with dyn_ctx(vct, world, "A", debug_outputs=0) as ctx:
            if two:
                ctx.set_frames_in_flight(2)
            run_pass(ctx)
            if two:
                ctx.trace(planes)                              # slot 0's G-buffer: these planes
            for i, k in enumerate(order):
                if two:
                    ctx.select_frame_slot(0)
                    ctx.trace_resident()                       # queued, not waited for: slot 0 has a trace in flight ...
                    ctx.select_frame_slot(1)                   # ... while slot 1 updates, passes, bounces and traces
                ctx.update_dynamic_positions(world[k][0])
                run_pass(ctx)
                ctx.bounce()
                steps = ctx.last_step_count()
                frame = ctx.trace(planes)
                out.append((frame, ctx.download_chain(), steps))
        return out
    got, ref = play(True), play(False)
    for i, k in enumerate(order):
        l1, steps = want(oracle, world, k)
        assert np.array_equal(got[i][0], ref[i][0]), (i, k, "frame")
        assert np.array_equal(got[i][1], ref[i][1]), (i, k, "chain")
        assert got[i][2] == ref[i][2] == steps, (i, k, got[i][2], ref[i][2], steps)
        assert np.array_equal(ref[i][1], oracle.build_mips(l1)), (i, k)
    assert not np.array_equal(ref[0][0], ref[1][0])


# ---- 11. facade and demo --------------------------------------------------------------------------------------------
def box_obj(path, half=150.0):
    v = [(x, y, z) for z in (-half, half) for y in (-half, half) for x in (-half, half)]
    quads = [(1, 3, 4, 2), (5, 6, 8, 7), (1, 2, 6, 5), (3, 7, 8, 4), (1, 5, 7, 3), (2, 4, 8, 6)]      # outward, CCW
    path.write_text("".join(f"v {x} {y} {z}\n" for x, y, z in v) +
                    "".join(f"f {a} {b} {c}\nf {a} {c} {d}\n" for a, b, c, d in quads))
    return str(path)


def demo(*args):
    exe = os.path.join(ROOT, "voxel-cone-tracing_amd", "vct_demo")
    assert os.path.exists(exe), "build it with `make demo`"
    out = subprocess.run([exe, "--scene", "procedural:cornell", "--voxels", "64", "--size", "64x64", "--shadow", "256", *args],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [ln for ln in out.stdout.split("\n") if ln.startswith("frames=")][-1]
    return dict(kv.split("=") for kv in line.split()), out.stdout


def test_the_demo_and_the_facade_bounce_over_the_object(vct, tmp_path):
    """vct_demo --dynamic-obj FILE --bounces 2 --dynamic-bounce: Voxel_Cone_Tracing with Bounces = 2 and DynamicBounce.  Its
    frame differs from --bounces 1 and from the static --bounces 2, and equals the frame of the same stages driven through
    the binding (the route of test_gpu_parity.test_facade_demo_matches_binding)."""
    from voxel_cone_tracing_amd import scene as sc
    import raster_oracle
    obj = box_obj(tmp_path / "box.obj")
    both, text = demo("--frames", "1", "--dynamic-obj", obj, "--bounces", "2", "--dynamic-bounce")
    assert re.search(r"dynamic mesh: triangles=12 bricks=(\d+) of (\d+) fragments=(\d+) skipped=0 left_out=0", text), text[-1000:]
    one, _ = demo("--frames", "1", "--dynamic-obj", obj)
    static2, _ = demo("--frames", "1", "--bounces", "2")
    assert len({both["fnv1a"], one["fnv1a"], static2["fnv1a"]}) == 3, (both, one, static2)
    V2, w, h, S = 64, 64, 64, 256
    scene, mover = sc.Scene(sc.CORNELL), sc.Scene(obj)
    light = (0.0, 1.0, 0.25)
    depth, light_vp = raster_oracle.shadow_map(sc, scene, light, S)
    planes = raster_oracle.gbuffer(sc, scene, sc.default_camera(position=(0.0, 0.0, 58.0)), w, h, depth, light_vp)
    with vct.Context(vct.default_config(voxel_dim=V2, width=w, height=h, shadow_map_size=S, voxel_attributes=1)) as ctx:
        ctx.set_camera_position((0.0, 0.0, 58.0))
        ctx.set_light_direction(light)
        ctx.upload_triangles(scene.pos, scene.material, scene.albedo)
        ctx.upload_shadow_map(depth, light_vp)
        ctx.set_dynamic_bounce(True)
        ctx.set_dynamic_mesh(mover.pos, mover.material, mover.albedo)
        run_pass(ctx)
        ctx.bounce()
        frame = ctx.trace(planes)
        assert int(both["cone_steps"]) == ctx.last_step_count()
    hsh = 1469598103934665603
    for x in frame.reshape(-1).tolist():
        hsh = ((hsh ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert both["fnv1a"] == f"{hsh:016x}"
