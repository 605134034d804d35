"""GPU: point queries (include/vct.h "point queries": vct_gather_points, vct_cone_points) against the CPU oracle through
tests/point_query_ref.py, on the inputs of tests/pqcases.py (whose classes tests/test_point_query_cases.py proves), and
against the screen trace's own debug outputs.

Bar, everywhere: every float of every point bit-identical to the reference, except that NaN equals NaN; every step count
equal; the executed-step total equal to the reference's sum.  No point is left out.  V = 32 throughout; n <= 514, except
for the 2640 pixels of the 60 x 44 frame that is held against the screen trace."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import components_ref as cr
import pqcases as pc
import point_query_ref as pq
import synth
import test_gpu_march_params as mp
import vctpkg

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEVICE = "host", "device"


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


@pytest.fixture(scope="module")
def chain(oracle):
    return oracle.build_mips(pc.level0())


@pytest.fixture(scope="module", params=[1, 0], ids=["repeat", "clamp"])
def wctx(request, vct, chain):
    """One context per wrap mode with the cases' chain uploaded."""
    with vct.Context(vct.default_config(wrap_repeat=request.param, **pc.config())) as ctx:
        ctx.upload_chain(chain)
        yield ctx


_refs = {}


def reference(oracle, chain, name, wrap):
    key = (name, wrap)
    if key not in _refs:
        p = oracle.default_params(pc.V, G=pc.G, max_distance=pc.MAX_DISTANCE, wrap_repeat=wrap)
        _refs[key] = pq.gather(oracle, p, chain, pc.get(name))
    return _refs[key]


def gather_on(ctx, pts, where, sort=False):
    """(gather, cones, steps) of a gather query with host or device (torch) memory."""
    pts = np.ascontiguousarray(pts, f32)
    if where == HOST:
        return ctx.gather_points(pts, want_cones=True, want_steps=True, sort=sort)
    import torch
    n = pts.shape[0]
    d_pts = torch.from_numpy(pts).cuda()
    d_out = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    d_cones = torch.full((n, 6, 4), -7.0, dtype=torch.float32, device="cuda")
    d_steps = torch.full((n, 6), 201, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.gather_points(d_pts.data_ptr(), n=n, out_device_ptr=d_out.data_ptr(), cones_device_ptr=d_cones.data_ptr(),
                      steps_device_ptr=d_steps.data_ptr(), sort=sort)
    ctx.synchronize()
    return d_out.cpu().numpy(), d_cones.cpu().numpy(), d_steps.cpu().numpy()


def cones_on(ctx, pts, aperture, where, sort=False):
    pts = np.ascontiguousarray(pts, f32)
    if where == HOST:
        return ctx.cone_points(pts, aperture, want_steps=True, sort=sort)
    import torch
    n = pts.shape[0]
    d_pts = torch.from_numpy(pts).cuda()
    d_out = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    d_steps = torch.full((n,), 201, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.cone_points(d_pts.data_ptr(), aperture, n=n, out_device_ptr=d_out.data_ptr(), steps_device_ptr=d_steps.data_ptr(), sort=sort)
    ctx.synchronize()
    return d_out.cpu().numpy(), d_steps.cpu().numpy()


def check_gather(ctx, got, ref, idx, what, sorted_=False):
    g, c, s = got
    pq.assert_floats_match(c, ref["cones"][idx], f"{what}: raw cones")
    assert np.array_equal(s, ref["steps"][idx]), f"{what}: per-cone step counts"
    pq.assert_floats_match(g, ref["gather"][idx], f"{what}: gather")
    n, steps, kind, was_sorted = ctx.last_point_query()
    assert (n, kind, was_sorted) == (len(idx), 0, int(sorted_)), what
    assert steps == int(ref["steps"][idx].astype(np.int64).sum()), f"{what}: executed steps"


# ---- 1. bit equality with the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [HOST, DEVICE])
@pytest.mark.parametrize("name", pc.CASES)
def test_gather_equals_the_oracle(vct, oracle, chain, wctx, name, where):
    pts = pc.get(name)
    ref = reference(oracle, chain, name, wctx.cfg.wrap_repeat)
    for n in pc.SIZES + (pts.shape[0],):
        idx = np.arange(n) % pts.shape[0]
        check_gather(wctx, gather_on(wctx, pts[idx], where), ref, idx, f"{name} n={n} {where}")
    # without the optional outputs: the other instantiation, the same gather
    g = wctx.gather_points(pts)
    pq.assert_floats_match(g, ref["gather"], f"{name}: gather alone")
    assert wctx.last_point_query()[1] == ref["total_steps"]
    assert wctx.last_point_query_ms() > 0.0


# ---- 2. single cones --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [HOST, DEVICE])
@pytest.mark.parametrize("aperture", [0, 1])
def test_single_cones_equal_the_oracle(vct, oracle, chain, wctx, aperture, where):
    wrap = wctx.cfg.wrap_repeat
    p = oracle.default_params(pc.V, G=pc.G, max_distance=pc.MAX_DISTANCE, wrap_repeat=wrap)
    tan = float(pc.TAN_SPECULAR if aperture else pc.TAN_DIFFUSE)
    pts = pc.edge_cones()
    assert pts.shape[0] <= 514
    ref = pq.cones(oracle, p, chain, pts, tan)
    for n in (pts.shape[0], 65):
        out, steps = cones_on(wctx, pts[:n], aperture, where)
        pq.assert_floats_match(out, ref["cone"][:n], f"cones aperture {aperture} n={n}")
        assert np.array_equal(steps.astype(np.int64), ref["steps"][:n])
        q = wctx.last_point_query()
        assert q == (n, int(ref["steps"][:n].sum()), 1, 0)
    out = wctx.cone_points(pts, aperture)              # no step counts wanted
    pq.assert_floats_match(out, ref["cone"], "cones alone")


@pytest.mark.parametrize("name", ["patch", "scatter", "edge"])
def test_cones_along_the_gathers_directions_reproduce_its_cones(vct, oracle, chain, wctx, name):
    pts = pc.get(name)[:130]
    _, cones, steps = gather_on(wctx, pts, HOST)
    dirs = pq.cone_dirs(oracle, pts)
    for i in range(6):
        out, st = wctx.cone_points(pq.cone_points_of(pts, dirs[:, i]), 0, want_steps=True)
        pq.assert_floats_match(out, cones[:, i], f"{name}: cone {i}")
        assert np.array_equal(st, steps[:, i])


# ---- 3. both division forms, other march constants ------------------------------------------------------------------------
MARCH = {"verified_G": (dict(grid_world_size=mp.VERIFIED_G, max_distance=mp.VERIFIED_G / 2), mp.PRODUCT),
         "rejected_G": (dict(grid_world_size=mp.REJECTED_G, max_distance=mp.REJECTED_G / 2), mp.IEEE),
         "max_alpha": (dict(max_alpha=0.99), mp.IEEE),
         "max_distance": (dict(max_distance=41.5), None),
         "apertures": (dict(), None)}


@pytest.mark.parametrize("wrap", [1, 0])
@pytest.mark.parametrize("which", list(MARCH))
def test_division_forms_and_march_constants(vct, oracle, chain, which, wrap):
    consts, form = MARCH[which]
    cfg = dict(pc.config(wrap_repeat=wrap), **consts)
    G = cfg["grid_world_size"]
    pts = np.concatenate([pc.scatter()[:100], pc.patch()[:93]])
    pts[:, 0:3] *= f32(G / pc.G)
    with vct.Context(vct.default_config(**cfg)) as ctx:
        ctx.upload_chain(chain)
        if which == "apertures":
            ctx.set_cone_apertures(0.4, 0.12)
        p = mp.params(oracle, ctx)
        ref = pq.gather(oracle, p, chain, pts)
        got = ctx.gather_points(pts, want_cones=True, want_steps=True)
        if form is None:
            form = mp.expected_form(ctx)
        assert mp.form_of(ctx) == form, which
        check_gather(ctx, got, ref, np.arange(pts.shape[0]), which)
        cpts = pq.cone_points_of(pts, pq.cone_dirs(oracle, pts)[:, 2])
        for aperture, tan in ((0, p.tan_diffuse), (1, p.tan_specular)):
            want = pq.cones(oracle, p, chain, cpts, tan)
            out, st = ctx.cone_points(cpts, aperture, want_steps=True)
            pq.assert_floats_match(out, want["cone"], f"{which}: aperture {aperture}")
            assert np.array_equal(st.astype(np.int64), want["steps"])
        assert mp.form_of(ctx) == form


@pytest.mark.parametrize("wrap", [1, 0])
def test_gather_without_debug_outputs_under_the_ieee_divide(vct, oracle, chain, wrap):
    """k_query_march<WRAP, 0, GATHER, false>: the gather alone (no cones, no step counts asked for) with a grid size whose
    divisors the device rejects.  No debug outputs exist in this instantiation, so the bar is on what it writes: every
    gather float bit-equal to the oracle's and the executed-step total equal to the sum of the oracle's per-cone counts.
    193 points: three full waves and a tail of one lane; a coherent patch (cooperative blocks) and a scatter (per-lane)."""
    consts, form = MARCH["rejected_G"]
    cfg = dict(pc.config(wrap_repeat=wrap), **consts)
    pts = np.concatenate([pc.scatter()[:100], pc.patch()[:93]])
    pts[:, 0:3] *= f32(cfg["grid_world_size"] / pc.G)
    with vct.Context(vct.default_config(**cfg)) as ctx:
        ctx.upload_chain(chain)
        ref = pq.gather(oracle, mp.params(oracle, ctx), chain, pts)
        got = ctx.gather_points(pts)
        assert mp.form_of(ctx) == form
        pq.assert_floats_match(got, ref["gather"], "gather without debug outputs")
        n, steps, kind, was_sorted = ctx.last_point_query()
        assert (n, kind, was_sorted) == (pts.shape[0], 0, 0)
        assert steps == int(ref["steps"].astype(np.int64).sum())


# ---- 4. GPU against GPU: the screen trace's own cones -----------------------------------------------------------------------
def specular_dirs(planes, cam):
    """csrc/vct_trace.hip specular_dir in fp32: normalize(reflect(-E, N)), E = normalize(cam - P), N = planes 12-14."""
    g = np.asarray(planes, f32)
    with np.errstate(all="ignore"):
        E = cr._normalize([f32(cam[a]) - g[a] for a in range(3)])
        R = cr._normalize(cr._reflect([E[a] * f32(-1.0) for a in range(3)], [g[12], g[13], g[14]]))
    return np.stack(R, axis=1).astype(f32)


def check_against_trace(ctx, planes, cam, what):
    """The frame's pixels as points in linear pixel order: cones 0-5 from a gather, cone 6 from a specular single cone."""
    cones, steps = ctx.cones(), ctx.steps()
    live = ~(planes[18] < f32(0.5))
    pts = np.ascontiguousarray(planes[0:12].T)
    g, c, s = ctx.gather_points(pts, want_cones=True, want_steps=True)
    pq.assert_floats_match(c[live], cones[live, :6], f"{what}: cones 0-5")
    assert np.array_equal(s[live], steps[live, :6]), what
    with np.errstate(all="ignore"):
        pq.assert_floats_match(g[live], cr.gather(cones[live, :6]), f"{what}: gather")
    spec = np.ascontiguousarray(np.concatenate([pts[:, 0:6], specular_dirs(planes, cam)], axis=1))
    out, st = ctx.cone_points(spec, 1, want_steps=True)
    pq.assert_floats_match(out[live], cones[live, 6], f"{what}: cone 6")
    assert np.array_equal(st[live], steps[live, 6]), what
    return g, c, s


def test_frame_pixels_as_points_equal_the_debug_outputs(vct, oracle, chain):
    w, h = mp.W, mp.H
    planes = mp.gbuffer(pc.G, w, h)
    cam = (3.0, 4.0, -2.0)
    with vct.Context(vct.default_config(voxel_dim=pc.V, width=w, height=h, debug_outputs=1)) as ctx:
        ctx.set_camera_position(cam)
        ctx.upload_chain(chain)
        ctx.trace(planes)
        first = check_against_trace(ctx, planes, cam, "uploaded chain")
        # footprint records change nothing; trace_variant 3 does not reach the query, which stays exact
        ctx.set_footprint_records(True)
        ctx.trace(planes)
        again = check_against_trace(ctx, planes, cam, "footprint records")
        for a, b in zip(first, again):
            assert np.array_equal(pq.u32(a) if a.dtype == f32 else a, pq.u32(b) if b.dtype == f32 else b)
        ctx.set_footprint_records(False)
        ctx.set_trace_variant(3)
        ctx.trace(planes)
        pts = np.ascontiguousarray(planes[0:12].T)[:514]
        p = mp.params(oracle, ctx)
        ref = pq.gather(oracle, p, chain, pts)
        check_gather(ctx, ctx.gather_points(pts, want_cones=True, want_steps=True), ref, np.arange(pts.shape[0]), "variant 3")


def test_query_reads_the_bounce_chain(vct, oracle):
    from voxel_cone_tracing_amd import scene as sc
    V, w, h = 32, mp.W, mp.H
    light = (0.3, 1.0, 0.4)
    cam = sc.default_camera(position=(0.0, 0.0, 58.0))
    with vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=256, voxel_attributes=1,
                                        debug_outputs=1)) as ctx:
        ctx.upload_scene(sc.Scene(sc.CORNELL))
        ctx.set_light_direction(light)
        ctx.set_camera_position(tuple(cam.position))
        ctx.render_shadow_map(sc.light_view_proj(light))
        ctx.voxelize()
        ctx.inject_light()
        ctx.build_mips()
        radiance = ctx.download_chain()
        ctx.bounce()
        bounced = ctx.download_chain()
        assert not np.array_equal(radiance, bounced)
        ctx.render_gbuffer(sc.camera_view_proj(cam, w, h))
        ctx.trace_current()
        planes = ctx.download_gbuffer()
        assert (planes[18] >= 0.5).sum() > 500
        g, c, s = check_against_trace(ctx, planes, tuple(cam.position), "bounce chain")
        # ... and it is the bounce chain that was read: the oracle on the downloaded chains
        live = np.flatnonzero(~(planes[18] < f32(0.5)))[:514]
        pts = np.ascontiguousarray(planes[0:12].T)[live]
        p = mp.params(oracle, ctx)
        want = pq.gather(oracle, p, bounced, pts)
        pq.assert_floats_match(g[live], want["gather"], "bounce chain against the oracle")
        assert not np.array_equal(pq.u32(want["gather"]), pq.u32(pq.gather(oracle, p, radiance, pts)["gather"]))


# ---- 5. VCT_QUERY_SORT_CELLS ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [HOST, DEVICE])
@pytest.mark.parametrize("name", pc.CASES)
def test_sorted_march_gives_the_same_outputs(vct, oracle, chain, wctx, name, where):
    pts = pc.get(name)
    ref = reference(oracle, chain, name, wctx.cfg.wrap_repeat)
    for n in (pts.shape[0], 65, 1):
        idx = np.arange(n) % pts.shape[0]
        plain = gather_on(wctx, pts[idx], where)
        assert wctx.last_point_query()[3] == 0
        got = gather_on(wctx, pts[idx], where, sort=True)
        check_gather(wctx, got, ref, idx, f"{name} n={n} sorted", sorted_=True)
        for a, b in zip(plain, got):
            assert np.array_equal(a.view(np.uint32) if a.dtype == f32 else a, b.view(np.uint32) if b.dtype == f32 else b), name
    cpts = pq.cone_points_of(pts, pq.cone_dirs(oracle, pts)[:, 1])
    a, sa = cones_on(wctx, cpts, 0, where)
    b, sb = cones_on(wctx, cpts, 0, where, sort=True)
    assert wctx.last_point_query()[2:] == (1, 1)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(sa, sb)


def test_sort_with_every_point_equal(vct, oracle, chain, wctx):
    """Every key equal: a stable sort leaves the order alone, and whatever it did every index must receive its result."""
    one = pc.patch()[37]
    pts = np.ascontiguousarray(np.tile(one, (257, 1)))
    ref = pq.gather(oracle, oracle.default_params(pc.V, G=pc.G, max_distance=pc.MAX_DISTANCE, wrap_repeat=wctx.cfg.wrap_repeat),
                    chain, one[None])
    idx = np.zeros(257, np.int64)
    check_gather(wctx, gather_on(wctx, pts, HOST, sort=True), ref, idx, "equal points", sorted_=True)
    # two interleaved points: equal keys in runs, the results must land at the callers' indices
    two = np.ascontiguousarray(np.stack([pc.patch()[3], pc.scatter()[9]])[np.arange(300) % 2])
    ref2 = pq.gather(oracle, oracle.default_params(pc.V, G=pc.G, max_distance=pc.MAX_DISTANCE, wrap_repeat=wctx.cfg.wrap_repeat),
                     chain, two[:2])
    check_gather(wctx, gather_on(wctx, two, DEVICE, sort=True), ref2, np.arange(300) % 2, "two points", sorted_=True)


# ---- 6. empty chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [1, 0])
def test_empty_chain(vct, oracle, wrap):
    p = oracle.default_params(pc.V, G=pc.G, max_distance=pc.MAX_DISTANCE, wrap_repeat=wrap)
    nd, _ = oracle.max_steps(p, float(pc.TAN_DIFFUSE))
    ns, _ = oracle.max_steps(p, float(pc.TAN_SPECULAR))
    pts = np.concatenate([pc.patch(), pc.scatter()[:1]])
    with vct.Context(vct.default_config(wrap_repeat=wrap, **pc.config())) as ctx:
        g, c, s = ctx.gather_points(pts, want_cones=True, want_steps=True)
        assert not pq.u32(g).any() and not pq.u32(c).any()          # +0, not -0
        assert (s == nd).all()
        assert ctx.last_point_query() == (257, 257 * 6 * nd, 0, 0)
        cpts = pq.cone_points_of(pts, np.tile(np.array([0.0, 1.0, 0.0], f32), (257, 1)))
        for aperture, want in ((0, nd), (1, ns)):
            out, st = ctx.cone_points(cpts, aperture, want_steps=True)
            assert not pq.u32(out).any() and (st == want).all()


# ---- 7. frame slots -------------------------------------------------------------------------------------------------------------
def test_query_beside_a_trace_on_the_other_slot(vct, oracle, chain):
    w, h = 1920, 1080
    small = synth.random_gbuffer(4096, seed=4, extent=0.45 * pc.G)
    planes = np.ascontiguousarray(np.tile(small, (1, (w * h + 4095) // 4096))[:, :w * h])
    pts = pc.mixed()
    ref = reference(oracle, chain, "mixed", 1)
    idx = np.arange(pts.shape[0])
    with vct.Context(vct.default_config(voxel_dim=pc.V, width=w, height=h)) as ctx:
        ctx.upload_chain(chain)
        one_slot = gather_on(ctx, pts, HOST)
        check_gather(ctx, one_slot, ref, idx, "one slot")
        ctx.set_frames_in_flight(2)
        ctx.select_frame_slot(0)
        ctx.trace(planes)
        ctx.trace_resident()                          # queued on slot 0 ...
        ctx.select_frame_slot(1)
        got = gather_on(ctx, pts, DEVICE)             # ... and the query at once on slot 1
        check_gather(ctx, got, ref, idx, "slot 1")
        for a, b in zip(one_slot, got):
            assert np.array_equal(a.view(np.uint32) if a.dtype == f32 else a, b.view(np.uint32) if b.dtype == f32 else b)
        ctx.synchronize()


def test_queries_around_an_upload_each_see_their_own_chain(vct, oracle, chain):
    import torch
    chain2 = oracle.build_mips(synth.noise_volume(pc.V, seed=23, occupancy=0.2))
    pts = np.concatenate([pc.patch(), pc.scatter()])
    p = oracle.default_params(pc.V, G=pc.G, max_distance=pc.MAX_DISTANCE, wrap_repeat=1)
    want = [pq.gather(oracle, p, ch, pts) for ch in (chain, chain2)]
    assert not np.array_equal(pq.u32(want[0]["gather"]), pq.u32(want[1]["gather"]))
    n = pts.shape[0]
    for slots in (1, 2):
        with vct.Context(vct.default_config(**pc.config())) as ctx:
            if slots == 2:
                ctx.set_frames_in_flight(2)
            ctx.upload_chain(chain)
            d_pts = torch.from_numpy(pts).cuda()
            outs = [torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
            torch.cuda.synchronize()
            ctx.gather_points(d_pts.data_ptr(), n=n, out_device_ptr=outs[0].data_ptr())          # queued
            if slots == 2:
                ctx.select_frame_slot(1)              # the upload below is a writer on the other slot: it must wait for the query
            ctx.upload_chain(chain2)
            ctx.gather_points(d_pts.data_ptr(), n=n, out_device_ptr=outs[1].data_ptr())
            ctx.synchronize()
            for k in range(2):
                pq.assert_floats_match(outs[k].cpu().numpy(), want[k]["gather"], f"{slots} slot(s): query {k}")


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(vct, chain):
    L = vct.lib()
    INVALID = -1
    pts = pc.patch()[:8]
    cpts = np.ascontiguousarray(pts[:, :9])
    with vct.Context(vct.default_config(**pc.config())) as ctx:
        ctx.upload_chain(chain)
        h = ctx._h
        out = np.full((8, 4), -7.0, f32)
        cones = np.full((8, 6, 4), -7.0, f32)
        steps = np.full((8, 6), 201, np.uint8)
        P = lambda a: a.ctypes.data_as(C.c_void_p)

        def refused(rc, what):
            assert rc == INVALID, what
            assert L.vct_last_error(h).decode(), what
            assert (out == -7.0).all() and (cones == -7.0).all() and (steps == 201).all(), what

        refused(L.vct_gather_points(h, P(pts), -1, vct.MEM_HOST, P(out), P(cones), P(steps), 0), "n < 0")
        refused(L.vct_gather_points(h, P(pts), vct.POINT_QUERY_MAX + 1, vct.MEM_HOST, P(out), P(cones), P(steps), 0), "n > max")
        refused(L.vct_gather_points(h, None, 8, vct.MEM_HOST, P(out), P(cones), P(steps), 0), "null points")
        refused(L.vct_gather_points(h, P(pts), 8, vct.MEM_HOST, None, P(cones), P(steps), 0), "null output")
        refused(L.vct_gather_points(h, P(pts), 8, 2, P(out), P(cones), P(steps), 0), "bad location")
        refused(L.vct_gather_points(h, P(pts), 8, vct.MEM_HOST, P(out), P(cones), P(steps), 2), "unknown flags")
        refused(L.vct_cone_points(h, P(cpts), 8, vct.MEM_HOST, 2, P(out), P(steps), 0), "bad aperture")
        refused(L.vct_cone_points(h, P(cpts), 8, vct.MEM_HOST, -1, P(out), P(steps), 0), "bad aperture")
        refused(L.vct_cone_points(h, P(cpts), -5, vct.MEM_HOST, 0, P(out), P(steps), 0), "n < 0")
        refused(L.vct_cone_points(h, None, 8, vct.MEM_HOST, 0, P(out), P(steps), 0), "null points")
        refused(L.vct_cone_points(h, P(cpts), 8, vct.MEM_HOST, 0, None, P(steps), 0), "null output")
        refused(L.vct_cone_points(h, P(cpts), 8, 7, 0, P(out), P(steps), 0), "bad location")
        # n = 0 succeeds, whatever the pointers, and touches nothing
        assert L.vct_gather_points(h, None, 0, vct.MEM_HOST, None, None, None, 0) == 0
        assert L.vct_cone_points(h, None, 0, vct.MEM_DEVICE, 1, None, None, vct.QUERY_SORT_CELLS) == 0
        assert L.vct_gather_points(h, P(pts), 0, vct.MEM_HOST, P(out), P(cones), P(steps), 0) == 0
        assert (out == -7.0).all() and (cones == -7.0).all() and (steps == 201).all()
        with pytest.raises(vct.VctError):
            ctx.last_point_query()                    # no query has run yet
        assert ctx.gather_points(pts).shape == (8, 4)
        ctx.set_trace_timing(False)
        ctx.gather_points(pts)
        with pytest.raises(vct.VctError):
            ctx.last_point_query_ms()                 # issued with timing off
    with vct.Context(vct.default_config(anisotropic_mips=1, **pc.config())) as ctx:
        with pytest.raises(vct.VctError, match="anisotropic"):
            ctx.gather_points(pts)
        with pytest.raises(vct.VctError, match="anisotropic"):
            ctx.cone_points(cpts, 0)


# ---- 9. facade and demo -------------------------------------------------------------------------------------------------------
def test_demo_ambient_cubes_equal_the_ctypes_call(vct, tmp_path):
    """vct_demo --ambient-cubes drives Voxel_Cone_Tracing::GatherPoints from C++; the same points through ctypes on the
    chain the demo dumped give the same bits."""
    exe = os.path.join(ROOT, "voxel-cone-tracing_amd", "vct_demo")
    cubes, chain_file = str(tmp_path / "cubes.bin"), str(tmp_path / "chain.bin")
    V = 32
    out = subprocess.run([exe, "--scene", "procedural:cornell", "--voxels", str(V), "--size", "64x48", "--shadow", "256",
                          "--frames", "1", "--ambient-cubes", "3,2,2", cubes, "--dump-chain", chain_file],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ambient cubes: 3x2x2 probes, 72 gathers" in out.stdout, out.stdout[-500:]
    got = np.fromfile(cubes, f32)
    assert got.size == 3 * 2 * 2 * 6 * 4
    got = got.reshape(2, 2, 3, 6, 4)
    assert np.isfinite(got).all() and (got[..., 3] >= 0).all() and (got[..., 3] <= 1).all()
    assert (got[..., :3] > 0).any()                   # the probes see the lit box
    pts = np.fromfile(cubes + ".points", f32).reshape(-1, 12)
    chain = np.fromfile(chain_file, np.uint8).reshape(-1, 4)
    with vct.Context(vct.default_config(voxel_dim=V, width=8, height=8)) as ctx:
        ctx.upload_chain(chain)
        want = ctx.gather_points(pts)
    assert np.array_equal(pq.u32(got.reshape(-1, 4)), pq.u32(want))
