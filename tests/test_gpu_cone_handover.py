"""GPU: the cone hand-over of the three-wave trace kernel (csrc/vct_trace.hip k_trace_tile_split).  The waves of a tile
hand their results to the last one to arrive through the slabs they sampled from: the first diffuse wave the fold of its
own cones (the prefix of the oracle's chain over cones 0..5), the second its raw cones, the specular wave its cone and
the eye vector.  The last arriver -- any of the three -- continues the fold and composites.

Every case follows check() of tests/test_gpu_block_reuse.py, with debug outputs on: per-cone step counts and raw cones
against the oracle bit for bit (NaN equals NaN: sign and payload of a NaN differ between x86 and gfx950), the step
totals, the frame inside the parity bars, and the frame bit for bit against config.trace_variant 1 -- k_trace_tile, which
folds all six cones in one wave and hands nothing over.  The cases of "the other forms" (lighting components, emission
planes, gloss classes, the sky, the half-rate gather) have no such comparison: the host refuses every one of those
options beside trace_variant 1 .. 4 (VCT_ERR_INVALID, "... need the default trace kernel"), so the one-wave kernel
cannot run them.  They are held to the reference their own test files use, cones bit for bit.

Frame bars: relative L2 <= 1e-3 (tests/test_gpu_parity.py), and every fp16 channel within one fp16 ulp of the oracle's,
NaN where it is NaN -- the cones are bit-exact, so the Phong term's powf is the frame's only inexact operation and can
move a channel to the neighbouring half at most (tests/test_gpu_trace_inputs.py derives this).  Frames of 1000 values
or more also keep test_gpu_block_reuse's bar of 99.9 % equal halves.

Which wave arrives last is a race the test cannot observe; what it can do is make the waves' lifetimes differ, and
assert in the oracle's step counts that they do: a wave lives for as many march-loop iterations as the longest lane of
each of its cones needs (wave_iterations)."""
import numpy as np
import pytest

import components_ref as cr
import diffuse_rate_ref as drr
import emission_ref as er
import gbcases as gc
import gloss_ref as gr
import point_query_ref as pq
import sky_ref as sr
import synth
import vctpkg

pytestmark = pytest.mark.gpu

f32 = np.float32
REL_L2_TOL = 1e-3          # tests/test_gpu_parity.py
CONSTS = {"grid_world_size": "G", "max_distance": "max_distance", "max_alpha": "max_alpha", "tan_diffuse": "tan_diffuse",
          "tan_specular": "tan_specular", "shininess": "shininess", "ambient_factor": "ambient_factor",
          "wrap_repeat": "wrap_repeat"}
CAM, LIGHT = gc.CAM, gc.LIGHT
CAM_GRAZING = (300.0, -17.0, 0.0)    # three units above the floor patch, far away: the specular cone leaves nearly level


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


def make_ctx(vct, V, w, h, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, debug_outputs=1, **kw))
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    return ctx


def floor(w, h, V, discard=0.0, seed=3):
    """A coherent floor patch on which an 8x8 tile is one voxel wide (test_gpu_block_reuse.floor), with discarded pixels."""
    extent = 0.5 * (150.0 / V) * max(w, h) / 8.0
    planes = synth.coherent_gbuffer(w, h, seed=seed, plane_y=-20.0, extent=extent)
    if discard:
        planes[18, np.random.default_rng(seed + 1).uniform(size=w * h) < discard] = 0.0
    return planes


def thin_shell(V, seed=7):
    return synth.noise_volume(V, seed=seed, occupancy=0.08)


def faint(V, seed=2, divisor=16):
    """Every voxel occupied, nearly transparent: every cone runs its table out."""
    return np.random.default_rng(seed).integers(0, 256, (V, V, V, 4), dtype=np.uint8) // np.uint8(divisor)


def faint_with_opaque_slab(V, axis, lo, hi):
    """faint() with the voxels lo <= index < hi of one axis opaque, in random colours: cones that reach the slab end there."""
    l0 = faint(V)
    sl = [slice(None)] * 3
    sl[axis] = slice(lo, hi)
    blk = np.random.default_rng(1).integers(0, 256, l0[tuple(sl)].shape, dtype=np.uint8)
    blk[..., 3] = 255
    l0[tuple(sl)] = blk
    return l0


def wave_iterations(steps, w, h):
    """[ntiles, 3]: march-loop iterations of a tile's three waves (cones 0-2, cones 3-5, specular) -- a wave marches a
    cone until its last lane has ended.  Whole tiles only."""
    assert w % 8 == 0 and h % 8 == 0
    s = steps.reshape(h // 8, 8, w // 8, 8, 7).transpose(0, 2, 1, 3, 4).reshape(-1, 64, 7).max(axis=1).astype(np.int64)
    return np.stack([s[:, 0:3].sum(1), s[:, 3:6].sum(1), s[:, 6]], axis=1)


def row_steps(ref_steps, w, h):
    per_pixel_row = np.zeros(((h + 7) // 8) * 8, np.int64)
    per_pixel_row[:h] = ref_steps.astype(np.int64).sum(axis=1).reshape(h, w).sum(axis=1)
    return np.array([per_pixel_row[r:r + 8].sum() for r in range(0, h, 8)], np.uint64)


def half_order(hv):
    hv = np.asarray(hv, np.uint16).astype(np.int64)
    return np.where(hv & 0x8000, -(hv & 0x7fff), hv)


def assert_frame(vct, got16, want32, want16, what):
    """The parity bars of the module docstring; got16, want16 [npix, 4] fp16 bits, want32 [npix, 4] fp32."""
    got16, want16 = np.asarray(got16).reshape(-1, 4), np.asarray(want16).reshape(-1, 4)
    nan = (want16 & 0x7fff) > 0x7c00
    assert np.array_equal((got16 & 0x7fff) > 0x7c00, nan), f"{what}: NaN in different places"
    got = vct.half_to_float(got16)
    ok = np.isfinite(want32).all(1) & np.isfinite(got).all(1)
    err = synth.rel_l2(got[ok], want32[ok])
    dist = np.abs(half_order(got16) - half_order(want16))[~nan]
    same = (got16 == want16)[~nan].mean()
    print(f"{what}: frame relative L2 {err:.3e}, worst fp16 distance {int(dist.max())}, equal halves {same:.4f}")
    assert err <= REL_L2_TOL, (what, err)
    assert dist.max() <= 1, (what, int(dist.max()))
    if got16.size >= 1000:
        assert same > 0.999, (what, same)


def oracle_params(oracle, ctx, **kw):
    cfg = ctx.current_config()
    base = {o: getattr(cfg, k) for k, o in CONSTS.items()}
    base.update(camera_pos=CAM, light_dir=LIGHT)
    base.update(kw)
    return oracle.default_params(cfg.voxel_dim, **base)


def check(vct, oracle, ctx, chain, planes, w, h, cam=None):
    """One whole-frame trace against the oracle and against the one-wave kernel; returns (oracle result, frame)."""
    if cam is not None:
        ctx.set_camera_position(cam)
    p = oracle_params(oracle, ctx, **({} if cam is None else {"camera_pos": cam}))
    ref = oracle.trace(p, chain, planes, nthreads=8, want_cones=True)
    out = ctx.trace(planes).copy()
    assert np.array_equal(ctx.steps(), ref["steps"]), "per-cone step counts differ"
    pq.assert_floats_match(ctx.cones(), ref["cones"], "raw cones")
    assert ctx.last_step_count() == ref["total_steps"]
    assert np.array_equal(ctx.last_row_steps(), row_steps(ref["steps"], w, h))
    assert_frame(vct, out, ref["rgba32f"], ref["rgba16f"], "frame")
    ctx.set_trace_variant(1)                     # one wave folds all six cones: the same frame, bit for bit
    try:
        assert np.array_equal(ctx.trace(planes), out), "frame differs from the kernel that hands nothing over"
    finally:
        ctx.set_trace_variant(0)
    return ref, out


CLEAR = np.array([0x3800, 0x3800, 0x3800, 0x3c00], np.uint16)       # (0.5, 0.5, 0.5, 1)


# ---- partial tiles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,w,h", [(32, 20, 12), (16, 9, 9)])
def test_partial_tiles_and_discarded_pixels(vct, oracle, V, w, h):
    """Tiles ragged in both axes and 15 % discarded pixels: lanes outside the frame and lanes that march nothing hand
    over zero cones, which must stay +0 through the prefix fold, and a discarded pixel keeps the clear colour."""
    chain = oracle.build_mips(thin_shell(V))
    planes = floor(w, h, V, discard=0.15)
    dead = planes[18] < f32(0.5)
    assert 0 < dead.sum() < w * h
    with make_ctx(vct, V, w, h) as ctx:
        ctx.upload_chain(chain)
        ref, out = check(vct, oracle, ctx, chain, planes, w, h)
        assert not ref["steps"][dead].any() and ref["steps"][~dead].any()
        assert (out.reshape(-1, 4)[dead] == CLEAR).all()
        assert not ctx.cones()[dead].view(np.uint32).any()


# ---- every wave as the last arriver ----------------------------------------------------------------------------------------
LIFETIMES = {
    # name: (volume, config, apertures, camera, order asserted on wave_iterations' columns [first, second, specular])
    "specular_last": (lambda V: faint_with_opaque_slab(V, 2, 15, V), {}, None, CAM_GRAZING,
                      lambda it: (it[:, 2] > it[:, 0]).all() and (it[:, 2] > it[:, 1]).all()),
    "a_diffuse_wave_last": (lambda V: faint(V), dict(max_distance=60.0), (0.577, 0.9), None,
                            lambda it: (it[:, 2] < it[:, 0]).all() and (it[:, 2] < it[:, 1]).all()),
    "first_wave_last": (lambda V: faint_with_opaque_slab(V, 0, 17, V), dict(max_distance=60.0), (0.2, 0.9), None,
                        lambda it: (it[:, 0] > it[:, 1]).all() and (it[:, 1] > it[:, 2]).all()),
    "second_wave_last": (lambda V: faint_with_opaque_slab(V, 0, 0, 15), dict(max_distance=60.0), (0.2, 0.9), None,
                         lambda it: (it[:, 1] > it[:, 0]).all() and (it[:, 0] > it[:, 2]).all()),
}


@pytest.mark.parametrize("name", list(LIFETIMES))
def test_every_wave_as_last_arriver(vct, oracle, name):
    """The waves' lifetimes made to differ, in every tile of the frame:
    specular_last        an opaque slab beside the patch ends the diffuse cones early, and the specular cone, nearly
                         level under a grazing camera, runs its table out
    a_diffuse_wave_last  a faint volume, apertures (0.577, 0.9) and a short max_distance: the specular table is shorter
                         than three diffuse marches (the two diffuse waves live equally long)
    first_wave_last      a slab on the side cones 3-5 lean to, diffuse aperture 0.2 (seven steps): the second wave ends early
    second_wave_last     the slab on the other side: the first wave ends early"""
    volume, cfg, apertures, cam, order = LIFETIMES[name]
    V, w, h = 32, 16, 16
    chain = oracle.build_mips(volume(V))
    planes = floor(w, h, V)
    with make_ctx(vct, V, w, h, **cfg) as ctx:
        if apertures:
            ctx.set_cone_apertures(*apertures)
        ctx.upload_chain(chain)
        ref, _ = check(vct, oracle, ctx, chain, planes, w, h, cam=cam)
        it = wave_iterations(ref["steps"], w, h)
        print(f"{name}: wave iterations per tile {it.tolist()}")
        assert order(it), it.tolist()


# ---- non-finite G-buffer lanes ---------------------------------------------------------------------------------------------
def test_nan_cones_pass_through_prefix_and_folds(vct, oracle):
    """A NaN tangent frame (six NaN diffuse cones: through the first wave's prefix, the second wave's raw cones and the
    last arriver's folds), the camera on the surface point (a NaN specular cone and eye vector) and an infinite normal,
    on lanes 27, 28 and 36 of tile 0 -- the anchor lane and two neighbours.  Every other pixel is the clean frame's."""
    V, w, h = 32, 20, 12
    env = gc.Env(150.0)
    t_zero, on_camera = gc._tangent_frames(env, False)[0], gc._view_vector(env, False)[0]
    base = floor(w, h, V, discard=0.05)
    a, b, c = 3 * w + 3, 3 * w + 4, 4 * w + 4
    base[18, [a, b, c]] = 1.0
    planes = base.copy()
    for pix, spec in ((a, t_zero), (b, on_camera)):
        px = planes[:, pix].copy()
        with np.errstate(all="ignore"):
            spec(px)
        planes[:, pix] = px
    planes[3:6, c] = np.inf                              # cone start = P + N * vs: an infinite position, NaN samples
    chain = oracle.build_mips(thin_shell(V))
    with make_ctx(vct, V, w, h) as ctx:
        ctx.upload_chain(chain)
        _, clean = check(vct, oracle, ctx, chain, base, w, h)
        clean_steps, clean_cones = ctx.steps().copy(), ctx.cones().copy()
        ref, out = check(vct, oracle, ctx, chain, planes, w, h)
        assert np.isnan(ref["cones"][a, :6]).all() and (ref["steps"][a, :6] == 1).all()
        assert np.isnan(ref["cones"][b, 6]).all() and ref["steps"][b, 6] == 1
        assert np.isnan(ref["cones"][c]).all()
        others = np.ones(w * h, bool)
        others[[a, b, c]] = False
        assert np.array_equal(out.reshape(-1, 4)[others], clean.reshape(-1, 4)[others])
        assert np.array_equal(ctx.steps()[others], clean_steps[others])
        assert np.array_equal(ctx.cones()[others].view(np.uint32), clean_cones[others].view(np.uint32))


# ---- clamp to edge -----------------------------------------------------------------------------------------------------------
def test_clamp_to_edge(vct, oracle):
    """wrap_repeat = 0: the instantiations without block reuse, with their own register budget."""
    V, w, h = 16, 20, 12
    chain = oracle.build_mips(thin_shell(V, seed=9))
    with make_ctx(vct, V, w, h, wrap_repeat=0) as ctx:
        ctx.upload_chain(chain)
        ref, _ = check(vct, oracle, ctx, chain, floor(w, h, V, discard=0.1), w, h)
        assert ref["steps"].max() > 3


# ---- the other forms of the kernel --------------------------------------------------------------------------------------------
FV, FW, FH = 32, 16, 16


@pytest.fixture(scope="module")
def forms(oracle):
    """(chain, planes, oracle params, the oracle's trace) shared by the cases below; planes is left unchanged."""
    chain = oracle.build_mips(thin_shell(FV, seed=12))
    planes = floor(FW, FH, FV, discard=0.1)
    p = oracle.default_params(FV, camera_pos=CAM, light_dir=LIGHT)
    return chain, planes, p, oracle.trace(p, chain, planes, nthreads=8, want_cones=True)


def forms_ctx(vct, forms):
    ctx = make_ctx(vct, FV, FW, FH)
    ctx.upload_chain(forms[0])
    return ctx


@pytest.mark.parametrize("off", ["diffuse", "specular"])
def test_components_with_a_cone_group_switched_off(vct, forms, off):
    """COMP: the waves of a group nothing reads march zero steps, hand over zero cones and arrive at once."""
    chain, planes, p, ref = forms
    mask = (cr.SHOW_SPECULAR | cr.SHOW_INDIRECT_SPECULAR) if off == "diffuse" else (cr.SHOW_DIFFUSE | cr.SHOW_INDIRECT_DIFFUSE)
    assert cr.marched_groups(mask) == ((False, True) if off == "diffuse" else (True, False))
    live = ~(planes[18] < f32(0.5))
    with forms_ctx(vct, forms) as ctx:
        ctx.set_lighting_components(mask)
        out = ctx.trace(planes)
        want = cr.masked_cones(ref["cones"], mask)
        pq.assert_floats_match(ctx.cones(), want, f"{off} off: cones")
        steps = ctx.steps()
        if off == "diffuse":
            assert not steps[:, :6].any() and np.array_equal(steps[:, 6], ref["steps"][:, 6])
        else:
            assert not steps[:, 6].any() and np.array_equal(steps[:, :6], ref["steps"][:, :6])
        assert ctx.last_step_count() == cr.marched_steps(ref["steps"], mask)
        comp = cr.composite(planes, want, CAM, LIGHT, p.ambient_factor, p.shininess, mask)
        assert_frame(vct, out, comp["rgba32f"], cr.to_f16_bits(comp["rgba32f"]), f"{off} off")
        assert (out.reshape(-1, 4)[~live] == CLEAR).all()


def test_components_with_emission_planes(vct, forms):
    chain, planes, p, ref = forms
    E = np.abs(np.random.default_rng(8).normal(size=(3, FW * FH))).astype(f32)
    with forms_ctx(vct, forms) as ctx:
        ctx.set_pixel_emission(E)
        out = ctx.trace(planes)
        assert np.array_equal(ctx.steps(), ref["steps"])
        pq.assert_floats_match(ctx.cones(), ref["cones"], "emission: cones")
        want16 = er.frame(ref["rgba32f"], planes, E)
        assert_frame(vct, out, vct.half_to_float(want16), want16, "emission")


def test_two_gloss_classes_in_one_tile(vct, oracle, forms):
    """GLOSS: the specular wave marches once per class and keeps each lane's cone until its last march is over."""
    chain, planes, p, _ = forms
    classes = list(gr.CLASSES[:2])
    plane = gr.checkerboard(FW, FH, 2)
    assert len(np.unique(plane[:8 * FW].reshape(8, FW)[:, :8])) == 2           # both classes inside tile 0
    ref = gr.trace(oracle, p, chain, planes, classes, plane)
    live = ~(planes[18] < f32(0.5))
    with forms_ctx(vct, forms) as ctx:
        ctx.set_gloss_classes(classes)
        ctx.set_pixel_gloss(plane)
        out = ctx.trace(planes)
        assert np.array_equal(ctx.steps(), ref["steps"])
        pq.assert_floats_match(ctx.cones()[live], ref["cones"][live], "gloss: cones")
        assert ctx.last_step_count() == ref["total_steps"]
        assert_frame(vct, out, ref["rgba32f"], ref["rgba16f"], "gloss")
        assert (out.reshape(-1, 4)[~live] == CLEAR).all()


@pytest.mark.parametrize("gloss", [False, True], ids=["plain", "gloss"])
def test_sky(vct, oracle, forms, gloss):
    """SKY: every marched cone adds the sky behind its march -- with gloss classes, to the cone the wave kept."""
    chain, planes, p, _ = forms
    live = ~(planes[18] < f32(0.5))
    classes = list(gr.CLASSES[:2])
    plane = gr.checkerboard(FW, FH, 2)
    if gloss:
        ref = gr.select([sr.trace(oracle, gr.class_params(p, c), chain, planes, sr.SH) for c in classes], plane, classes)
    else:
        ref = sr.trace(oracle, p, chain, planes, sr.SH)
    with forms_ctx(vct, forms) as ctx:
        if gloss:
            ctx.set_gloss_classes(classes)
            ctx.set_pixel_gloss(plane)
        ctx.set_sky(sr.SH)
        out = ctx.trace(planes)
        assert np.array_equal(ctx.steps(), ref["steps"])
        pq.assert_floats_match(ctx.cones()[live], ref["cones"][live], "sky: cones")
        assert ctx.last_step_count() == ref["total_steps"]
        assert_frame(vct, out, ref["rgba32f"], ref["rgba16f"], "sky")
        assert (out.reshape(-1, 4)[~live] == CLEAR).all()


def test_half_rate_diffuse_gather(vct, forms):
    """HALF: the diffuse waves march nothing and hand nothing over; the composite takes the pass's gather."""
    chain, planes, p, ref = forms
    live = ~(planes[18] < f32(0.5))
    r2 = drr.restate(planes, FW, FH, f32(p.G) / f32(FV), ref, CAM, LIGHT, p.ambient_factor, p.shininess)
    marched = r2["cls"]["marched"]
    assert 0 < marched.sum() < live.sum()
    with forms_ctx(vct, forms) as ctx:
        full = ctx.trace(planes).reshape(-1, 4).copy()
        ctx.set_diffuse_rate(2)
        got = ctx.trace(planes)
        assert np.array_equal(ctx.steps(), r2["steps"]) and ctx.last_step_count() == r2["total_steps"]
        pq.assert_floats_match(ctx.cones()[live], r2["cones"][live], "rate 2: cones")
        assert np.array_equal(got.reshape(-1, 4)[marched], full[marched])        # pixels that march their own cones: rate 1's
        assert_frame(vct, got, r2["rgba32f"], cr.to_f16_bits(r2["rgba32f"]), "rate 2")


# ---- row-limited, strided and packed launches ----------------------------------------------------------------------------------
def test_rows_strided_and_packed_launches(vct, oracle):
    """Launches of at most half the frame take the instantiation without issue priority around the loads."""
    V, w, h = 32, 8, 24
    chain = oracle.build_mips(thin_shell(V, seed=14))
    planes = floor(w, h, V, discard=0.1)
    with make_ctx(vct, V, w, h) as ctx:
        ctx.upload_chain(chain)
        ref, full = check(vct, oracle, ctx, chain, planes, w, h)
        per_row = row_steps(ref["steps"], w, h)
        for r in range(3):
            part = ctx.trace(planes, rows=(r, r + 1))
            assert np.array_equal(part[r * 8:r * 8 + 8], full[r * 8:r * 8 + 8]) and ctx.last_step_count() == per_row[r]
            sel = slice(r * 64, r * 64 + 64)
            assert np.array_equal(ctx.steps()[sel], ref["steps"][sel])
            pq.assert_floats_match(ctx.cones()[sel], ref["cones"][sel], f"row {r}: cones")
        ctx.trace(planes)
        for rank in range(3):
            ctx.trace_gbuffer_strided(rank, 3, 3)
            ctx.synchronize()
            assert ctx.last_step_count() == per_row[rank]
            assert np.array_equal(ctx.download_frame()[rank * 8:rank * 8 + 8], full[rank * 8:rank * 8 + 8])
        assert ctx.selftest_interleaved(3) == 0


# ---- two launches in a row ---------------------------------------------------------------------------------------------------------
def test_two_launches_in_a_row(vct, oracle):
    """Nothing a launch left in a slab may reach the next one's hand-over: the same frame from the same context, again
    after a launch with other apertures (other cones in every slab) in between."""
    V, w, h = 32, 20, 12
    chain = oracle.build_mips(thin_shell(V, seed=12))
    planes = floor(w, h, V, discard=0.1)
    with make_ctx(vct, V, w, h) as ctx:
        ctx.upload_chain(chain)
        _, first = check(vct, oracle, ctx, chain, planes, w, h)
        steps, cones = ctx.steps().copy(), ctx.cones().copy()
        assert np.array_equal(ctx.trace(planes), first)
        ctx.trace_resident(); ctx.trace_resident(); ctx.synchronize()
        assert np.array_equal(ctx.download_frame(), first)
        ctx.set_cone_apertures(0.3, 0.2)
        other = ctx.trace(planes).copy()
        assert not np.array_equal(other, first)
        ctx.set_cone_apertures(0.577, 0.07)
        assert np.array_equal(ctx.trace(planes), first)
        assert np.array_equal(ctx.steps(), steps) and np.array_equal(ctx.cones().view(np.uint32), cones.view(np.uint32))
