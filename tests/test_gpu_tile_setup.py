"""GPU: what a tile of the screen trace does around its marches (csrc/vct_trace.hip k_trace_tile_split, k_trace_tile) --
the tile's coordinates from the launch's multiplier and shift (csrc/vct_tilediv.h), the composite's unit light vector from
the host, the eye vector E handed from the specular wave to the composite in LDS, and the one arrival word that counts the
waves and sums their steps.

Every case compares HIP with the CPU oracle the way tests/test_gpu_parity.py does, at its tolerance (REL_L2_TOL, 99.9 %
of the fp16 values equal), with debug outputs on: per-cone step counts and raw cone vec4s bit for bit, the step total
(the sum of the per-tile counts the last arriver stores) and the per-row histogram.  Where the oracle's frame holds a NaN
(a zero light vector or a camera on a surface point can give one), the frame must hold a NaN in the same channels, and the
bars apply to the other pixels.  V = 32 throughout; one oracle run per (planes, uniforms), shared.

The forms the oracle does not trace itself are held to the references their own tests use: components_ref (masks),
diffuse_rate_ref (rate 2), gloss_ref (classes), sky_ref (sky) -- each formed from the oracle's cones.

The packed form (pack_rows) of a strided launch runs through the library's self-test, vct_selftest_interleaved; the packed
form of a row RANGE is launched only by a rank of a multi-GPU frame and shares the kernel's `oy` with the strided one."""
import numpy as np
import pytest

import components_ref as cr
import diffuse_rate_ref as dr
import gloss_ref as gr
import sky_ref as sr
import synth
import vctpkg

pytestmark = pytest.mark.gpu

f32 = np.float32
REL_L2_TOL = 1e-3          # tests/test_gpu_parity.py
V = 32
CAM, LIGHT = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


@pytest.fixture(scope="module")
def chain(oracle):
    return oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.2))


_planes, _refs = {}, {}


def gbuffer(w, h, seed=42):
    if (w, h, seed) not in _planes:
        _planes[(w, h, seed)] = synth.random_gbuffer(w * h, seed=seed, discard_frac=0.05)
    return _planes[(w, h, seed)]


def reference(oracle, chain, key, planes, **kw):
    """The oracle's trace with raw cones, once per key."""
    if key not in _refs:
        _refs[key] = oracle.trace(params(oracle, **kw), chain, planes, nthreads=8, want_cones=True)
    return _refs[key]


def params(oracle, **kw):
    return oracle.default_params(V, **{"camera_pos": CAM, "light_dir": LIGHT, **kw})


def make_ctx(vct, w, h, chain, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, debug_outputs=kw.pop("debug_outputs", 1), **kw))
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    ctx.upload_chain(chain)
    return ctx


def row_steps(steps, w, h):
    per_pixel_row = np.asarray(steps).astype(np.int64).sum(axis=1).reshape(h, w).sum(axis=1)
    return np.array([per_pixel_row[r:r + 8].sum() for r in range(0, h, 8)], np.uint64)


def assert_floats_match(got, want, what):
    """Bit-identical where `want` is not NaN, NaN where it is (sign and payload of a NaN differ between host and device)."""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in different places"
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), f"{what}: not bit-identical"


def assert_frame_matches(vct, out, want32, want16, what, sel=None):
    """test_gpu_parity.check_frame's frame bars on the pixels `sel`, NaN channels in the same places."""
    out = np.asarray(out, np.uint16).reshape(-1, 4)
    want32, want16 = np.asarray(want32, f32).reshape(-1, 4), np.asarray(want16, np.uint16).reshape(-1, 4)
    if sel is not None:
        out, want32, want16 = out[sel], want32[sel], want16[sel]
    want_nan = (want16 & 0x7fff) > 0x7c00
    assert np.array_equal((out & 0x7fff) > 0x7c00, want_nan), f"{what}: NaN in different pixels / channels"
    ok = ~want_nan.any(axis=1) & np.isfinite(want32).all(axis=1)
    err = synth.rel_l2(vct.half_to_float(out[ok]), want32[ok])
    same16 = (out[ok] == want16[ok]).mean()
    print(f"{what}: rel-L2 {err:.3e}, fp16 equal {same16:.6f}, pixels with a NaN {int(want_nan.any(axis=1).sum())}")
    assert err <= REL_L2_TOL, (what, err)
    assert same16 > 0.999, (what, same16)
    return int(want_nan.any(axis=1).sum())


def check_whole(vct, ctx, ref, out, w, h, what):
    """A whole-frame trace just made: debug outputs, totals and the frame against `ref` (the oracle's dict shape)."""
    assert np.array_equal(ctx.steps(), ref["steps"]), f"{what}: per-cone step counts differ"
    assert_floats_match(ctx.cones(), ref["cones"], f"{what}: raw cones")
    assert ctx.last_step_count() == ref["total_steps"], what
    assert np.array_equal(ctx.last_row_steps(), row_steps(ref["steps"], w, h)), what
    return assert_frame_matches(vct, out, ref["rgba32f"], ref["rgba16f"], what)


@pytest.mark.parametrize("w,h", [(8, 8), (136, 8), (8, 136), (1032, 16), (1001, 17)])
def test_frame_sizes(vct, oracle, chain, w, h):
    """One tile (tiles_x = 1: the divisor the host does not certify, so the kernel divides); one tile row of 17; one tile
    column of 17; 258 tiles = two full XCD groups of 128 and a partial one; partial tiles on both edges (126 x 3)."""
    planes = gbuffer(w, h)
    ref = reference(oracle, chain, ("size", w, h), planes)
    with make_ctx(vct, w, h, chain) as ctx:
        check_whole(vct, ctx, ref, ctx.trace(planes), w, h, f"{w}x{h}")


def test_row_ranges_and_strided_rows(vct, oracle, chain):
    """64 x 64 = 8 x 8 tiles.  A fresh context's debug outputs are zero, so the rows a launch must not touch show no steps:
    trace_gbuffer_rows(1, 3) writes rows 1 and 2, trace_gbuffer_strided(1, 8, 3) rows 1, 4 and 7.  Launches of at most
    half the frame take the kernel without issue priority around the loads."""
    w = h = 64
    planes = gbuffer(w, h, seed=5)
    ref = reference(oracle, chain, ("rows", w, h), planes)
    per_row = row_steps(ref["steps"], w, h)
    rows_of = np.repeat(np.arange(8), 8 * w)

    def check_rows(ctx, traced, untouched, what):
        ctx.synchronize()
        sel = np.isin(rows_of, traced)
        assert ctx.last_step_count() == int(per_row[list(traced)].sum()), what
        assert np.array_equal(ctx.steps()[sel], ref["steps"][sel]), what
        assert_floats_match(ctx.cones()[sel], ref["cones"][sel], what)
        assert not ctx.steps()[np.isin(rows_of, untouched)].any(), f"{what}: a row outside the launch was traced"
        assert_frame_matches(vct, ctx.download_frame(), ref["rgba32f"], ref["rgba16f"], what, sel)

    with make_ctx(vct, w, h, chain) as ctx:
        ctx.trace(planes, rows=(0, 1))                       # binds the G-buffer; row 0
        check_rows(ctx, [0], [1, 2, 3, 4, 5, 6, 7], "rows (0, 1)")
        ctx.trace_gbuffer_rows(1, 3)
        check_rows(ctx, [1, 2], [3, 4, 5, 6, 7], "rows (1, 3)")
    with make_ctx(vct, w, h, chain) as ctx:
        ctx.trace(planes, rows=(0, 1))
        ctx.trace_gbuffer_strided(1, 8, 3)
        check_rows(ctx, [1, 4, 7], [2, 3, 5, 6], "strided (1, 8, 3)")
        hist = ctx.last_row_steps()
        assert np.array_equal(hist[[1, 4, 7]], per_row[[1, 4, 7]])
        check_whole(vct, ctx, ref, ctx.trace(planes), w, h, "whole frame after the slabs")
        # (last: a packed launch stores its debug outputs at the packed pixel's index)
        assert ctx.selftest_interleaved(3) == 0               # the packed strided launches against one whole launch
        assert ctx.selftest_interleaved(8) == 0               # one tile row per rank


LIGHTS = {"default": (0.0, 1.0, 0.25), "axis": (0.0, 0.0, -1.0), "tiny": (3e-20, 4e-20, 0.0), "huge": (1e19, 1e19, 1e19),
          "zero": (0.0, 0.0, 0.0)}


@pytest.mark.parametrize("name", sorted(LIGHTS))
def test_lights(vct, oracle, chain, name):
    """The unit light vector comes from the host: non-unit, axis-aligned, squares that are denormal (3e-20), a sum of squares
    just under FLT_MAX (1e19), and the zero vector, whose 0 / 0 the composite's fmaxf terms drop or keep as the oracle's do."""
    w, h = 40, 24
    planes = gbuffer(w, h, seed=9)
    light = LIGHTS[name]
    ref = reference(oracle, chain, ("light", name), planes, light_dir=light)
    with make_ctx(vct, w, h, chain) as ctx:
        ctx.set_light_direction(light)
        check_whole(vct, ctx, ref, ctx.trace(planes), w, h, f"light {name}")
    if name not in ("default", "zero"):
        other = reference(oracle, chain, ("light", "default"), planes, light_dir=LIGHTS["default"])
        assert not np.array_equal(ref["rgba16f"], other["rgba16f"])          # the light reaches the frame


def test_camera_on_a_surface_point(vct, oracle, chain):
    """E = normalize(0) = NaN for pixels whose position is the camera's: lane 27 of the first tile (the cooperative
    sampler's anchor) and a lane of the last, partial tile.  The NaN goes through LDS into the composite untouched."""
    w, h = 21, 13
    planes = gbuffer(w, h, seed=13).copy()
    planes[18, [3 * w + 3, 12 * w + 20]] = 1.0
    cam = tuple(float(v) for v in planes[0:3, 3 * w + 3])
    planes[0:3, 12 * w + 20] = planes[0:3, 3 * w + 3]
    ref = reference(oracle, chain, ("on_camera",), planes, camera_pos=cam)
    assert np.isnan(ref["cones"][[3 * w + 3, 12 * w + 20], 6]).any()
    for variant in (0, 1):
        with make_ctx(vct, w, h, chain, trace_variant=variant) as ctx:
            ctx.set_camera_position(cam)
            nans = check_whole(vct, ctx, ref, ctx.trace(planes), w, h, f"camera on a surface point, variant {variant}")
            assert nans >= 2


def form_case(oracle, chain):
    w, h = 40, 24
    planes = gbuffer(w, h, seed=21)
    return w, h, planes, reference(oracle, chain, ("forms",), planes)


def test_plain_and_prio_by_launch_size(vct, oracle, chain):
    w, h, planes, ref = form_case(oracle, chain)
    with make_ctx(vct, w, h, chain) as ctx:
        full = ctx.trace(planes).copy()                              # more than half the frame: issue priority around the loads
        check_whole(vct, ctx, ref, full, w, h, "whole frame")
        part = ctx.trace(planes, rows=(1, 2))                        # a third: the plain kernel
        assert np.array_equal(part[8:16], full[8:16]) and ctx.last_step_count() == int(row_steps(ref["steps"], w, h)[1])


@pytest.mark.parametrize("mask", [cr.SHOW_DIFFUSE | cr.SHOW_INDIRECT_DIFFUSE | cr.SHOW_SPECULAR,
                                  cr.SHOW_SPECULAR | cr.SHOW_INDIRECT_SPECULAR], ids=["specular_group_off", "diffuse_group_off"])
def test_lighting_components(vct, oracle, chain, mask):
    """Specular group off with the direct specular term shown: the specular wave marches nothing and must still hand E
    over.  Diffuse group off: the diffuse waves arrive at once with zero cones."""
    w, h, planes, ref = form_case(oracle, chain)
    dif, spc = cr.marched_groups(mask)
    assert (dif, spc) == ((True, False) if mask & cr.SHOW_DIFFUSE else (False, True))
    p = params(oracle)
    want = cr.composite(planes, cr.masked_cones(ref["cones"], mask), CAM, LIGHT, p.ambient_factor, p.shininess, mask)
    assert (want["direct"][:, 1] > 0).mean() > 0.1                   # the Phong term, and so E, shows in many pixels
    want_steps = ref["steps"].copy()
    want_steps[:, :6] *= dif
    want_steps[:, 6] *= spc
    alive = want["alive"]
    with make_ctx(vct, w, h, chain) as ctx:
        ctx.set_lighting_components(mask)
        out = ctx.trace(planes)
        assert np.array_equal(ctx.steps(), want_steps)
        assert_floats_match(ctx.cones()[alive], cr.masked_cones(ref["cones"], mask)[alive], "masked cones")
        assert ctx.last_step_count() == cr.marched_steps(ref["steps"], mask)
        assert np.array_equal(ctx.last_row_steps(), row_steps(want_steps, w, h))
        assert_frame_matches(vct, out, want["rgba32f"], cr.to_f16_bits(want["rgba32f"]), f"mask {mask}")


def test_half_rate_diffuse(vct, oracle, chain):
    w, h, planes, ref = form_case(oracle, chain)
    p = params(oracle)
    want = dr.restate(planes, w, h, f32(p.G) / f32(V), ref, CAM, LIGHT, p.ambient_factor, p.shininess)
    with make_ctx(vct, w, h, chain) as ctx:
        ctx.set_diffuse_rate(2)
        out = ctx.trace(planes)
        assert np.array_equal(ctx.steps(), want["steps"])
        alive = want["cls"]["alive"]
        assert_floats_match(ctx.cones()[alive], want["cones"][alive], "rate 2 cones")
        assert ctx.last_step_count() == want["total_steps"]
        assert_frame_matches(vct, out, want["rgba32f"], cr.to_f16_bits(want["rgba32f"]), "rate 2")


def test_two_gloss_classes(vct, oracle, chain):
    w, h, planes, _ = form_case(oracle, chain)
    classes = gr.CLASSES[:2]
    plane = gr.checkerboard(w, h, 2)
    ref = gr.trace(oracle, params(oracle), chain, planes, classes, plane, nthreads=8)
    with make_ctx(vct, w, h, chain) as ctx:
        ctx.set_gloss_classes(classes)
        ctx.set_pixel_gloss(plane)
        check_whole(vct, ctx, ref, ctx.trace(planes), w, h, "two gloss classes")


def test_sky(vct, oracle, chain):
    w, h, planes, _ = form_case(oracle, chain)
    ref = sr.trace(oracle, params(oracle), chain, planes, sr.SH, nthreads=8)
    with make_ctx(vct, w, h, chain) as ctx:
        ctx.set_sky(sr.SH)
        check_whole(vct, ctx, ref, ctx.trace(planes), w, h, "sky")


def test_clamp_mode(vct, oracle, chain):
    w, h, planes, _ = form_case(oracle, chain)
    ref = reference(oracle, chain, ("forms", "clamp"), planes, wrap_repeat=0)
    with make_ctx(vct, w, h, chain, wrap_repeat=0) as ctx:
        check_whole(vct, ctx, ref, ctx.trace(planes), w, h, "clamp")


def test_one_wave_per_tile(vct, oracle, chain):
    """config.trace_variant 1 is k_trace_tile: the tile's coordinates by the same multiplier, E recomputed at the composite."""
    w, h, planes, ref = form_case(oracle, chain)
    with make_ctx(vct, w, h, chain, trace_variant=1) as ctx:
        check_whole(vct, ctx, ref, ctx.trace(planes), w, h, "variant 1")


def test_largest_arrival_word(vct, oracle):
    """Eight gloss classes of VCT_MAX_STEPS = 1024 steps each on one tile that holds all eight, in a volume so faint that
    the cones run their tables out: the largest step total a tile's arrival word has to carry beside the arrival count
    (debug outputs keep steps as bytes, so they are off: the stored total and the frame are what is compared)."""
    w = h = 8
    vs = f32(150.0) / f32(V)
    md = float(vs * f32(1024) + vs * f32(0.5))                 # one-voxel steps: 1024 of them end below max_distance
    classes = [(1e-5 * (k + 1), 20.0 + k) for k in range(8)]
    l0 = synth.noise_volume(V, seed=3, occupancy=0.1)
    l0[..., 3] //= 128
    faint = oracle.build_mips(l0)
    planes = synth.random_gbuffer(w * h, seed=17)
    plane = gr.checkerboard(w, h, 8)
    assert len(np.unique(plane)) == 8
    p = params(oracle, max_distance=md)
    for tan, _ in classes:
        assert oracle.max_steps(p, tan)[0] == 1024
    ref = gr.trace(oracle, p, faint, planes, classes, plane, nthreads=8)
    # the oracle keeps per-cone steps as bytes, so the tile's total is formed from whole runs: class k's run over a
    # G-buffer in which only the pixels of class k are alive counts exactly their cones
    total = 0
    for k, cls in enumerate(classes):
        only_k = planes.copy()
        only_k[18, plane != k] = 0.0
        total += oracle.trace(gr.class_params(p, cls), faint, only_k, nthreads=8)["total_steps"]
    assert total > 64 * 900                                     # most specular cones run the 1024 steps out
    with make_ctx(vct, w, h, faint, debug_outputs=0, max_distance=md) as ctx:
        ctx.set_gloss_classes(classes)
        assert (ctx.get_gloss_classes()[1] == 1024).all()
        ctx.set_pixel_gloss(plane)
        out = ctx.trace(planes)
        assert ctx.last_step_count() == total
        assert int(ctx.last_row_steps()[0]) == total
        assert_frame_matches(vct, out, ref["rgba32f"], ref["rgba16f"], "eight classes of 1024 steps")
