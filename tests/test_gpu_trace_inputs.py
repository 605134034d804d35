"""GPU: the cone trace on the adversarial G-buffers of tests/gbcases.py (whose classes tests/test_gbuffer_cases.py proves
on the oracle), in every launch form, against the oracle on the same planes.  beyond_contract pixels are never built here.

Bars, per pixel -- none of them per frame:
  * per-cone step counts equal for every in-frame pixel, and the step total;
  * raw cones of live pixels bit-identical where the oracle's component is not NaN (so +-inf and the sign of zero are
    compared), NaN where it is NaN (sign and payload differ between x86 and gfx950 and are not compared);
  * every fp16 channel of the frame within 1 fp16 ulp of the oracle's rgba16f, NaN where it is NaN, the same inf where it
    is inf.  Derived, not measured: the cones are bit-exact, so the only inexact operation is the powf of the Phong term
    (trace.fs:213); test_gbuffer_cases.check_powf_margin shows that 17 fp32 ulps of it stay under a quarter of the fp16
    spacing on these inputs, so the rounding can only move to the neighbouring half;
  * pixels whose Phong term is exactly zero in the oracle (spec * shadow == 0, or specColor == 0): bit-equal;
  * discarded pixels: exactly the clear colour with alpha 1 (the oracle's bits).
Every comparison asserts the 1-ulp bar itself; the last test only prints the worst distance the run has seen."""
import numpy as np
import pytest

import components_ref as cr
import diffuse_rate_ref as dr
import gbcases as gc
import synth
import vctpkg

pytestmark = pytest.mark.gpu

f32 = np.float32
COMP_MASK = cr.SHOW_ALL & ~cr.SHOW_DIFFUSE      # a non-default mask that still marches both cone groups
ALL_AOV = cr.AOV_INDIRECT_DIFFUSE | cr.AOV_INDIRECT_SPECULAR | cr.AOV_DIRECT
WORST = {"ulp": 0, "channels": 0}
G150 = tuple(n for n in gc.CASE_NAMES if gc.FAMILIES[n][1] == 150.0)
G100 = tuple(n for n in gc.CASE_NAMES if gc.FAMILIES[n][1] == 100.0)


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


@pytest.fixture(scope="module")
def volume(oracle):
    l0 = synth.noise_volume(gc.V, occupancy=0.3)
    return l0, oracle.build_mips(l0), oracle.build_mips_aniso(l0)


_refs = {}


def params(oracle, case, wrap, V=gc.V):
    return oracle.default_params(V, G=case.G, max_distance=case.max_distance, wrap_repeat=wrap, camera_pos=gc.CAM,
                                 light_dir=gc.LIGHT)


def reference(oracle, volume, case, wrap, aniso=False):
    key = (case.name, case.w, case.h, wrap, aniso)
    if key not in _refs:
        p = params(oracle, case, wrap)
        if aniso:
            _refs[key] = oracle.trace_aniso(p, volume[1], volume[2], case.planes, nthreads=8, want_cones=True)
        else:
            _refs[key] = oracle.trace(p, volume[1], case.planes, nthreads=8, want_cones=True)
    return _refs[key]


def context(vct, case, wrap, **kw):
    ctx = vct.Context(vct.default_config(debug_outputs=1, wrap_repeat=wrap, **case.config(), **kw))
    ctx.set_camera_position(gc.CAM)
    ctx.set_light_direction(gc.LIGHT)
    return ctx


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_floats_match(got, want, what):
    """Bit-identical where `want` is not NaN; NaN where it is."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in different places"
    assert np.array_equal(u32(got)[~nan], u32(want)[~nan]), f"{what}: not bit-identical"


def half_order(h):
    """fp16 bits -> integers in the order of the values (+-0 coincide, inf follows the largest finite half)."""
    h = np.asarray(h, np.uint16).astype(np.int64)
    return np.where(h & 0x8000, -(h & 0x7fff), h)


def assert_halves_match(got16, want16, exact, what):
    """The module docstring's frame bars.  got16 / want16: uint16 [n, 4]; exact: [n] bool, pixels that must be bit-equal."""
    got16, want16 = np.asarray(got16, np.uint16).reshape(-1, 4), np.asarray(want16, np.uint16).reshape(-1, 4)
    want_nan = (want16 & 0x7fff) > 0x7c00
    got_nan = (got16 & 0x7fff) > 0x7c00
    assert np.array_equal(got_nan, want_nan), f"{what}: NaN in different pixels / channels"
    want_inf = (want16 & 0x7fff) == 0x7c00
    assert np.array_equal((got16 & 0x7fff) == 0x7c00, want_inf), f"{what}: inf in different pixels / channels"
    assert np.array_equal(got16[want_inf], want16[want_inf]), f"{what}: an overflowing channel is not the same inf"
    dist = np.abs(half_order(got16) - half_order(want16))
    dist[want_nan] = 0
    worst = int(dist.max()) if dist.size else 0
    WORST["ulp"] = max(WORST["ulp"], worst)
    WORST["channels"] += int(dist.size)
    print(f"{what}: worst fp16 distance {worst}, channels off by one {int((dist == 1).sum())} of {dist.size}")
    assert worst <= 1, f"{what}: {np.argwhere(dist > 1)[:8]} differ by more than one fp16 ulp (worst {worst})"
    ex = np.broadcast_to(np.asarray(exact, bool)[:, None], dist.shape) & ~want_nan
    assert not dist[ex].any() and np.array_equal(got16[ex], want16[ex]), f"{what}: a pixel without a Phong term is not bit-equal"


def exact_pixels(planes, cones, p, mask=cr.SHOW_ALL):
    """Pixels whose Phong term spec * shadow * specColor is exactly zero (or not shown), and the discarded ones."""
    comp = cr.composite(planes, cones, gc.CAM, gc.LIGHT, p.ambient_factor, p.shininess, mask)
    with np.errstate(invalid="ignore"):
        no_term = (comp["direct"][:, 1] == 0) | (np.asarray(planes)[19:22] == 0).all(0) | (not mask & cr.SHOW_SPECULAR)
    return no_term | ~comp["alive"]


def check(vct, oracle, ctx, case, ref, out, what, sel=None, want16=None, mask=cr.SHOW_ALL, total=True):
    """One trace's frame and debug outputs against the oracle's `ref` on the pixels `sel` (default: the frame)."""
    n = case.w * case.h
    sel = np.ones(n, bool) if sel is None else sel
    steps, cones = ctx.steps(), ctx.cones()
    assert np.array_equal(steps[sel], ref["steps"][sel]), f"{what}: per-cone step counts differ"
    live = sel & ~(case.planes[18] < f32(0.5))
    assert_floats_match(cones[live], ref["cones"][live], f"{what}: raw cones")
    if total:
        assert ctx.last_step_count() == int(ref["steps"][sel].astype(np.int64).sum()), what
    p = params(oracle, case, ctx.cfg.wrap_repeat)
    want16 = ref["rgba16f"] if want16 is None else want16
    assert_halves_match(out.reshape(-1, 4)[sel], want16[sel], exact_pixels(case.planes, ref["cones"], p, mask)[sel], what)


def rows_mask(case, row0, row1):
    sel = np.zeros(case.w * case.h, bool)
    sel[row0 * 8 * case.w: min(row1 * 8, case.h) * case.w] = True
    return sel


@pytest.mark.parametrize("wrap", [1, 0])
@pytest.mark.parametrize("w,h", gc.FRAMES)
@pytest.mark.parametrize("names", [G150, G100], ids=["g150", "g100"])
def test_every_family_in_every_launch_form(vct, oracle, volume, names, w, h, wrap):
    """Trace variants 0, 1, 2 and 4, footprint records, a slab of tile rows, a strided slab, and a non-default component
    mask with all three outputs (against components_ref.composite), every family of one grid size on one context."""
    cases = [gc.get_case(n, w, h) for n in names]
    filler = synth.random_gbuffer(w * h, seed=7, discard_frac=0.0)
    with context(vct, cases[0], wrap) as ctx:
        ctx.upload_chain(volume[1])
        for case in cases:
            ref = reference(oracle, volume, case, wrap)
            tag = f"{case.name} {w}x{h} wrap {wrap}"
            for variant in (0, 1, 2, 4):
                ctx.set_trace_variant(variant)
                check(vct, oracle, ctx, case, ref, ctx.trace(case.planes), f"{tag} variant {variant}")
            ctx.set_trace_variant(0)
            ctx.set_footprint_records(True)
            check(vct, oracle, ctx, case, ref, ctx.trace(case.planes), f"{tag} footprint records")
            ctx.set_footprint_records(False)
            # slab: tile row 1 only; strided slab: every second row of [0, 2) = tile row 0, of the G-buffer the slab left
            # resident.  A whole-frame trace of an unrelated G-buffer goes first, so that neither launch finds the right
            # frame, steps or cones already there; a row that a launch does not trace keeps what was there.
            stale = ctx.trace(filler)
            out = ctx.trace(case.planes, rows=(1, 2))
            check(vct, oracle, ctx, case, ref, out, f"{tag} slab", sel=rows_mask(case, 1, 2))
            assert np.array_equal(ctx.download_frame()[:8], stale[:8]), f"{tag} slab: wrote outside its rows"
            ctx.trace_gbuffer_strided(0, 2, 2)
            ctx.synchronize()
            check(vct, oracle, ctx, case, ref, ctx.download_frame(), f"{tag} strided slab", sel=rows_mask(case, 0, 1))
            # lighting components + the three per-component outputs
            ctx.set_lighting_components(COMP_MASK)
            ctx.set_aov_outputs(ALL_AOV)
            p = params(oracle, case, wrap)
            want = cr.composite(case.planes, cr.masked_cones(ref["cones"], COMP_MASK, ALL_AOV), gc.CAM, gc.LIGHT,
                                p.ambient_factor, p.shininess, COMP_MASK)
            out = ctx.trace(case.planes)
            check(vct, oracle, ctx, case, ref, out, f"{tag} components", want16=cr.to_f16_bits(want["rgba32f"]), mask=COMP_MASK)
            never = np.zeros(w * h, bool)
            for bit, key in ((vct.AOV_INDIRECT_DIFFUSE, "ind"), (vct.AOV_INDIRECT_SPECULAR, "spec_cone")):
                assert_halves_match(ctx.download_aov(bit), cr.to_f16_bits(want[key]), ~never, f"{tag} output {key}")
            assert_halves_match(ctx.download_aov(vct.AOV_DIRECT), cr.to_f16_bits(want["direct"]),
                                exact_pixels(case.planes, ref["cones"], p), f"{tag} output direct")
            ctx.set_lighting_components(cr.SHOW_ALL)
            ctx.set_aov_outputs(0)


@pytest.mark.parametrize("wrap", [1, 0])
@pytest.mark.parametrize("w,h", gc.FRAMES)
@pytest.mark.parametrize("names", [G150, G100], ids=["g150", "g100"])
def test_every_family_through_the_anisotropic_chains(vct, oracle, volume, names, w, h, wrap):
    cases = [gc.get_case(n, w, h) for n in names]
    with context(vct, cases[0], wrap, anisotropic_mips=1) as ctx:
        ctx.upload_volume(volume[0])
        ctx.build_mips()
        assert np.array_equal(ctx.download_aniso(), volume[2])
        for case in cases:
            ref = reference(oracle, volume, case, wrap, aniso=True)
            check(vct, oracle, ctx, case, ref, ctx.trace(case.planes), f"{case.name} {w}x{h} wrap {wrap} anisotropic")


@pytest.mark.parametrize("w,h", gc.FRAMES)
@pytest.mark.parametrize("names", [G150, G100], ids=["g150", "g100"])
def test_every_family_at_diffuse_rate_2(vct, oracle, volume, names, w, h):
    """The half-rate gather: the restatement's acceptance tests must classify NaN and zero normals as the kernel does
    (every comparison with a NaN is false: rejected) -- marched_pixels, steps and cones equal; the frame held to the
    restatement by test_gpu_diffuse_rate.py's bars (relative L2 <= 1e-4, >= 99.9 % of the halves equal) over the channels
    the restatement gives a finite value, and NaN / inf where it gives those."""
    cases = [gc.get_case(n, w, h) for n in names]
    with context(vct, cases[0], 1) as ctx:
        ctx.upload_chain(volume[1])
        ctx.set_diffuse_rate(2)
        for case in cases:
            ref = reference(oracle, volume, case, 1)
            p = params(oracle, case, 1)
            want = dr.restate(case.planes, w, h, f32(p.G) / f32(gc.V), ref, gc.CAM, gc.LIGHT, p.ambient_factor, p.shininess)
            tag = f"{case.name} {w}x{h} rate 2"
            out = ctx.trace(case.planes).reshape(-1, 4)
            assert ctx.diffuse_rate() == (2, int(want["marched"].sum())), tag
            assert np.array_equal(ctx.steps(), want["steps"]), tag
            live = want["cls"]["alive"]
            assert_floats_match(ctx.cones()[live], want["cones"][live], tag)
            assert ctx.last_step_count() == want["total_steps"], tag
            want16 = cr.to_f16_bits(want["rgba32f"])
            wf = vct.half_to_float(want16)
            fin = np.isfinite(wf)
            assert np.array_equal(out[~fin] & 0x7c00, want16[~fin] & 0x7c00) and \
                np.array_equal((out[~fin] & 0x3ff) != 0, (want16[~fin] & 0x3ff) != 0), f"{tag}: NaN / inf in other places"
            l2 = synth.rel_l2(vct.half_to_float(out)[fin], wf[fin])
            eq = (out[fin] == want16[fin]).mean()
            print(f"{tag}: rel-L2 {l2:.3e}, fp16 equal {eq:.6f}")
            assert l2 <= 1e-4 and eq >= 0.999, tag


def test_poisoned_padding_of_a_callers_tiled_buffer(vct, oracle, volume):
    """A caller's TILED / DEVICE G-buffer of the ragged frame, its out-of-frame lanes zero and then NaN, inf and 3e38 in
    every plane (alpha >= 0.5 included): frame, steps and cones equal bit for bit, whole frame and the slab of the last
    tile row.  The cooperative sampler picks its anchor among the LIVE lanes; a padding lane is never one."""
    import torch
    w, h = gc.FRAMES[1]
    for name in ("tangent_frames", "positions_g150"):
        case = gc.get_case(name, w, h)
        tiled, inside = gc.to_tiled(case.planes, w, h)
        ref = reference(oracle, volume, case, 1)
        results = []
        filler = synth.random_gbuffer(w * h, seed=7, discard_frac=0.0)
        with context(vct, case, 1) as ctx:
            ctx.upload_chain(volume[1])
            for buf in (tiled, gc.poison_padding(tiled, inside)):
                dev = torch.from_numpy(buf).cuda()
                for rows in (None, (1, 2)):
                    ctx.trace(filler)           # an unrelated frame first: no launch finds its results already there
                    out = ctx.trace(dev.data_ptr(), rows=rows, layout=vct.GB_TILED).copy()
                    results.append((out, ctx.steps().copy(), ctx.cones().copy(), ctx.last_step_count()))
                    check(vct, oracle, ctx, case, ref, out, f"{name} tiled rows {rows}",
                          sel=None if rows is None else rows_mask(case, 1, 2))
                torch.cuda.synchronize()
        for clean, bad in zip(results[:2], results[2:]):
            assert np.array_equal(clean[0], bad[0]) and np.array_equal(clean[1], bad[1])
            assert np.array_equal(clean[2].view(np.uint32), bad[2].view(np.uint32)) and clean[3] == bad[3]


@pytest.mark.parametrize("wrap", [1, 0])
def test_nan_cones_over_an_empty_block(vct, oracle, wrap):
    """A whole frame of pixels with a zero tangent: the six diffuse cone directions are NaN and every texel index of the
    tile is 0, so the cooperative sampler serves the tile from the block around texel 0 -- empty here.  A NaN weight times
    a zero texel is NaN (the oracle: one step per diffuse cone, NaN cones); the block's all-zero shortcut must not turn that
    into 0.  The specular cone runs along reflect(-E, N) with the world-space bump normal, which has no tangent in it: it stays
    finite and marches through the empty part of the volume beside the NaN lanes."""
    w, h = 16, 8
    l0 = np.zeros((gc.V,) * 3 + (4,), np.uint8)
    l0[6:10, 6:10, 6:10] = 255
    chain = oracle.build_mips(l0)
    planes = gc.base_gbuffer(w, h)
    planes[6:9] = 0
    planes[18, 5] = 0
    case = gc.Case("zero_tangent_frame", w, h, gc.Env(150.0), planes, None, None, None)
    p = params(oracle, case, wrap)
    ref = oracle.trace(p, chain, planes, nthreads=8, want_cones=True)
    live = planes[18] >= 0.5
    assert (ref["steps"][live, :6] == 1).all() and np.isnan(ref["cones"][live, :6]).all()
    assert np.isfinite(ref["cones"][live, 6]).all()
    with context(vct, case, wrap) as ctx:
        ctx.upload_chain(chain)
        for variant in (0, 1, 2, 4):
            ctx.set_trace_variant(variant)
            check(vct, oracle, ctx, case, ref, ctx.trace(planes), f"empty block wrap {wrap} variant {variant}")


def test_clean_random_gbuffer_per_pixel(vct, oracle):
    """The per-pixel bars on an existing clean case: test_gpu_parity.test_trace_random_gbuffer's inputs, variant 0."""
    V, w, h = 64, 128, 128
    chain = oracle.build_mips(synth.noise_volume(V))
    planes = synth.random_gbuffer(w * h, seed=42, discard_frac=0.05)
    p = oracle.default_params(V)
    ref = oracle.trace(p, chain, planes, nthreads=8, want_cones=True)
    with vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, debug_outputs=1)) as ctx:
        ctx.upload_chain(chain)
        out = ctx.trace(planes)
        assert np.array_equal(ctx.steps(), ref["steps"])
        assert np.array_equal(ctx.cones().view(np.uint32), ref["cones"].view(np.uint32))
        comp = cr.composite(planes, ref["cones"], p.camera_pos[:], p.light_dir[:], p.ambient_factor, p.shininess)
        exact = (comp["direct"][:, 1] == 0) | ~comp["alive"]
        assert_halves_match(out.reshape(-1, 4), ref["rgba16f"], exact, "clean random G-buffer")


def test_worst_fp16_distance_over_the_module():
    """Report only: the worst distance over the comparisons this process has made (each asserted the bar of 1 itself)."""
    print(f"worst fp16 distance over {WORST['channels']} compared channels: {WORST['ulp']}")
