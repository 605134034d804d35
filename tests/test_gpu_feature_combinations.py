"""GPU: the newer features together -- sky, gloss classes, pixel emission, local lights, the half-rate gather, lighting
components and per-component outputs in ONE launch -- against tests/frame_ref.py, which stacks the features' own reference
modules (tests/test_frame_ref_restatement.py holds it to each of them).  Each feature file composes its reference by hand for
the pairs its author thought of; this file runs a fixed table of combinations, one context per case.

Shapes: V = 16 and 32, frames 24 x 16 (whole tiles) and 37 x 21 (ragged in both axes), debug outputs on.  Inputs: dense
(30 %) and thin (8 %) noise volumes under the coherent floor with a lifted block, a lifted one-pixel line and 5 % discarded
pixels (test_gpu_sky.rate2_gbuffer's construction), on which rate 2 both interpolates and marches.  Before any launch the
inputs are shown, on the reference, not to be degenerate (test_the_inputs_are_not_degenerate).

Bars, all the project's own: per-cone steps, their total and the raw cones of live pixels bit for bit (NaN equals NaN); the
frame by test_gpu_cone_handover.assert_frame (relative L2 <= 1e-3, every fp16 channel within one fp16 ulp -- derived in
test_gpu_trace_inputs.py); at rate 2 the pixels that march their own cones equal rate 1's frame bit for bit; lit planes as
test_gpu_lights.test_specular_term holds them (fp16 values: >= 99.9 % equal, the rest within one ulp, +0 where discarded);
outputs as test_gpu_sky and test_gpu_components hold them (the specular cone's halves equal, the others within one ulp).

Accounting, after test_gpu_march_params.py's REACHED / launch_of: every launch records which instantiation of
k_trace_tile_split's SKY / GLOSS / HALF forms and of k_point_march the dispatch selected for it, and the last test asserts
that the set reached is the set vct_plan_launch (csrc/vct_trace_forms.h) and launch_point_march can select."""
import numpy as np
import pytest

import components_ref as cr
import frame_ref as fr
import gbuffer_import_ref as ir
import gloss_ref as gr
import lights_ref as lr
import point_query_ref as pq
import sky_ref as sr
import synth
import vctpkg
from test_gpu_cone_handover import assert_frame, half_order
from test_gpu_diffuse_rate import MASKS
from test_gpu_march_params import IEEE, LOOSE_HALF, PRODUCT, step_table, structurally_ok

pytestmark = pytest.mark.gpu

f32 = np.float32
G = 150.0
CAM, LIGHT = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)
CLASSES = list(gr.CLASSES[:3])
ALL_AOV = cr.AOV_INDIRECT_DIFFUSE | cr.AOV_INDIRECT_SPECULAR | cr.AOV_DIRECT
CLEAR = np.array([0x3800, 0x3800, 0x3800, 0x3c00], np.uint16)      # (0.5, 0.5, 0.5, 1)
# lights for the floor patch (y around -20, |x|, |z| <= 60): each reaches part of the frame only
TWO_LIGHTS = [lr.point((10.0, -10.0, -20.0), (400.0, 300.0, 200.0), 45.0, 2.0),
              lr.spot((-40.0, 10.0, 20.0), (900.0, 900.0, 500.0), 70.0, 1.5, (0.6, -1.0, -0.3), 0.9, 0.3)]
ONE_LIGHT = TWO_LIGHTS[:1]
SCENES = {"dense32": (32, 37, 21, 0.3), "thin32": (32, 24, 16, 0.08), "dense16": (16, 24, 16, 0.3), "thin16": (16, 37, 21, 0.08)}

# ---- the instantiations a launch with these features can select (csrc/vct_trace_forms.h, csrc/vct_trace.hip) --------------
# k_trace_tile_split<WRAP, FASTDIV, SF_COMP | {SF_PRIO, SF_HALF, SF_GLOSS, SF_SKY}>, as (WRAP, division, PRIO, SKY, GLOSS, HALF):
#   vct_plan_launch (csrc/vct_trace_forms.h), the rate-1 branches: with a sky (GLOSS by the plane, PRIO by spec_prio) or with
#     gloss classes alone; with neither, the ordinary COMP forms, which test_gpu_march_params.py accounts for;
#   vct_plan_launch, the half-rate branch: the pass's last launch, whole frames only, so PRIO always; every SKY x GLOSS.
# k_point_march<WRAP, FASTDIV, LISTED, WAVES = 1, SKY>, as (WRAP, division, LISTED, SKY): launch_point_march (csrc/vct_trace.hip),
#   once with LISTED = false and once with true in every half-rate pass (launch_half_rate).  WAVES = 2 is an A/B switch of the
#   environment (VCT_DIFFUSE_RATE_WAVES) and not a form a caller can select.
SPLIT_FORMS = ({("k_trace_tile_split", wrap, div, prio, sky, gloss, False) for wrap in (0, 1) for div in (IEEE, PRODUCT)
                for prio in (False, True) for sky, gloss in ((True, False), (False, True), (True, True))}
               | {("k_trace_tile_split", wrap, div, True, sky, gloss, True) for wrap in (0, 1) for div in (IEEE, PRODUCT)
                  for sky in (False, True) for gloss in (False, True)})
POINT_FORMS = {("k_point_march", wrap, div, listed, sky) for wrap in (0, 1) for div in (IEEE, PRODUCT)
               for listed in (False, True) for sky in (False, True)}
REACHED = set()


def launch_of(wrap, div, what, ty):
    """The instantiations vct_launch_trace selects for a launch of `what` (csrc/vct_trace_forms.h vct_plan_launch)."""
    sky, gloss = what["sky"] is not None, what["classes"] is not None
    if what["rate"] == 2 and cr.marched_groups(what["mask"], what["aov"])[0]:
        return {("k_trace_tile_split", wrap, div, True, sky, gloss, True),
                ("k_point_march", wrap, div, False, sky), ("k_point_march", wrap, div, True, sky)}
    if not (sky or gloss):
        return set()
    r0, r1, stride = what["row_span"] or (0, ty, 1)
    slab = ((r1 - r0) // stride) * 2 <= ty                             # vct_launch_trace_rows: p.spec_prio
    return {("k_trace_tile_split", wrap, div, not slab, sky, gloss, False)}


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def floor_gbuffer(w, h):
    """The coherent floor with a lifted block, a lifted one-pixel line and 5 % discarded pixels."""
    g = synth.coherent_gbuffer(w, h).reshape(23, h, w).copy()
    g[1, 2:6, 3:9] += 10.0
    g[1, :, 13] += 10.0
    g[18][np.random.default_rng(5).uniform(size=(h, w)) < 0.05] = 0.0
    return np.ascontiguousarray(g.reshape(23, h * w), f32)


_scenes = {}


def scene(oracle, name):
    if name not in _scenes:
        V, w, h, occ = SCENES[name]
        r = np.random.default_rng(8)
        _scenes[name] = dict(V=V, w=w, h=h, ty=(h + 7) // 8, planes=floor_gbuffer(w, h),
                             chain=oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=occ)),
                             E=r.uniform(0.0, 2.0, (3, w * h)).astype(f32), gloss_plane=gr.checkerboard(w, h, 3, in_frame_extra=200),
                             caches={})
    return _scenes[name]


def everything(s, **kw):
    d = dict(classes=CLASSES, gloss_plane=s["gloss_plane"], sky=sr.SH, emission=s["E"], lights=TWO_LIGHTS)
    d.update(kw)
    return d


def test_the_inputs_are_not_degenerate(oracle):
    """On the reference alone: rate 2 both interpolates and marches, every gloss class is in some tile, cones end open and
    closed, and every light reaches some voxels and pixels and not others."""
    for name in SCENES:
        s = scene(oracle, name)
        V, w, h = s["V"], s["w"], s["h"]
        p = oracle.default_params(V, camera_pos=CAM, light_dir=LIGHT)
        ref = fr.frame_ref(oracle, p, s["chain"], s["planes"], w, h, fr.attached(**everything(s, rate=2)),
                           s["caches"].setdefault("check", {}))
        live = ref["live"]
        assert 0 < ref["marched"].sum() < live.sum(), name
        tile = (np.arange(w * h) // w // 8) * ((w + 7) // 8) + (np.arange(w * h) % w) // 8
        cls = gr.clamp_class(s["gloss_plane"], len(CLASSES))
        for k in range(len(CLASSES)):
            assert len(np.unique(tile[live & (cls == k)])) >= 1 and (cls[live] == k).any(), (name, k)
        pairs = {(t, k) for t, k in zip(tile[live], cls[live])}
        assert len(pairs) == len(np.unique(tile[live])) * len(CLASSES), name          # every class in every tile
        alpha = sr.oracle_runs(oracle, p, s["chain"], s["planes"])[1]["cones"][live][..., 0]
        if name.startswith("dense"):
            assert (alpha < f32(p.max_alpha)).any() and (alpha >= f32(p.max_alpha)).any(), name
        else:
            assert (alpha < f32(p.max_alpha)).any(), name
        P = [s["planes"][0], s["planes"][1], s["planes"][2]]
        c = lr.voxel_centres(V, G)
        centres = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
        for light in TWO_LIGHTS + lr.many_lights():
            L = lr.fold(light)
            inside = lr.term(L, P)[0][live]
            if light in TWO_LIGHTS:
                assert inside.any() and not inside.all(), name
            d2 = ((centres - np.asarray(light["position"], f32)) ** 2).sum(1)
            assert (d2 < light["radius"] ** 2).any() and not (d2 < light["radius"] ** 2).all(), name
        lit = ref["lit"][:, live]
        assert (lit != s["E"][:, live]).any(0).sum() >= 20 and (lit == s["E"][:, live]).all(0).sum() >= 20, name


# ---- one context, one launch ----------------------------------------------------------------------------------------------
def context(vct, s, debug=1, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=s["V"], width=s["w"], height=s["h"], debug_outputs=debug, voxel_attributes=1, **kw))
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    ctx.upload_chain(s["chain"])
    return ctx


def params(oracle, ctx):
    cfg = ctx.current_config()
    return oracle.default_params(cfg.voxel_dim, G=cfg.grid_world_size, max_distance=cfg.max_distance, max_alpha=cfg.max_alpha,
                                 tan_diffuse=cfg.tan_diffuse, tan_specular=cfg.tan_specular, shininess=cfg.shininess,
                                 ambient_factor=cfg.ambient_factor, wrap_repeat=cfg.wrap_repeat, camera_pos=CAM, light_dir=LIGHT)


def expected_form(ctx, classes):
    """test_gpu_march_params.expected_form with the class tables: one verdict covers the diffuse table, the specular table
    and every class's (include/vct.h "per-material gloss")."""
    cfg = ctx.current_config()
    tans = [cfg.tan_diffuse, cfg.tan_specular] + [c[0] for c in (classes or [])]
    tables = [st for t in tans for st in step_table(cfg.voxel_dim, cfg.grid_world_size, t, cfg.max_distance)]
    if f32(1.0) - f32(cfg.max_alpha) < f32(2.0 ** -5):
        return IEEE
    for st in tables:
        if st[2] and not (st[3] >= f32(2.0 ** -10) and f32(1.0) - st[3] >= f32(2.0 ** -10)):
            return IEEE
    for d in sorted({float(f32(cfg.grid_world_size) * f32(0.5))} | {float(st[1]) for st in tables}):
        if not structurally_ok(d) or ctx.selftest_const_divide(d) > 0:
            return IEEE
    return PRODUCT


def attach(ctx, what):
    ctx.set_diffuse_rate(1)
    ctx.set_gloss_classes(what["classes"])
    if what["classes"] is not None:
        ctx.set_pixel_gloss(what["gloss_plane"])
    ctx.set_sky(what["sky"])
    ctx.set_pixel_emission(what["emission"])
    ctx.set_lights(what["lights"])
    ctx.set_lighting_components(what["mask"])
    ctx.set_aov_outputs(what["aov"])
    ctx.set_diffuse_rate(what["rate"])


def f16_ulps(a, b):
    return np.abs(half_order(cr.to_f16_bits(a)) - half_order(cr.to_f16_bits(b)))


def launch_and_check(vct, oracle, ctx, s, name, form=None, launch=None, planes=None, set_state=True, full=None, **kw):
    """Attach `kw` (frame_ref.attached's arguments), launch (vct_trace of the scene's planes unless `launch` does it and
    returns the frame), and hold everything the launch left to frame_ref.  Returns (frame [npix, 4], reference)."""
    what = fr.attached(**kw)
    planes = s["planes"] if planes is None else planes
    w, h = s["w"], s["h"]
    cfg = ctx.current_config()
    if set_state:
        attach(ctx, what)
    want_form = expected_form(ctx, what["classes"])
    if form is not None:
        assert want_form == form, f"{name}: the restated rule disagrees with the case's intent"
    p = params(oracle, ctx)
    cache = s["caches"].setdefault((bytes(p), planes.tobytes() if planes is not s["planes"] else None), {})
    ref = fr.frame_ref(oracle, p, s["chain"], planes, w, h, what, cache)
    out = (launch() if launch else ctx.trace(planes, rows=kw.get("rows"))).reshape(-1, 4)
    assert ctx.stage_counts()["march_division"] == want_form, name
    REACHED.update(launch_of(cfg.wrap_repeat, want_form, what, s["ty"]))
    sel, live = ref["sel"], ref["live"]
    if cfg.debug_outputs:
        assert np.array_equal(ctx.steps()[sel], ref["steps"][sel]), f"{name}: per-cone step counts"
        pq.assert_floats_match(ctx.cones()[sel & live], ref["cones"][sel & live], f"{name}: raw cones")
    assert ctx.last_step_count() == ref["total_steps"], name
    assert_frame(vct, out[sel], ref["frame32"][sel], ref["frame16"][sel], name)
    assert (out[sel & ~live] == CLEAR).all(), f"{name}: a discarded pixel is not the clear colour"
    if what["rate"] == 2 and full is not None and ref["marched"].any():
        assert np.array_equal(out[ref["marched"]], full[ref["marched"]]), f"{name}: a pixel that marches its own cones is not rate 1's"
        assert ctx.diffuse_rate() == (2, int(ref["marched"].sum())), name
    if what["lights"]:
        got = ctx.download_pixel_lights()
        d = f16_ulps(got[:, sel], ref["lit"][:, sel])
        print(f"{name}: lit planes: fp16 values equal {(d == 0).mean():.5f}, max {d.max()} ulp")
        assert (d == 0).mean() >= 0.999 and d.max() <= 1, name
        assert not got[:, sel & ~live].any(), name
    for bit, want in ref["outputs"].items():
        got = ctx.download_aov(bit).reshape(-1, 4)
        want16 = cr.to_f16_bits(want)
        assert (got[sel & ~live] == 0).all(), (name, bit)
        if bit == cr.AOV_INDIRECT_SPECULAR:
            assert np.array_equal(got[sel & live], want16[sel & live]), f"{name}: specular output"
        else:
            finite = ((want16 & 0x7fff) <= 0x7c00).all(1) & sel & live
            assert np.abs(half_order(got[finite]) - half_order(want16[finite])).max() <= 1, (name, bit)
    return out, ref


# ---- the table ------------------------------------------------------------------------------------------------------------
SWEEPS = [("dense32", 1, {}, PRODUCT), ("thin32", 0, {}, PRODUCT),
          ("dense16", 1, dict(max_alpha=0.97), IEEE), ("thin16", 0, dict(max_alpha=0.97), IEEE)]


@pytest.mark.parametrize("name,wrap,consts,form", SWEEPS,
                         ids=[f"{n}-wrap{w}-{'ieee' if f == IEEE else 'product'}" for n, w, _, f in SWEEPS])
def test_every_sky_gloss_half_form(vct, oracle, name, wrap, consts, form):
    """Lights and emission planes attached throughout; sky x gloss classes at rate 1 (whole frame: the PRIO forms; tile rows
    (1, 2): the forms without) and at rate 2."""
    s = scene(oracle, name)
    with context(vct, s, wrap_repeat=wrap, **consts) as ctx:
        for sky, gloss in ((True, False), (False, True), (True, True), (False, False)):
            kw = dict(emission=s["E"], lights=TWO_LIGHTS, sky=sr.SH if sky else None)
            if gloss:
                kw.update(classes=CLASSES, gloss_plane=s["gloss_plane"])
            what = f"{name} wrap={wrap} sky={sky} gloss={gloss}"
            full, _ = launch_and_check(vct, oracle, ctx, s, what + " rate 1", form, **kw)
            full = full.copy()
            launch_and_check(vct, oracle, ctx, s, what + " rows (1, 2)", form, rows=(1, 2), **kw)
            launch_and_check(vct, oracle, ctx, s, what + " rate 2", form, rate=2, full=full, **kw)


@pytest.mark.parametrize("wrap", [1, 0])
def test_everything_at_once(vct, oracle, wrap):
    """Sky + a three-class checkerboard + emission planes + a point and a spot light, at rate 1 and at rate 2; then with one
    light and with the full table of 64."""
    s = scene(oracle, "dense32")
    with context(vct, s, wrap_repeat=wrap) as ctx:
        for lights, tag in ((TWO_LIGHTS, "point + spot"), (ONE_LIGHT, "1 light"), (lr.many_lights(), "64 lights")):
            kw = everything(s, lights=lights)
            full, ref = launch_and_check(vct, oracle, ctx, s, f"everything, {tag}, wrap={wrap}, rate 1", PRODUCT, **kw)
            launch_and_check(vct, oracle, ctx, s, f"everything, {tag}, wrap={wrap}, rate 2", PRODUCT, rate=2, full=full.copy(), **kw)
        plain, _ = launch_and_check(vct, oracle, ctx, s, "everything detached again", PRODUCT)
        assert not np.array_equal(plain, full)


@pytest.mark.parametrize("mask", MASKS)
def test_everything_under_a_component_mask(vct, oracle, mask):
    s = scene(oracle, "thin32")
    with context(vct, s) as ctx:
        kw = everything(s, mask=mask)
        full, ref = launch_and_check(vct, oracle, ctx, s, f"mask {mask} rate 1", PRODUCT, **kw)
        dif, spc = cr.marched_groups(mask)
        assert ref["steps"][:, :6].any() == dif and ref["steps"][:, 6].any() == spc
        _, r2 = launch_and_check(vct, oracle, ctx, s, f"mask {mask} rate 2", PRODUCT, rate=2, full=full.copy(), **kw)
        assert r2["marched"].any() == dif


def test_everything_with_every_output_on(vct, oracle):
    s = scene(oracle, "dense32")
    with context(vct, s) as ctx:
        kw = everything(s, aov=ALL_AOV)
        full, _ = launch_and_check(vct, oracle, ctx, s, "outputs, rate 1", PRODUCT, **kw)
        launch_and_check(vct, oracle, ctx, s, "outputs, rate 2", PRODUCT, rate=2, full=full.copy(), **kw)
        # (nothing this mask shows reads a cone: the outputs alone have both groups marched)
        launch_and_check(vct, oracle, ctx, s, "outputs under a mask", PRODUCT, mask=MASKS[0], **kw)


def test_strided_rows(vct, oracle):
    """vct_trace_resident_strided: every second tile row, both phases, over another frame's rows."""
    s = scene(oracle, "thin16")
    ty = s["ty"]
    with context(vct, s) as ctx:
        kw = everything(s)
        launch_and_check(vct, oracle, ctx, s, "whole frame first", **kw)
        for first in (0, 1):
            ctx.set_sky(-sr.SH)
            ctx.trace(s["planes"])                        # another frame in every row, other lit planes too
            ctx.set_sky(sr.SH)

            def strided():
                ctx.trace_gbuffer_strided(first, ty, 2)
                return ctx.download_frame()
            launch_and_check(vct, oracle, ctx, s, f"rows {first}, {first + 2}, ..", launch=strided, set_state=False,
                             rows=(first, ty), row_stride=2, **kw)


def test_slot_1_of_two(vct, oracle):
    """Two frame slots (which refuse the debug outputs): slot 1 with everything, slot 0 with other planes in between."""
    s = scene(oracle, "dense32")
    with context(vct, s, debug=0) as ctx:
        ctx.set_frames_in_flight(2)
        ctx.select_frame_slot(1)
        kw = everything(s, aov=ALL_AOV)
        full, _ = launch_and_check(vct, oracle, ctx, s, "slot 1, rate 1", PRODUCT, **kw)
        full = full.copy()
        ctx.select_frame_slot(0)                          # slot 0: its own planes, another frame
        ctx.set_pixel_emission(s["E"][::-1].copy())
        ctx.set_pixel_gloss(np.zeros(s["w"] * s["h"], np.uint8))
        ctx.trace(s["planes"])
        ctx.select_frame_slot(1)
        assert np.array_equal(ctx.download_frame().reshape(-1, 4), full)
        launch_and_check(vct, oracle, ctx, s, "slot 1, rate 2", PRODUCT, rate=2, full=full, **kw)
        ctx.select_frame_slot(0)
        other, _ = launch_and_check(vct, oracle, ctx, s, "slot 0 afterwards", PRODUCT, **everything(s, emission=s["E"][::-1].copy()))
        assert not np.array_equal(other, full)


def test_after_an_import_with_material_ids(vct, oracle):
    """vct_import_gbuffer with material ids fills the slot's emission and gloss planes from the material tables: the frame of
    what it wrote, at both rates."""
    s = scene(oracle, "thin32")
    w, h, g = s["w"], s["h"], s["planes"]
    npix, nmat = w * h, 4
    r = np.random.default_rng(12)
    emission = r.uniform(0.0, 2.0, (nmat, 3)).astype(f32)
    mat_class = np.array([2, 0, 1, 200], np.uint8)
    material = r.integers(0, nmat + 2, npix).astype(np.uint16)
    spec = np.zeros((npix, 4), f32)
    spec[:, :3] = g[19:22].T
    inputs = dict(position=np.ascontiguousarray(g[0:3].T), normal=np.ascontiguousarray(g[3:6].T),
                  shading_normal=np.ascontiguousarray(g[12:15].T), albedo=np.ascontiguousarray(g[15:19].T), specular=spec,
                  shadow=np.ascontiguousarray(g[22]), material=material)
    _, em, gl = ir.restate(w, h, emission=emission, mat_class=mat_class, normal_scale=0.05, albedo_format=ir.COLOR_F32X4,
                           specular_format=ir.COLOR_F32X4, **inputs)
    assert em.any() and len(np.unique(gr.clamp_class(gl, 3))) == 3 and (material >= nmat).any()
    with context(vct, s) as ctx:
        ctx.upload_triangles(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], f32), np.zeros(1, np.int32), np.ones((nmat, 4), f32))
        ctx.upload_chain(s["chain"])
        ctx.upload_emission(emission)
        ctx.set_gloss_classes(CLASSES)
        ctx.upload_material_gloss(mat_class)
        ctx.set_sky(sr.SH)
        ctx.set_lights(TWO_LIGHTS)
        ctx.import_gbuffer(normal_scale=0.05, **inputs)
        imported = ctx.download_gbuffer()
        assert np.array_equal(imported[0:3].view(np.uint32), g[0:3].view(np.uint32)) and np.array_equal(imported[18], g[18])
        assert np.array_equal(ctx.download_pixel_emission().view(np.uint32), em.view(np.uint32))
        assert np.array_equal(ctx.download_pixel_gloss(), gl)
        kw = dict(classes=CLASSES, gloss_plane=gl, sky=sr.SH, emission=em, lights=TWO_LIGHTS)
        full, _ = launch_and_check(vct, oracle, ctx, s, "imported, rate 1", PRODUCT, launch=ctx.trace_current, planes=imported,
                                   set_state=False, **kw)
        ctx.set_diffuse_rate(2)
        launch_and_check(vct, oracle, ctx, s, "imported, rate 2", PRODUCT, launch=ctx.trace_current, planes=imported,
                         set_state=False, rate=2, full=full.copy(), **kw)


@pytest.mark.parametrize("wrap", [1, 0])
def test_the_loose_half_aperture_on_the_ieee_divide(vct, oracle, wrap):
    """test_gpu_march_params.LOOSE_HALF as the diffuse aperture: a blend fraction below 2^-10 puts every march launch of the
    context -- the class tables' too -- on the IEEE divide."""
    s = scene(oracle, "thin16")
    with context(vct, s, wrap_repeat=wrap, tan_diffuse=LOOSE_HALF) as ctx:
        kw = everything(s)
        full, _ = launch_and_check(vct, oracle, ctx, s, f"loose half wrap={wrap} rate 1", IEEE, **kw)
        launch_and_check(vct, oracle, ctx, s, f"loose half wrap={wrap} rate 2", IEEE, rate=2, full=full.copy(), **kw)


def test_zz_every_reachable_form_was_reached():
    """Runs last in this module (pytest keeps the order of definition): the tests above have reached every instantiation the
    dispatch can select for these features, and nothing else."""
    assert {x for x in REACHED if x[0] == "k_trace_tile_split"} == SPLIT_FORMS
    assert {x for x in REACHED if x[0] == "k_point_march"} == POINT_FORMS
