"""The cone march away from the reference's constants: grid size, distance and opacity limits, apertures and the shading
constants (vct_config fields and setters), against the CPU oracle under the same parameters.

The march has two families of kernels.  vct_refresh_steps (csrc/vct_api_trace.hip) picks the verified two-term product for its
constant divisions only when every divisor passes the device's exhaustive check, 1 - max_alpha >= 2^-5 and every blend
fraction lies in [2^-10, 1 - 2^-10]; anything else runs the IEEE-divide instantiations (FASTDIV = 0).  Every test here
asserts which form ran (vct_get_stage_counts [2]), from a restatement of that rule.  Bars as in test_gpu_parity.py:
per-cone step counts and raw cone vec4s bit-equal, the RGBA16F frame within 1e-3 relative L2 with >= 99.9 % of the
halves equal, and the step total equal to the oracle's."""
import numpy as np
import pytest

import components_ref as cr
import synth
import vctpkg

pytestmark = pytest.mark.gpu

REL_L2_TOL = 1e-3
IEEE, PRODUCT = 1, 2                         # vct_get_stage_counts [2]
f32 = np.float32
V, W, H = 32, 60, 44                         # ragged: 8 x 6 tiles of 8 x 8
# grid sizes found once with selftest_const_divide on the MI355X: G / 2 of VERIFIED_G and the step divisors of its
# default tables pass the device check (a divisor outside the shipped table); G / 2 of REJECTED_G does not
VERIFIED_G = 100.0
REJECTED_G = 99.7
LOOSE_HALF = 0.5 * (1 + 2.0 ** -11)          # first step's blend fraction log2(1 + 2^-11) ~ 7e-4 < 2^-10
CONSTS = {"grid_world_size": "G", "max_distance": "max_distance", "max_alpha": "max_alpha",
          "tan_diffuse": "tan_diffuse", "tan_specular": "tan_specular", "shininess": "shininess",
          "ambient_factor": "ambient_factor", "wrap_repeat": "wrap_repeat"}
COMP_MASK = cr.SHOW_ALL & ~cr.SHOW_DIFFUSE    # a non-default mask that still marches both cone groups
ALL_AOV = cr.AOV_INDIRECT_DIFFUSE | cr.AOV_INDIRECT_SPECULAR | cr.AOV_DIRECT

# the FASTDIV = 0 launches vct_plan_launch can name (csrc/vct_trace_forms.h): (kernel, WRAP, template choice)
IEEE_TRACE_LAUNCHES = (
    {("k_trace_tile", wrap, coop) for wrap in (0, 1) for coop in (False, True)}
    | {("k_trace_tile_split", wrap, "COMPACT", False) for wrap in (0, 1)}
    | {("k_trace_tile_split", wrap, branch, comp) for wrap in (0, 1) for comp in (False, True)
       for branch in ("ANISO", "PRIO", "plain") + (("CELLS",) if wrap else ())})
IEEE_BOUNCE_LAUNCHES = {(k, wrap) for k in ("k_bounce_march", "k_bounce_bricks") for wrap in (0, 1)}
REACHED = set()


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


def make_ctx(vct, w=W, h=H, debug=1, **kw):
    return vct.Context(vct.default_config(voxel_dim=kw.pop("voxel_dim", V), width=w, height=h, debug_outputs=debug,
                                          **kw))


def params(oracle, ctx):
    cfg = ctx.current_config()
    return oracle.default_params(cfg.voxel_dim, **{o: getattr(cfg, k) for k, o in CONSTS.items()})


def gbuffer(G, w=W, h=H, seed=3, discard_frac=0.05):
    return synth.random_gbuffer(w * h, seed=seed, discard_frac=discard_frac, extent=0.45 * G)


def volume(seed=5, occupancy=0.12, Vd=V):
    return synth.noise_volume(Vd, seed=seed, occupancy=occupancy)


# ---- restatement of vct_refresh_steps / build_steps (csrc/vct_api_trace.hip) -------------------------------------------------
def step_table(Vd, G, tan, md):
    """[(dist, occlusion divisor, two levels, blend fraction, lod)] of one cone group, fp32 as build_steps."""
    vs = f32(G) / f32(Vd)
    maxl = f32(int(np.log2(Vd)))
    dist, out = vs, []
    while dist < f32(md):
        assert len(out) <= 4096
        diam = max(vs, f32(2.0) * f32(tan) * dist)
        lod = np.log2(diam / vs, dtype=f32)
        two, frac = False, f32(0)
        if lod > 0:
            lam = min(lod, maxl)
            frac = f32(lam - np.floor(lam))
            two = bool(frac != 0)
        out.append((dist, f32(1.0) + f32(0.03) * diam, two, frac, lod))
        dist = f32(dist + diam)
    return out


def structurally_ok(d):
    b = int(f32(d).view(np.uint32))
    e, m = (b >> 23) & 0xff, b & 0x7fffff
    return d > 0 and e != 0xff and m != 0x7fffff and 4 <= e <= 250


def expected_form(ctx):
    """IEEE unless every precondition of the verified product holds and the device check passes every divisor."""
    cfg = ctx.current_config()
    tables = [step_table(cfg.voxel_dim, cfg.grid_world_size, t, cfg.max_distance) for t in (cfg.tan_diffuse, cfg.tan_specular)]
    if f32(1.0) - f32(cfg.max_alpha) < f32(2.0 ** -5):
        return IEEE
    for st in tables[0] + tables[1]:
        if st[2] and not (st[3] >= f32(2.0 ** -10) and f32(1.0) - st[3] >= f32(2.0 ** -10)):
            return IEEE
    divs = {float(f32(cfg.grid_world_size) * f32(0.5))} | {float(st[1]) for st in tables[0] + tables[1]}
    for d in sorted(divs):
        if not structurally_ok(d) or ctx.selftest_const_divide(d) > 0:
            return IEEE
    return PRODUCT


def form_of(ctx):
    return ctx.stage_counts()["march_division"]


def launch_of(variant, wrap, aniso, cells, slab, comp):
    """Which instantiation vct_launch_trace dispatches to (csrc/vct_trace_forms.h vct_plan_launch), restated by hand."""
    if not aniso and variant in (1, 2):
        return ("k_trace_tile", wrap, variant == 2)
    if not aniso and variant == 4:
        return ("k_trace_tile_split", wrap, "COMPACT", False)
    branch = "ANISO" if aniso else "CELLS" if (wrap and cells) else "plain" if slab else "PRIO"
    return ("k_trace_tile_split", wrap, branch, comp)


def check(vct, oracle, ctx, chain, planes, form=None, rows=None, aniso=None, mask=None, cells=False):
    """One trace against the oracle (test_gpu_parity.check_frame's bars), the division form asserted; records the
    instantiation an IEEE-divide launch reached."""
    cfg = ctx.current_config()
    w, h = cfg.width, cfg.height
    p = params(oracle, ctx)
    if aniso is None:
        ref = oracle.trace(p, chain, planes, nthreads=8, want_cones=True)
    else:
        ref = oracle.trace_aniso(p, chain, aniso, planes, nthreads=8, want_cones=True)
    want_form = expected_form(ctx)
    if form is not None:
        assert want_form == form, "the restated rule disagrees with the case's intent"
    out = ctx.trace(planes, rows=rows)
    assert form_of(ctx) == want_form
    sel = np.ones(h * w, bool)
    if rows is not None:
        sel[:] = False
        sel[rows[0] * 8 * w: min(rows[1] * 8, h) * w] = True
    if cfg.debug_outputs:
        steps, cones = ctx.steps(), ctx.cones()
        assert np.array_equal(steps[sel], ref["steps"][sel]), "per-cone step counts differ"
        assert np.array_equal(cones[sel].view(np.uint32), ref["cones"][sel].view(np.uint32)), \
            "raw cone results are not bit-identical"
    want32 = ref["rgba32f"]
    want16 = ref["rgba16f"]
    if mask is not None:
        want32 = cr.composite(planes, cr.masked_cones(ref["cones"], mask, ALL_AOV), p.camera_pos[:], p.light_dir[:],
                              p.ambient_factor, p.shininess, mask)["rgba32f"]
        want16 = cr.to_f16_bits(want32)
        alive = planes[18] >= 0.5
        isp = ctx.download_aov(vct.AOV_INDIRECT_SPECULAR).reshape(-1, 4)
        assert np.array_equal(isp[alive & sel], cr.to_f16_bits(ref["cones"][:, 6, :])[alive & sel])
    got = vct.half_to_float(out.reshape(-1, 4))[sel]
    err = synth.rel_l2(got, want32[sel])
    assert err <= REL_L2_TOL, err
    same16 = (out.reshape(-1, 4)[sel] == want16[sel]).mean()
    assert same16 > 0.999, same16
    if rows is None:
        assert ctx.last_step_count() == ref["total_steps"]
    else:
        assert ctx.last_step_count() == int(ref["steps"][sel].astype(np.int64).sum())
    if want_form == IEEE:
        slab = rows is not None and (rows[1] - rows[0]) * 2 <= (h + 7) // 8
        REACHED.add(launch_of(cfg.trace_variant, cfg.wrap_repeat, aniso is not None, cells, slab, mask is not None))
    return ref, out


# ---- cases ----------------------------------------------------------------------------------------------------------
def test_control_defaults(vct, oracle):
    chain = oracle.build_mips(volume())
    with make_ctx(vct) as ctx:
        assert form_of(ctx) == 0                          # no march yet
        ctx.upload_chain(chain)
        check(vct, oracle, ctx, chain, gbuffer(150.0), form=PRODUCT)


@pytest.mark.parametrize("max_alpha,form", [(0.97, IEEE), (1.0, IEEE), (0.5, PRODUCT), (0.0, None)])
def test_max_alpha(vct, oracle, max_alpha, form):
    chain = oracle.build_mips(volume())
    planes = gbuffer(150.0)
    alive = planes[18] >= 0.5
    with make_ctx(vct, max_alpha=max_alpha) as ctx:
        ctx.upload_chain(chain)
        ref, _ = check(vct, oracle, ctx, chain, planes, form=form)
        nd = len(step_table(V, 150.0, 0.577, 75.0))
        ns = len(step_table(V, 150.0, 0.07, 75.0))
        steps = ctx.steps()
        assert (steps[:, :6] <= nd).all() and (steps[:, 6] <= ns).all()
        if max_alpha == 0.0:                              # alpha < 0 never holds: no step, zero cones
            assert not steps.any() and not ctx.cones().any() and ctx.last_step_count() == 0
        if max_alpha == 1.0:                              # a cone runs its table unless alpha reaches exactly 1
            assert (steps[alive, 6] == ns).mean() > 0.2
            assert (steps[alive] > 0).all()


def odd_even_apertures():
    """Specular apertures whose tables (V 32, G 150, distance 75) have an odd and an even length (the march loop is
    unrolled by two and alternates two register sets)."""
    p_len = {t: len(step_table(V, 150.0, t, 75.0)) for t in (0.07, 0.105, 0.2, 0.15, 0.3)}
    odd = next(t for t, n in p_len.items() if n % 2 == 1)
    even = next(t for t, n in p_len.items() if n % 2 == 0)
    return odd, even


@pytest.mark.parametrize("case", ["loose_half", "half", "two", "three", "odd", "even"])
def test_apertures(vct, oracle, case):
    odd, even = odd_even_apertures()
    tan = {"loose_half": LOOSE_HALF, "half": 0.5, "two": 2.0, "three": 3.0, "odd": odd, "even": even}[case]
    td, ts = (0.577, tan) if case in ("odd", "even") else (tan, tan)
    md = 150.0 if case in ("two", "three") else 75.0
    table = step_table(V, 150.0, ts, md)
    if case == "loose_half":
        assert table[0][2] and 0 < table[0][3] < 2.0 ** -10
    if case == "half":                                    # lod = log2(2^k): integer levels, one sample per step
        assert all(not st[2] for st in table) and all(float(st[4]).is_integer() for st in table)
    if case in ("two", "three"):                          # clamped at the top level within a few steps
        assert len(table) <= 4 and table[-1][4] > np.log2(V)
    if case in ("odd", "even"):
        assert len(table) % 2 == (1 if case == "odd" else 0)
    chain = oracle.build_mips(volume(seed=9))
    with make_ctx(vct, tan_diffuse=td, tan_specular=ts, max_distance=md) as ctx:
        ctx.upload_chain(chain)
        check(vct, oracle, ctx, chain, gbuffer(150.0, seed=4), form=IEEE if case == "loose_half" else None)


def test_grid_size_verified_at_run_time(vct, oracle):
    """A grid size outside the shipped divisor table whose divisors pass the device check: the verified product, and a
    second context (the process-wide verdict cache) gives the same frame."""
    G = VERIFIED_G
    chain = oracle.build_mips(volume())
    planes = gbuffer(G)
    frames = []
    for _ in range(2):
        with make_ctx(vct, grid_world_size=G, max_distance=G / 2) as ctx:
            ctx.upload_chain(chain)
            _, out = check(vct, oracle, ctx, chain, planes, form=PRODUCT)
            frames.append((out.copy(), ctx.cones().copy()))
    assert np.array_equal(frames[0][0], frames[1][0])
    assert np.array_equal(frames[0][1].view(np.uint32), frames[1][1].view(np.uint32))


def test_grid_size_rejected_by_the_device(vct, oracle):
    G = REJECTED_G
    chain = oracle.build_mips(volume())
    with make_ctx(vct, grid_world_size=G, max_distance=G / 2) as ctx:
        assert ctx.selftest_const_divide(G / 2) > 0
        ctx.upload_chain(chain)
        check(vct, oracle, ctx, chain, gbuffer(G), form=IEEE)


@pytest.mark.parametrize("G", [150.0, VERIFIED_G])
@pytest.mark.parametrize("which", ["at_voxel", "above_voxel", "four_grids"])
def test_max_distance(vct, oracle, G, which):
    vs = f32(G) / f32(V)
    md = {"at_voxel": float(vs), "above_voxel": float(np.nextafter(vs, f32(np.inf))), "four_grids": 4.0 * G}[which]
    chain = oracle.build_mips(volume(occupancy=0.04))
    planes = gbuffer(G)
    alive = planes[18] >= 0.5
    for wrap in ((0, 1) if which == "four_grids" else (1,)):
        with make_ctx(vct, grid_world_size=G, max_distance=md, wrap_repeat=wrap) as ctx:
            ctx.upload_chain(chain)
            check(vct, oracle, ctx, chain, planes)
            steps = ctx.steps()
            if which == "at_voxel":                       # both tables empty: the composite of zero cones
                assert not steps.any() and not ctx.cones().any()
            if which == "above_voxel":
                assert (steps[alive] == 1).all() and not steps[~alive].any()
            if which == "four_grids":
                assert steps[alive, 6].max() > len(step_table(V, G, 0.07, G / 2))


@pytest.mark.parametrize("shininess,ambient", [(0.0, 0.1), (1.0, 0.1), (200.0, 0.1), (20.0, 0.5)])
def test_shading_constants(vct, oracle, shininess, ambient):
    chain = oracle.build_mips(volume())
    planes = gbuffer(150.0, discard_frac=0.1)
    dead = planes[18] < 0.5
    with make_ctx(vct, shininess=shininess) as ctx:
        ctx.set_ambient_factor(ambient)
        ctx.upload_chain(chain)
        _, out = check(vct, oracle, ctx, chain, planes, form=PRODUCT)
        clear = vct.half_to_float(out.reshape(-1, 4))[dead]
        assert (clear[:, :3] == (1.0 if ambient >= 0.5 else 0.5)).all() and (clear[:, 3] == 1.0).all()   # VCT.h:156-159


IEEE_CASES = {"max_alpha": dict(max_alpha=0.97), "loose_half": dict(tan_diffuse=LOOSE_HALF, tan_specular=LOOSE_HALF),
              "rejected_G": dict(grid_world_size=REJECTED_G, max_distance=REJECTED_G / 2)}


def test_ieee_instantiation_sweep(vct, oracle):
    """Every IEEE-divide trace instantiation (both wrap modes; trace variants 1, 2, 4; whole frame and slab; footprint
    records; anisotropic mips; lighting components with outputs) against the oracle, each under every IEEE case."""
    l0 = volume(seed=11)
    chain = oracle.build_mips(l0)
    aniso = oracle.build_mips_aniso(l0)
    REACHED.difference_update({x for x in REACHED if x[0].startswith("k_trace")})
    for name, consts in IEEE_CASES.items():
        planes = gbuffer(consts.get("grid_world_size", 150.0), seed=7)
        for wrap in (0, 1):
            with make_ctx(vct, wrap_repeat=wrap, **consts) as ctx:
                ctx.upload_chain(chain)
                for comp in (False, True):
                    if comp:
                        ctx.set_lighting_components(COMP_MASK)
                        ctx.set_aov_outputs(ALL_AOV)
                    mask = COMP_MASK if comp else None
                    check(vct, oracle, ctx, chain, planes, form=IEEE, mask=mask)                     # PRIO
                    check(vct, oracle, ctx, chain, planes, form=IEEE, mask=mask, rows=(1, 4))        # plain
                    ctx.set_footprint_records(True)
                    check(vct, oracle, ctx, chain, planes, form=IEEE, mask=mask, cells=True)         # CELLS / PRIO
                    ctx.set_footprint_records(False)
                ctx.set_lighting_components(cr.SHOW_ALL)
                ctx.set_aov_outputs(0)
                for variant in (1, 2, 4):
                    ctx.set_trace_variant(variant)
                    check(vct, oracle, ctx, chain, planes, form=IEEE)
                ctx.set_trace_variant(0)
            with make_ctx(vct, wrap_repeat=wrap, anisotropic_mips=1, **consts) as ctx:
                ctx.upload_volume(l0)
                ctx.build_mips()
                assert np.array_equal(ctx.download_aniso(), aniso)
                check(vct, oracle, ctx, chain, planes, form=IEEE, aniso=aniso)
                ctx.set_lighting_components(COMP_MASK)
                ctx.set_aov_outputs(ALL_AOV)
                check(vct, oracle, ctx, chain, planes, form=IEEE, aniso=aniso, mask=COMP_MASK)
    assert {x for x in REACHED if x[0].startswith("k_trace")} == IEEE_TRACE_LAUNCHES


def random_scene(ntri, seed):
    r = np.random.default_rng(seed)
    c = r.uniform(-1300, 1300, (ntri, 1, 3))
    pos = c + r.normal(scale=25.0, size=(ntri, 3, 3))
    pos[0] = [[-1000, -1000, 200], [1000, -1000, 200], [1000, 1000, 200]]
    mat = r.integers(0, 5, ntri).astype(np.int32)
    alb = r.uniform(0.1, 1.0, (5, 4)).astype(np.float32)
    return pos.astype(np.float32), mat, alb


@pytest.mark.parametrize("wrap,max_alpha,form", [(0, 0.97, IEEE), (1, 0.97, IEEE), (1, 0.95, None)])
def test_bounce(vct, oracle, wrap, max_alpha, form):
    """The second bounce under a non-table diffuse aperture: bounce-1 level 0 and its chain bit-equal to the oracle's."""
    Vb, tan = 32, 0.3
    pos, mat, alb = random_scene(300, seed=33)
    with make_ctx(vct, 16, 8, voxel_dim=Vb, voxel_attributes=1, wrap_repeat=wrap, max_alpha=max_alpha,
                  tan_diffuse=tan) as ctx:
        p = params(oracle, ctx)
        sc = oracle.make_scene(pos, mat, alb)
        l0, want_alb, want_nrm = oracle.voxelize_conservative_attr(p, sc)
        chain0 = oracle.build_mips(l0)
        want_l1, want_steps = oracle.bounce(p, chain0, want_alb, want_nrm, nthreads=8)
        assert (want_l1 != l0).any() and want_steps > 0
        want_form = expected_form(ctx)
        if form is not None:
            assert want_form == form
        ctx.upload_triangles(pos, mat, alb)
        ctx.voxelize()
        ctx.inject_light()
        ctx.build_mips()
        assert np.array_equal(ctx.download_chain(), chain0)
        ctx.bounce()
        assert form_of(ctx) == want_form
        assert ctx.last_step_count() == want_steps
        assert np.array_equal(ctx.download_chain(), oracle.build_mips(want_l1))
        if want_form == IEEE:
            REACHED.update({("k_bounce_march", wrap), ("k_bounce_bricks", wrap)})
    if (wrap, max_alpha) == (1, 0.97):
        assert {x for x in REACHED if x[0].startswith("k_bounce")} == IEEE_BOUNCE_LAUNCHES


def test_switching_apertures_on_one_context(vct, oracle):
    """Default apertures -> an IEEE-form aperture -> back: each frame equals a fresh context's, the form follows."""
    chain = oracle.build_mips(volume())
    planes = gbuffer(150.0)
    fresh = {}
    for td in (0.577, LOOSE_HALF):
        with make_ctx(vct, tan_diffuse=td) as ctx:
            ctx.upload_chain(chain)
            _, out = check(vct, oracle, ctx, chain, planes)
            fresh[td] = (out.copy(), ctx.cones().copy(), form_of(ctx))
    assert fresh[0.577][2] == PRODUCT and fresh[LOOSE_HALF][2] == IEEE
    with make_ctx(vct) as ctx:
        ctx.upload_chain(chain)
        for td in (0.577, LOOSE_HALF, 0.577):
            ctx.set_cone_apertures(td, 0.07)
            out = ctx.trace(planes)
            assert form_of(ctx) == fresh[td][2]
            assert np.array_equal(out, fresh[td][0])
            assert np.array_equal(ctx.cones().view(np.uint32), fresh[td][1].view(np.uint32))


def aperture_for_steps(n, md, Vd=V, G=150.0):
    """Specular apertures (n steps, n + 1 steps) at max_distance md, by bisection on the aperture with the step loop
    (the oracle's max_steps is checked against it)."""
    lo, hi = 1e-7, 1.0                                     # lo: more than n steps, hi: fewer
    assert len(step_table(Vd, G, lo, md)) > n >= len(step_table(Vd, G, hi, md))
    for _ in range(200):
        mid = float(f32((lo + hi) / 2))
        if mid in (lo, hi):
            break
        if len(step_table(Vd, G, mid, md)) > n:
            lo = mid
        else:
            hi = mid
    assert len(step_table(Vd, G, hi, md)) == n and len(step_table(Vd, G, lo, md)) == n + 1, (lo, hi)
    return hi, lo


@pytest.mark.parametrize("debug,limit", [(1, 255), (0, 1024)])
def test_step_table_limits(vct, oracle, debug, limit):
    """debug_outputs keeps per-cone counts as bytes: 255 steps are traced exactly, 256 refused.  Without them the table
    holds VCT_MAX_STEPS = 1024 entries: 1024 are traced exactly, 1025 refused.  After a refusal a valid aperture
    gives the earlier frame back bit for bit."""
    vs = f32(150.0) / f32(V)
    md = float(vs * f32(limit + 1) + vs * f32(0.5))        # a vanishing aperture takes limit + 1 steps of one voxel
    ok_tan, over_tan = aperture_for_steps(limit, md)
    l0 = volume(occupancy=0.1)
    l0[..., 3] //= 64                                      # faint voxels: cones live for hundreds of steps
    chain = oracle.build_mips(l0)
    w, h = 24, 16
    planes = gbuffer(150.0, w, h)
    with make_ctx(vct, w, h, debug=debug, max_distance=md, tan_specular=ok_tan) as ctx:
        p = params(oracle, ctx)
        assert oracle.max_steps(p, ok_tan)[0] == limit and oracle.max_steps(p, over_tan)[0] == limit + 1
        ctx.upload_chain(chain)
        ref, out = check(vct, oracle, ctx, chain, planes, rows=None)
        out = out.copy()
        if debug:
            assert ctx.steps()[:, 6].max() == limit
        else:
            assert ref["total_steps"] > 255 * w * h / 2          # many cones longer than a byte counts
        ctx.set_cone_apertures(0.577, over_tan)
        with pytest.raises(vct.VctError):
            ctx.trace(planes)
        ctx.set_cone_apertures(0.577, ok_tan)
        assert np.array_equal(ctx.trace(planes), out)
        assert ctx.last_step_count() == ref["total_steps"]


def test_create_applies_the_setters_checks(vct):
    """vct_create refuses the config values the setters refuse."""
    for kw in (dict(tan_diffuse=0.0), dict(tan_specular=-0.1), dict(tan_diffuse=float("nan")), dict(trace_variant=5),
               dict(trace_variant=-1)):
        with pytest.raises(vct.VctError):
            make_ctx(vct, **kw)
