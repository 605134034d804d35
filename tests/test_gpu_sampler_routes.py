"""GPU: the routes of the block-reuse sampler of the default trace kernel (csrc/vct_trace.hip sample_level_reuse).

A level sample is served in one of five ways -- by the block the wave holds in its second slab, by that block known to be
all zero, by a fresh cooperative block, by a fresh block that turns out all zero, or per lane -- and the sampler reaches
each by wave-uniform branches.  Every case here builds, at the smallest shapes at which the route can go wrong, an input
on which one of the routes is taken (stated in its docstring) and compares HIP with the CPU oracle bit for bit, with debug
outputs on: per-cone step counts, raw cone vec4s, last_step_count and last_row_steps; the RGBA16F frame inside the parity
bars and byte for byte against the one-wave-per-tile kernel (config.trace_variant 1), which samples without reuse -- the
way tests/test_gpu_block_reuse.py::check does.

Which route a sample takes cannot be seen from a release build.  CASES below is the registry of the inputs: the
instrumented build (-DVCT_STATS=1, Context.last_trace_stats, as tools/trace_stats.py reads it) run over the same CASES
shows the counter of each intended route non-zero (profiles/experiments/r18_sampler_routing_ab.txt has the table).

Frames are 64 x 16 to 64 x 24 pixels (16 to 24 tiles), volumes 16^3 and 32^3; a case is an oracle trace of a thousand
pixels and two or three launches."""
import os

import numpy as np
import pytest

import components_ref as cr
import diffuse_rate_ref as drr
import gbcases as gc
import synth
import vctpkg

pytestmark = pytest.mark.gpu

f32 = np.float32
REL_L2_TOL = 1e-3          # tests/test_gpu_parity.py
CONSTS = {"grid_world_size": "G", "max_distance": "max_distance", "max_alpha": "max_alpha", "tan_diffuse": "tan_diffuse",
          "tan_specular": "tan_specular", "shininess": "shininess", "ambient_factor": "ambient_factor",
          "wrap_repeat": "wrap_repeat"}
CAM, LIGHT = gc.CAM, gc.LIGHT
CAM_ABOVE = (10.0, 140.0, -5.0)      # above the floor patch: the specular cone goes up, with the diffuse ones
W = 64


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


def make_ctx(vct, V, w, h, level_form=False, debug=1, **kw):
    """A context with debug outputs; level_form: created under VCT_LEVEL_DESCRIPTORS=1 (read at vct_create), which takes
    the kernels that form a resource per level and fetch instead of the chain's."""
    old = os.environ.pop("VCT_LEVEL_DESCRIPTORS", None)
    if level_form:
        os.environ["VCT_LEVEL_DESCRIPTORS"] = "1"
    try:
        ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, debug_outputs=debug, **kw))
    finally:
        os.environ.pop("VCT_LEVEL_DESCRIPTORS", None)
        if old is not None:
            os.environ["VCT_LEVEL_DESCRIPTORS"] = old
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    return ctx


# ---- volumes and G-buffers ------------------------------------------------------------------------------------------------------
def floor(w, h, V, plane_y=-20.0, tile_voxels=1.0, seed=3):
    """A coherent floor patch on which an 8x8 tile is `tile_voxels` voxels wide (150 world units across V voxels)."""
    extent = 0.5 * tile_voxels * (150.0 / V) * max(w, h) / 8.0
    return synth.coherent_gbuffer(w, h, seed=seed, plane_y=plane_y, extent=extent)


def thin_shell(V, seed=7):
    return synth.noise_volume(V, seed=seed, occupancy=0.08)


def dense(V, seed=5):
    """Random colours, every other voxel opaque and the rest empty (tests/test_gpu_block_reuse.py)."""
    r = np.random.default_rng(seed)
    l0 = r.integers(0, 256, (V, V, V, 4), dtype=np.uint8)
    l0[..., 3] = np.where(r.uniform(size=(V, V, V)) < 0.5, 255, 0)
    return l0


def faint(V, seed=2, divisor=16):
    """Every voxel occupied, nearly transparent: every cone runs its table out."""
    return np.random.default_rng(seed).integers(0, 256, (V, V, V, 4), dtype=np.uint8) // np.uint8(divisor)


def layers(V, first_filled, thick=4, seed=6):
    """Horizontal layers `thick` voxels high, in turn faint and empty, the layer that holds the floor patch (y = -20: voxel
    row 0.367 V) faint or empty by `first_filled`: a cone that climbs meets all-zero blocks, then filled ones, then
    all-zero ones again at the same level -- or the other way round."""
    l0 = faint(V, seed=seed, divisor=8)
    y0 = int((-20.0 + 75.0) / 150.0 * V)
    for y in range(V):
        filled = (((y - y0) // thick) % 2 == 0) == bool(first_filled)
        if not filled:
            l0[:, y] = 0
    return l0


def with_random_rows(planes, w, h, rows=(6, 7), seed=9):
    """`planes` with the pixel rows `rows` of every tile row replaced by independent random pixels: the tile's sample is a
    per-lane one while any of their lanes lives and a cooperative one once they have ended."""
    rnd = synth.random_gbuffer(w * h, seed=seed, extent=40.0)
    out = planes.copy()
    sel = np.isin(np.arange(h) % 8, rows).repeat(w)
    out[:, sel] = rnd[:, sel]
    return out


def live_lane_shapes(planes, w, h):
    """Tile 0: lane 27 discarded (the anchor comes from the first live lane).  Tile 1: one live pixel.  Tile 2: none."""
    out = planes.copy()
    alpha = out[18].reshape(h, w)
    alpha[3, 3] = 0.0                                # lane 27 of tile 0 = pixel (x 3, y 3)
    alpha[0:8, 8:16] = 0.0
    alpha[5, 13] = 1.0
    alpha[0:8, 16:24] = 0.0
    return out


# name -> (V, h, volume, planes, config kw, camera): the registry the instrumented build is run over as well
def _cases():
    c = {}
    # the diffuse cones' first level is the second level of the step before: served by the held block, which is filled
    c["held_filled"] = (32, 16, dense(32), floor(W, 16, 32), {}, None)
    # a narrow specular cone stays on one pair of levels through the empty inside of the shell: the held block is all zero
    c["held_zero"] = (32, 16, thin_shell(32, seed=12), floor(W, 16, 32, tile_voxels=0.5), dict(tan_specular=0.07), CAM_ABOVE)
    # a tile 2.5 voxels wide: the held block of the right level no longer holds every footprint, a block at the new anchor does
    c["misfit_then_fresh"] = (32, 16, faint(32, seed=8, divisor=4), floor(W, 16, 32, tile_voxels=2.5), dict(tan_specular=0.07), CAM_ABOVE)
    # fresh all-zero blocks of both slabs followed, same level, by filled ones (zero bit written 0, then 1) ...
    c["zero_then_filled"] = (32, 16, layers(32, first_filled=False), floor(W, 16, 32, tile_voxels=0.5), dict(tan_specular=0.07), CAM_ABOVE)
    # ... and filled ones followed by all-zero ones (1, then 0)
    c["filled_then_zero"] = (32, 16, layers(32, first_filled=True), floor(W, 16, 32, tile_voxels=0.5), dict(tan_specular=0.07), CAM_ABOVE)
    # per-lane samples while the random rows live, cooperative and held ones beside them and after them
    c["per_lane_between"] = (32, 16, thin_shell(32, seed=9), with_random_rows(floor(W, 16, 32), W, 16), {}, None)
    # 16^3 and twice the march distance: the last steps sample the levels of 4, 2 and 1 texels, whose block wraps onto
    # itself; the floor 1.5 voxels under the grid's top face, so that every cone crosses the GL_REPEAT seam
    c["coarsest_levels_seam"] = (16, 16, faint(16), floor(W, 16, 16, plane_y=75.0 - 1.5 * 150.0 / 16), dict(max_distance=150.0), CAM_ABOVE)
    c["live_lane_shapes"] = (32, 16, thin_shell(32, seed=9), live_lane_shapes(floor(W, 16, 32), W, 16), {}, None)
    return c


CASES = _cases()


def row_steps(ref_steps, w, h):
    per_pixel_row = ref_steps.astype(np.int64).sum(axis=1).reshape(h, w).sum(axis=1)
    return np.array([per_pixel_row[r:r + 8].sum() for r in range(0, h, 8)], np.uint64)


def oracle_params(oracle, ctx, cam):
    cfg = ctx.current_config()
    kw = {o: getattr(cfg, k) for k, o in CONSTS.items()}
    return oracle.default_params(cfg.voxel_dim, camera_pos=CAM if cam is None else cam, light_dir=LIGHT, **kw)


def assert_cones(ctx, ref, sel=slice(None)):
    assert np.array_equal(ctx.steps()[sel], ref["steps"][sel]), "per-cone step counts differ"
    assert np.array_equal(ctx.cones()[sel].view(np.uint32), ref["cones"][sel].view(np.uint32)), "raw cone results are not bit-identical"


def check(vct, oracle, ctx, chain, planes, w, h, cam=None):
    """One whole-frame trace against the oracle and the kernel without reuse; returns (oracle result, frame)."""
    if cam is not None:
        ctx.set_camera_position(cam)
    ref = oracle.trace(oracle_params(oracle, ctx, cam), chain, planes, nthreads=8, want_cones=True)
    out = ctx.trace(planes).copy()
    assert_cones(ctx, ref)
    assert ctx.last_step_count() == ref["total_steps"]
    assert np.array_equal(ctx.last_row_steps(), row_steps(ref["steps"], w, h))
    err = synth.rel_l2(vct.half_to_float(out.reshape(-1, 4)), ref["rgba32f"])
    assert err <= REL_L2_TOL, err
    assert (out.reshape(-1, 4) == ref["rgba16f"]).mean() > 0.999
    ctx.set_trace_variant(1)                     # one wave per tile, no reuse: the same frame, bit for bit
    try:
        assert np.array_equal(ctx.trace(planes), out), "frame differs from the kernel without reuse"
    finally:
        ctx.set_trace_variant(0)
    return ref, out


def run_case(vct, oracle, name):
    V, h, l0, planes, kw, cam = CASES[name]
    chain = oracle.build_mips(l0)
    with make_ctx(vct, V, W, h, **kw) as ctx:
        ctx.upload_chain(chain)
        return check(vct, oracle, ctx, chain, planes, W, h, cam=cam)[0]


# ---- one case per route ---------------------------------------------------------------------------------------------------------
def test_held_block_serves_a_filled_sample(vct, oracle):
    """Route: served by the held block, block filled.  Diffuse cones over a dense volume: the first level of a step is the
    second level of the step before, one or two texels on (counters reuse_hits_diffuse_first, coop_hit)."""
    ref = run_case(vct, oracle, "held_filled")
    assert ref["steps"][:, :6].max() >= 2                      # a second step exists whose first level was held


def test_held_block_known_all_zero(vct, oracle):
    """Route: served by the held block, known all zero.  A narrow specular cone walks through the empty inside of a thin
    shell on one pair of levels (reuse_hits_zero_specular_*)."""
    ref = run_case(vct, oracle, "held_zero")
    assert ref["steps"][:, 6].max() > 8


def test_candidate_does_not_fit_then_fresh_block(vct, oracle):
    """Route: a held block of the sample's level that does not hold every live footprint, then a fresh block that does.  A
    floor patch whose tiles are 2.5 voxels wide: footprints drift past the block's three origins per axis from one step
    to the next (reuse_candidates_* above reuse_hits_*, coop_hit)."""
    run_case(vct, oracle, "misfit_then_fresh")


@pytest.mark.parametrize("order", ["zero_then_filled", "filled_then_zero"])
def test_fresh_zero_and_filled_blocks_of_one_level(vct, oracle, order):
    """Route: fresh block all zero, in slab 0 and in slab 1, and a fresh filled block of the same level behind it -- the
    descriptor's zero bit is written 0 and then 1 -- and the other way round.  Horizontal faint and empty layers four
    voxels high, cones that climb through them (coop_zero, coop_hit, reuse_hits_zero_*)."""
    ref = run_case(vct, oracle, order)
    assert ref["steps"][:, 6].max() > 8                        # through several layers


def test_per_lane_sample_between_held_ones(vct, oracle):
    """Route: per lane, which must leave slab and descriptor alone.  Two pixel rows of every tile are independent random
    pixels, the other six a coherent floor: the tile's samples are per-lane ones while a random lane lives at that cone,
    cooperative and held ones at the other cones and steps (fallback beside reuse_hits_*)."""
    run_case(vct, oracle, "per_lane_between")


def test_levels_of_four_two_and_one_texels_across_the_seam(vct, oracle):
    """Every route's block at the levels whose 4x4x4 block wraps onto itself, anchors below 0 and past N - 1: 16^3, twice the
    march distance, the floor 1.5 voxels under the top face."""
    ref = run_case(vct, oracle, "coarsest_levels_seam")
    assert (ref["steps"][:, :6] >= 4).all()                    # diffuse steps at LOD 0.2, 1.3, 2.4, 3.5: levels 0 ... 4


def test_live_lane_shapes(vct, oracle):
    """A tile whose lane 27 is discarded (anchor from the first live lane), a tile with one live pixel (every sample
    cooperative: its own anchor), a tile with none (no wave marches)."""
    ref = run_case(vct, oracle, "live_lane_shapes")
    tile = ref["steps"].reshape(16, W, 7)
    assert not tile[0:8, 16:24].any() and tile[5, 13].any() and not tile[3, 3].any()


# ---- launch forms that instantiate the path differently -----------------------------------------------------------------------
FORMS_V, FORMS_H = 32, 24


@pytest.fixture(scope="module")
def forms(oracle):
    """(chain, planes, oracle trace) shared by the launch forms, left unchanged: a thin shell under a floor patch with two
    random pixel rows per tile row -- held, fresh, all-zero and per-lane samples in one frame."""
    chain = oracle.build_mips(thin_shell(FORMS_V, seed=14))
    planes = with_random_rows(floor(W, FORMS_H, FORMS_V), W, FORMS_H)
    planes[18, np.random.default_rng(4).uniform(size=W * FORMS_H) < 0.1] = 0.0
    p = oracle.default_params(FORMS_V, camera_pos=CAM, light_dir=LIGHT)
    return chain, planes, oracle.trace(p, chain, planes, nthreads=8, want_cones=True)


def test_whole_frame(vct, oracle, forms):
    """PRIO: the whole-frame launch, against the oracle and the kernel without reuse."""
    chain, planes, ref = forms
    with make_ctx(vct, FORMS_V, W, FORMS_H) as ctx:
        ctx.upload_chain(chain)
        got, _ = check(vct, oracle, ctx, chain, planes, W, FORMS_H)
        assert np.array_equal(got["steps"], ref["steps"])


def test_row_subset(vct, forms):
    """No PRIO: launches of one tile row of three (trace_gbuffer_rows) give the whole frame's rows, cones and steps."""
    chain, planes, ref = forms
    per_row = row_steps(ref["steps"], W, FORMS_H)
    with make_ctx(vct, FORMS_V, W, FORMS_H) as ctx:
        ctx.upload_chain(chain)
        full = ctx.trace(planes).copy()
        for r in range(3):
            ctx.trace_gbuffer_rows(r, r + 1)
            ctx.synchronize()
            assert ctx.last_step_count() == per_row[r]
            assert np.array_equal(ctx.download_frame()[r * 8:r * 8 + 8], full[r * 8:r * 8 + 8])
            assert_cones(ctx, ref, slice(r * 8 * W, (r + 1) * 8 * W))


def test_lighting_mask(vct, forms):
    """COMP: a non-default lighting mask marches the specular group alone."""
    chain, planes, ref = forms
    mask = cr.SHOW_SPECULAR | cr.SHOW_INDIRECT_SPECULAR
    with make_ctx(vct, FORMS_V, W, FORMS_H) as ctx:
        ctx.upload_chain(chain)
        ctx.set_lighting_components(mask)
        ctx.trace(planes)
        want = cr.masked_cones(ref["cones"], mask)
        assert np.array_equal(ctx.cones().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(ctx.steps()[:, 6], ref["steps"][:, 6]) and not ctx.steps()[:, :6].any()


def test_half_rate(vct, forms):
    """HALF: set_diffuse_rate(2) -- the pixels that march their own diffuse cones get the full-rate cones and pixels."""
    chain, planes, ref = forms
    r2 = drr.restate(planes, W, FORMS_H, f32(150.0) / f32(FORMS_V), ref, CAM, LIGHT)
    marched = r2["cls"]["marched"]
    assert 0 < marched.sum() < (planes[18] >= 0.5).sum()
    with make_ctx(vct, FORMS_V, W, FORMS_H) as ctx:
        ctx.upload_chain(chain)
        full = ctx.trace(planes).reshape(-1, 4).copy()
        ctx.set_diffuse_rate(2)
        got = ctx.trace(planes)
        assert np.array_equal(ctx.steps(), r2["steps"]) and ctx.last_step_count() == r2["total_steps"]
        assert np.array_equal(ctx.cones().view(np.uint32), r2["cones"].view(np.uint32))
        assert np.array_equal(got.reshape(-1, 4)[marched], full[marched])


def test_level_descriptor_form(vct, forms):
    """No CHAIN: a context created under VCT_LEVEL_DESCRIPTORS=1; the frame is the chain form's, byte for byte."""
    chain, planes, ref = forms
    with make_ctx(vct, FORMS_V, W, FORMS_H) as ctx:
        ctx.upload_chain(chain)
        want = ctx.trace(planes).copy()
    with make_ctx(vct, FORMS_V, W, FORMS_H, level_form=True) as ctx:
        ctx.upload_chain(chain)
        got = ctx.trace(planes)
        assert_cones(ctx, ref)
        assert ctx.last_step_count() == ref["total_steps"]
        assert np.array_equal(got, want)


def test_both_slots(vct, forms):
    """Both slots of a two-slot context (which refuses the debug outputs) trace the frame, slot 1 first: the one-slot
    context's frame, which test_whole_frame compares with the oracle, byte for byte, and its step count."""
    chain, planes, ref = forms
    with make_ctx(vct, FORMS_V, W, FORMS_H) as ctx:
        ctx.upload_chain(chain)
        want = ctx.trace(planes).copy()
        assert_cones(ctx, ref)
    with make_ctx(vct, FORMS_V, W, FORMS_H, debug=0) as ctx:
        ctx.upload_chain(chain)
        ctx.set_frames_in_flight(2)
        try:
            for slot in (1, 0, 1):
                ctx.select_frame_slot(slot)
                assert np.array_equal(ctx.trace(planes), want), slot
                assert ctx.last_step_count() == ref["total_steps"]
        finally:
            ctx.select_frame_slot(0)
