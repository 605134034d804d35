"""GPU: block reuse in the default trace kernel (csrc/vct_trace.hip BlockDesc) -- a cooperative level sample whose live
footprints all lie inside a 4x4x4 block that the wave already holds in LDS gathers from it instead of fetching a block.

Every case compares HIP with the CPU oracle the way tests/test_gpu_parity.py does, with debug outputs on: per-cone step
counts and raw cone vec4s bit for bit, last_step_count and last_row_steps, the frame inside the parity bars.  Bit for bit,
the frame is compared with the frame of the one-wave-per-tile kernel (config.trace_variant 1), which samples without
reuse and composites the same way: a frame is a function of the cones, and the oracle's own frame differs from any GPU
frame by an ulp of powf in a few pixels.

The frames are coherent (synth.coherent_gbuffer with an `extent` at which an 8x8 tile spans about one voxel), so that the
samples are cooperative and consecutive steps find the previous step's block; the shapes are the ones at which the path
can go wrong: all-zero blocks followed by filled ones, lanes that end at different steps, the grid face under GL_REPEAT
and under clamp (where reuse is off), levels of 4, 2 and 1 texels, a changing anchor lane, long runs on one pair of
levels, the instantiations without issue priority and with lighting components, and two launches in a row.

No test here can assert that a sample took the reuse path: only the instrumented build's counters show that
(tools/trace_stats.py; profiles/r07_reuse_stats.json).  What the tests assert is that the kernels with the path give the
oracle's bits on inputs built so that it is taken.  Reuse is instantiated for GL_REPEAT only, so the clamp case of
test_grid_face runs the unchanged sampler: it is there to keep that so."""
import numpy as np
import pytest

import components_ref as cr
import synth
import vctpkg

pytestmark = pytest.mark.gpu

REL_L2_TOL = 1e-3          # tests/test_gpu_parity.py
CONSTS = {"grid_world_size": "G", "max_distance": "max_distance", "max_alpha": "max_alpha", "tan_diffuse": "tan_diffuse",
          "tan_specular": "tan_specular", "shininess": "shininess", "ambient_factor": "ambient_factor",
          "wrap_repeat": "wrap_repeat"}
CAM_ABOVE = (10.0, 140.0, -5.0)      # above the floor patch: the specular cone goes up, with the diffuse ones


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


def make_ctx(vct, V, w, h, **kw):
    return vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, debug_outputs=1, **kw))


def floor(w, h, V, plane_y=-20.0, tile_voxels=1.0, seed=3):
    """A coherent floor patch on which an 8x8 tile is `tile_voxels` voxels wide (150 world units across V voxels)."""
    extent = 0.5 * tile_voxels * (150.0 / V) * max(w, h) / 8.0
    return synth.coherent_gbuffer(w, h, seed=seed, plane_y=plane_y, extent=extent)


def thin_shell(V, seed=7):
    return synth.noise_volume(V, seed=seed, occupancy=0.08)


def dense(V, seed=5):
    """Random colours, every other voxel opaque and the rest empty: the filtered alpha of the first steps varies across
    a tile from 0 to 1, so cones end after a few steps, each lane at a step of its own."""
    r = np.random.default_rng(seed)
    l0 = r.integers(0, 256, (V, V, V, 4), dtype=np.uint8)
    l0[..., 3] = np.where(r.uniform(size=(V, V, V)) < 0.5, 255, 0)
    return l0


def faint(V, seed, divisor):
    """Every voxel occupied, bytes U[0, 255 / divisor]: cones march on for many steps."""
    return np.random.default_rng(seed).integers(0, 256, (V, V, V, 4), dtype=np.uint8) // np.uint8(divisor)


def row_steps(ref_steps, w, h):
    per_pixel_row = ref_steps.astype(np.int64).sum(axis=1).reshape(h, w).sum(axis=1)
    return np.array([per_pixel_row[r:r + 8].sum() for r in range(0, h, 8)], np.uint64)


def check(vct, oracle, ctx, chain, planes, w, h, cam=None):
    """One whole-frame trace against the oracle; returns (oracle result, frame)."""
    cfg = ctx.current_config()
    kw = {o: getattr(cfg, k) for k, o in CONSTS.items()}
    if cam is not None:
        ctx.set_camera_position(cam)
        kw["camera_pos"] = cam
    ref = oracle.trace(oracle.default_params(cfg.voxel_dim, **kw), chain, planes, nthreads=8, want_cones=True)
    out = ctx.trace(planes).copy()
    assert np.array_equal(ctx.steps(), ref["steps"]), "per-cone step counts differ"
    assert np.array_equal(ctx.cones().view(np.uint32), ref["cones"].view(np.uint32)), "raw cone results are not bit-identical"
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


@pytest.mark.parametrize("volume", ["thin_shell", "dense"])
def test_zero_and_filled_blocks(vct, oracle, volume):
    """Thin shell: a cone walks through empty space (all-zero descriptors) into the shell (a filled block of the same
    level after a zero one).  Dense: filled blocks throughout, lanes ending at different steps."""
    V, w, h = 32, 16, 16
    l0 = thin_shell(V) if volume == "thin_shell" else dense(V)
    chain = oracle.build_mips(l0)
    with make_ctx(vct, V, w, h) as ctx:
        ctx.upload_chain(chain)
        ref, _ = check(vct, oracle, ctx, chain, floor(w, h, V), w, h)
        alive_steps = ref["steps"]
        if volume == "thin_shell":
            assert alive_steps.max() > 8                              # cones that march far
        else:
            tile = alive_steps.reshape(h, w, 7)[:8, :8]               # lanes of one tile ending at different steps
            assert sum(len(np.unique(tile[..., c])) > 1 for c in range(7)) >= 2


@pytest.mark.parametrize("V,wrap", [(32, 1), (16, 0)])
def test_grid_face(vct, oracle, V, wrap):
    """The floor 1.5 voxels under the grid's top face, the camera above it: diffuse and specular cones leave through the
    face within a few steps -- blocks across the seam of GL_REPEAT, or (clamp, V = 16) hanging over the edge."""
    w, h = 16, 16
    chain = oracle.build_mips(faint(V, 8, 4))         # faint: cones march on through the face
    planes = floor(w, h, V, plane_y=75.0 - 1.5 * 150.0 / V)
    with make_ctx(vct, V, w, h, wrap_repeat=wrap) as ctx:
        ctx.upload_chain(chain)
        ref, _ = check(vct, oracle, ctx, chain, planes, w, h, cam=CAM_ABOVE)
        assert ref["steps"].min() >= 3                                 # step 3 lies 4.6 voxels out: past the face for every cone


def test_self_overlapping_blocks(vct, oracle):
    """V = 16, one tile: the diffuse march reaches the levels of 4, 2 and 1 texels, whose 4x4x4 block wraps onto itself."""
    V, w, h = 16, 8, 8
    chain = oracle.build_mips(faint(V, 2, 16))        # nearly transparent: every cone runs its table out
    with make_ctx(vct, V, w, h, max_distance=150.0) as ctx:
        ctx.upload_chain(chain)
        ref, _ = check(vct, oracle, ctx, chain, floor(w, h, V), w, h)
        # diffuse steps at 1, 2.2, 4.6 and 10 voxels: LOD 0.2, 1.3, 2.4, 3.5 -- levels (0, 1) ... (3, 4) of 16 ... 1 texels
        assert (ref["steps"][:, :6] == 4).all()


@pytest.mark.parametrize("case", ["lane_27_dead", "one_live_lane", "lane_27_ends_first"])
def test_changing_anchor_source(vct, oracle, case):
    """The anchor is the footprint of lane 27 while it is live, of the first live lane otherwise: between the fetch of a
    block and its reuse the source may change (another cone, a lane that ended)."""
    V, w, h = 32, 8, 8
    planes = floor(w, h, V)
    if case == "lane_27_dead":
        planes[18, np.random.default_rng(4).uniform(size=w * h) < 0.2] = 0.0       # (discard_frac of the random G-buffer)
        planes[18, 27] = 0.0
        l0 = thin_shell(V, seed=9)
    elif case == "one_live_lane":
        planes[18, :] = 0.0
        planes[18, 13] = 1.0
        l0 = thin_shell(V, seed=9)
    else:
        l0 = dense(V, seed=11)
    chain = oracle.build_mips(l0)
    with make_ctx(vct, V, w, h) as ctx:
        ctx.upload_chain(chain)
        ref, _ = check(vct, oracle, ctx, chain, planes, w, h)
        if case == "lane_27_ends_first":                               # for some cone, lane 27 ends before another lane does
            assert (ref["steps"][27] < ref["steps"].max(axis=0)).any()


@pytest.mark.parametrize("kw", [dict(tan_specular=0.07), dict(tan_specular=0.2), dict(max_distance=150.0, max_alpha=0.5)],
                         ids=["spec_0.07", "spec_0.2", "distance_alpha"])
def test_apertures_and_march_constants(vct, oracle, kw):
    """Narrow specular cones stay on one pair of levels for many steps (reuse in place, in both slabs); a doubled
    max_distance runs the tables to the coarsest level, where two_levels is false."""
    V, w, h = 32, 16, 16
    chain = oracle.build_mips(thin_shell(V, seed=12))
    with make_ctx(vct, V, w, h, **kw) as ctx:
        ctx.upload_chain(chain)
        check(vct, oracle, ctx, chain, floor(w, h, V, tile_voxels=0.5), w, h, cam=CAM_ABOVE)


def test_rows_strided_and_components(vct, oracle):
    """The instantiations besides the whole-frame default: tile-row ranges and strided rows of an 8 x 24 frame (launches of
    at most half the frame take the kernel without issue priority around the loads), the packed form through the
    library's self-test, and the lighting-components kernel (outputs on with every component shown: the default frame;
    a mask that marches the specular group alone)."""
    V, w, h = 32, 8, 24
    chain = oracle.build_mips(thin_shell(V, seed=14))
    planes = floor(w, h, V)
    with make_ctx(vct, V, w, h) as ctx:
        ctx.upload_chain(chain)
        ref, full = check(vct, oracle, ctx, chain, planes, w, h)
        per_row = row_steps(ref["steps"], w, h)
        for r in range(3):
            part = ctx.trace(planes, rows=(r, r + 1))
            assert np.array_equal(part[r * 8:r * 8 + 8], full[r * 8:r * 8 + 8]) and ctx.last_step_count() == per_row[r]
            sel = slice(r * 64, r * 64 + 64)
            assert np.array_equal(ctx.steps()[sel], ref["steps"][sel])
            assert np.array_equal(ctx.cones()[sel].view(np.uint32), ref["cones"][sel].view(np.uint32))
        ctx.trace(planes)
        for rank in range(3):
            ctx.trace_gbuffer_strided(rank, 3, 3)
            ctx.synchronize()
            assert ctx.last_step_count() == per_row[rank]
            assert np.array_equal(ctx.download_frame()[rank * 8:rank * 8 + 8], full[rank * 8:rank * 8 + 8])
        assert ctx.selftest_interleaved(3) == 0
        # lighting components
        ctx.set_aov_outputs(cr.AOV_INDIRECT_DIFFUSE | cr.AOV_INDIRECT_SPECULAR | cr.AOV_DIRECT)
        assert np.array_equal(ctx.trace(planes), full)
        assert np.array_equal(ctx.steps(), ref["steps"])
        assert np.array_equal(ctx.cones().view(np.uint32), ref["cones"].view(np.uint32))
        ctx.set_aov_outputs(0)
        mask = cr.SHOW_SPECULAR | cr.SHOW_INDIRECT_SPECULAR
        ctx.set_lighting_components(mask)
        ctx.trace(planes)
        want = cr.masked_cones(ref["cones"], mask)
        assert np.array_equal(ctx.cones().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(ctx.steps()[:, 6], ref["steps"][:, 6]) and not ctx.steps()[:, :6].any()


def test_descriptors_do_not_outlive_a_launch(vct, oracle):
    """Two launches over the resident G-buffer with another specular aperture in between: the second launch's step tables
    name other levels at the same steps, and nothing of the first launch's blocks may be taken for them."""
    V, w, h = 32, 16, 16
    chain = oracle.build_mips(thin_shell(V, seed=12))
    planes = floor(w, h, V, tile_voxels=0.5)
    with make_ctx(vct, V, w, h) as ctx:
        ctx.upload_chain(chain)
        ref, first = check(vct, oracle, ctx, chain, planes, w, h, cam=CAM_ABOVE)
        ctx.trace_resident(); ctx.synchronize()
        assert np.array_equal(ctx.download_frame(), first)
        ctx.set_cone_apertures(0.577, 0.2)
        ctx.trace_resident(); ctx.trace_resident(); ctx.synchronize()
        cfg = ctx.current_config()
        kw = {o: getattr(cfg, k) for k, o in CONSTS.items()}
        assert abs(kw["tan_specular"] - 0.2) < 1e-6
        ref2 = oracle.trace(oracle.default_params(V, camera_pos=CAM_ABOVE, **kw), chain, planes, nthreads=8, want_cones=True)
        assert np.array_equal(ctx.steps(), ref2["steps"]) and ctx.last_step_count() == ref2["total_steps"]
        assert np.array_equal(ctx.cones().view(np.uint32), ref2["cones"].view(np.uint32))
        assert not np.array_equal(ref2["steps"][:, 6], ref["steps"][:, 6])
