"""GPU: the kernels of the three stages without code in the project this one was modelled on -- voxel attributes, second
bounce (k_bounce_list / k_bounce_march / k_bounce_bricks and their DYN forms), directional mips (k_mip_aniso) and the
directional route of the march -- held DIRECTLY to tests/highprec_ref.py, the float64 restatement written from the
header's prose: no oracle in any assertion.  Each stage is fed what the GPU itself produced for the stage before, through
the downloads that exist.  The rule (|byte - exact| <= 0.5 + eps, eps derived, at most 2 % left out and those held to
1 + eps; the cone bound of four times the oracle's measured deviation) is stated in highprec_ref.py; the cases are those
of tests/highprec_cases.py, whose left-out shares tests/test_highprec_restatement.py holds under the cap without a GPU.

Known answers of the bounce on the GPU: a scene of albedo zero (level 0 rgb all zero: nothing changes) and a double-sided
triangle (mean normal (128, 128, 128): copied, no step).  The frame's known answers (lit from one side) stay CPU-only:
they need a level 0 lit in chosen voxels around a dark white-albedo voxel, and the voxelizer writes albedo times shadow,
so no mesh gives that level 0 -- and vct_bounce takes its attributes from the voxelizer alone."""
import numpy as np
import pytest

import dynbouncecases as db
import dyncases as dc
import highprec_cases as hc
import highprec_ref as hp
import vctpkg

pytestmark = pytest.mark.gpu
IEEE = 1                                     # vct_get_stage_counts [2], as tests/test_gpu_march_params.py reads it


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


def pr_of(ctx):
    """The context's march parameters, its float32 fields widened exactly."""
    c = ctx.current_config()
    return dict(V=int(c.voxel_dim), G=float(c.grid_world_size), max_distance=float(c.max_distance),
                max_alpha=float(c.max_alpha), tan_diffuse=float(c.tan_diffuse), tan_specular=float(c.tan_specular),
                wrap_repeat=int(c.wrap_repeat))


def run_pass(ctx):
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()


def level0(ctx):
    V = ctx.current_config().voxel_dim
    return ctx.download_chain()[:V ** 3].reshape(V, V, V, 4)


# ---- directional mips ---------------------------------------------------------------------------------------------------
def mips_of(vct, l0):
    V = l0.shape[0]
    with vct.Context(vct.default_config(voxel_dim=V, width=8, height=8, anisotropic_mips=1)) as ctx:
        ctx.upload_volume(l0)
        ctx.build_mips()
        assert np.array_equal(level0(ctx), l0)
        return ctx.download_aniso()


@pytest.mark.parametrize("V, kind", [(V, k) for V in (8, 32) for k in hc.VOLUMES] + [(64, "alphas")])
def test_directional_mips(vct, V, kind):
    """8 is the smallest grid vct_create accepts; at 64^3 level 1 has 32768 texels per direction, more than one trip of
    k_mip_aniso's grid-stride loop."""
    l0 = hc.volume(kind, V)
    aniso = mips_of(vct, l0)
    x = hp.aniso_chain_from_bytes(l0, aniso)                       # every level from the previous level's downloaded bytes
    worst = hp.agree(aniso, x, hp.EPS_MIP, f"{kind} {V}")
    print(kind, V, "largest |b - x| - 0.5:", worst, "eps", hp.EPS_MIP)
    assert len(np.unique(aniso.reshape(6, -1), axis=0)) == 6


def test_known_directional_blocks(vct):
    V = 8
    for blk, want in hc.known_blocks():
        aniso = mips_of(vct, hc.tiled(blk, V))
        for d, texel in want.items():
            assert (aniso[d, :(V // 2) ** 3] == texel).all(), (blk.tolist(), d, aniso[d, 0], texel)


# ---- directional trace --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame, wrap, c", [(f, w, 0) for f in ("random", "coherent") for w in (1, 0)] +
                         [("random", 1, 2), ("coherent", 0, 2)])
def test_directional_trace(vct, frame, wrap, c):
    planes = hc.frames()[frame]
    cfg = vct.default_config(voxel_dim=16, width=hc.W, height=hc.H, debug_outputs=1, anisotropic_mips=1, wrap_repeat=wrap,
                             **hc.constants_kw(c, hc.TRACE_CONSTANTS))
    with vct.Context(cfg) as ctx:
        ctx.set_camera_position(hc.CAMERA)
        ctx.upload_volume(hc.volume("noise", 16))
        ctx.build_mips()
        chain, aniso = ctx.download_chain(), ctx.download_aniso()
        ctx.trace(planes)
        if c == 2:
            assert ctx.stage_counts()["march_division"] == IEEE
        got = hp.check_cones(pr_of(ctx), chain, aniso, planes, hc.CAMERA, ctx.cones(), ctx.steps(), bound=hp.CONE_BOUND,
                             what=f"{frame} wrap={wrap} constants={c}")
        print(frame, wrap, c, got, "bound", hp.CONE_BOUND)
        assert got["marched"] >= 2000 and ctx.last_step_count() == got["steps"]


# ---- attributes ---------------------------------------------------------------------------------------------------------
ALBEDO = (0.9, 0.3, 0.25, 1.0)
ALBEDO_BYTES = (230, 77, 64)             # tests/test_highprec_restatement.py: 0.9f * 255 = 229.4999939, rounded twice
FAR_CORNER = [[-1400.0, -1400.0, -1400.0], [-1300.0, -1400.0, -1400.0], [-1400.0, -1300.0, -1400.0]]


def assert_known_attributes(l0, alb, nrm, want, what):
    occ = l0[..., 3] > 0
    assert occ.sum() >= 4 and np.array_equal(occ, nrm[..., 3] == 255) and np.array_equal(occ, alb[..., 3] == 255), what
    assert not nrm[~occ].any() and not alb[~occ].any(), what
    assert (nrm[occ][:, :3] == want).all(), (what, np.unique(nrm[occ], axis=0).tolist(), want)
    assert (alb[occ][:, :3] == ALBEDO_BYTES).all(), (what, np.unique(alb[occ], axis=0).tolist())
    hp.agree(alb[occ][:, :3], hp.albedo_lsb(ALBEDO[:3])[None, :], hp.EPS_UNORM, what)


def test_known_attributes_static_and_dynamic(vct):
    V = 16
    with vct.Context(dc.config(vct, V)) as ctx:
        for name, (tri, want) in hc.KNOWN_TRIANGLES.items():
            assert tuple(hp.quantise_normal(hp.face_normal(tri))) == want
            ctx.set_dynamic_mesh(None)
            ctx.upload_triangles(*hc.tri_mesh([tri], [ALBEDO]))
            run_pass(ctx)
            assert_known_attributes(level0(ctx), *ctx.voxel_attributes(), want, name)
            ctx.upload_triangles(*hc.tri_mesh([FAR_CORNER], [ALBEDO]))          # the same triangle as the dynamic mesh
            ctx.set_dynamic_mesh(*hc.tri_mesh([tri], [ALBEDO]))
            run_pass(ctx)
            assert_known_attributes(*ctx.download_dynamic_voxels(), want, name + ", dynamic")


def test_attribute_ranges_and_two_materials(vct):
    with vct.Context(dc.config(vct, 32)) as ctx:
        ctx.upload_triangles(*dc.static_scene())
        run_pass(ctx)
        l0, (alb, nrm) = level0(ctx), ctx.voxel_attributes()
        occ = l0[..., 3] > 0
        assert occ.sum() >= 1000
        assert (nrm[occ] >= 1).all() and (nrm[occ][:, 3] == 255).all() and (alb[occ][:, 3] == 255).all()
        assert not nrm[~occ].any() and not alb[~occ].any() and not l0[~occ].any()
    q = [[-500.0, -400.0, 100.0], [450.0, -400.0, 100.0], [450.0, 500.0, 100.0], [-500.0, 500.0, 100.0]]
    halves = ([q[0], q[1], q[2]], [q[0], q[2], q[3]])
    with vct.Context(dc.config(vct, 16)) as ctx:
        one = []
        for t in halves:
            ctx.upload_triangles(*hc.tri_mesh([t], [ALBEDO]))
            run_pass(ctx)
            one.append(level0(ctx)[..., 3] > 0)
        ctx.upload_triangles(*hc.tri_mesh(halves, [ALBEDO, (0.2, 0.8, 0.6, 1.0)], [0, 1]))
        run_pass(ctx)
        l0, (alb, nrm) = level0(ctx), ctx.voxel_attributes()
    occ, shared = l0[..., 3] > 0, one[0] & one[1]
    assert shared.sum() >= 4 and np.array_equal(occ, one[0] | one[1])
    assert (nrm[occ][:, :3] == (128, 128, 255)).all()
    m0, m1 = np.array(ALBEDO_BYTES), np.array((51, 204, 153))
    assert (alb[one[0] & ~shared][:, :3] == m0).all() and (alb[one[1] & ~shared][:, :3] == m1).all()
    s = alb[shared][:, :3].astype(np.int64)
    assert (s >= np.minimum(m0, m1)).all() and (s <= np.maximum(m0, m1)).all()


# ---- bounce -------------------------------------------------------------------------------------------------------------
def bounce_and_check(ctx, what, attrs=None, changed=100):
    """Download the chain and the attributes, bounce, and hold the new level 0 and the step count to the float64 bounce."""
    chain0 = ctx.download_chain()
    alb, nrm = attrs if attrs is not None else ctx.voxel_attributes()
    before = level0(ctx)
    ctx.bounce()
    out, steps = level0(ctx), ctx.last_step_count()
    assert (out != before).any(-1).sum() >= changed, what
    r = hp.check_bounce(pr_of(ctx), chain0, alb, nrm, out, steps, what)
    print(what, r)
    return r


@pytest.mark.parametrize("V, wrap, G, c", hc.GPU_BOUNCE_CASES)
def test_bounce(vct, V, wrap, G, c):
    with vct.Context(dc.config(vct, V, G=G, wrap_repeat=wrap, **hc.constants_kw(c))) as ctx:
        ctx.upload_triangles(*hc.static_mesh(G))
        ctx.upload_shadow_map(*hc.shadow_for(G))
        run_pass(ctx)
        assert len(np.unique(level0(ctx).reshape(-1, 4), axis=0)) >= 20
        bounce_and_check(ctx, f"{V} wrap={wrap} G={G} constants={c}")


def test_bounce_dense_scene_reaches_the_brick_kernel(vct):
    V = 16
    with vct.Context(dc.config(vct, V)) as ctx:
        ctx.upload_triangles(*db.dense16_static())
        run_pass(ctx)
        assert (level0(ctx)[..., 3] > 0).sum() > V ** 3 // 8          # the voxel list cannot hold them all: k_bounce_bricks
        bounce_and_check(ctx, "dense 16^3")


@pytest.mark.parametrize("V, emission", [(16, False), (64, False), (16, True), (64, True)])
def test_bounce_over_the_dynamic_mesh(vct, V, emission):
    with vct.Context(dc.config(vct, V)) as ctx:
        ctx.upload_triangles(*dc.static_scene())
        ctx.set_dynamic_bounce(True)
        ctx.set_dynamic_mesh(*dc.dynamic_mesh(dc.A))
        if emission:
            ctx.set_dynamic_emission(hc.EMISSION)
        run_pass(ctx)
        D3, S3 = ctx.download_dynamic_voxels(), (None,) + tuple(ctx.voxel_attributes())
        d = D3[0][..., 3] > 0
        assert d.sum() >= 50
        if V == 64:                                                   # bricks of the mover without a static slot
            assert (dc.bricks(d) & ~dc.bricks(S3[2][..., 3] == 255)).sum() >= 1
        if emission:
            with vct.Context(dc.config(vct, V)) as plain:             # the table shows in the downloaded level 0
                plain.upload_triangles(*dc.static_scene())
                plain.set_dynamic_mesh(*dc.dynamic_mesh(dc.A))
                run_pass(plain)
                assert ((level0(plain) != level0(ctx)).any(-1) & d).sum() >= 20
        bounce_and_check(ctx, f"mover A at {V}^3, emission={emission}", attrs=db.owner(D3, S3))


def test_known_bounces_through_a_mesh(vct):
    V = 16
    pos, mat, alb = dc.static_scene()
    with vct.Context(dc.config(vct, V)) as ctx:
        # albedo zero everywhere: level 0 rgb all zero and the albedo attribute zero -- every byte as it was
        ctx.upload_triangles(pos, mat, np.zeros_like(alb))
        run_pass(ctx)
        before = level0(ctx)
        assert (before[..., 3] == 255).sum() >= 300 and not before[..., :3].any()
        ctx.bounce()
        assert np.array_equal(level0(ctx), before) and ctx.last_step_count() > 0
        # a double-sided triangle: the mean of the two normals is (128, 128, 128) -- copied, and no cone marches
        tri = hc.KNOWN_TRIANGLES["ccw_z"][0]
        ctx.upload_triangles(*hc.tri_mesh([tri, [tri[0], tri[2], tri[1]]], [ALBEDO]))
        run_pass(ctx)
        before, (_, nrm) = level0(ctx), ctx.voxel_attributes()
        occ = before[..., 3] == 255
        assert occ.sum() >= 4 and (nrm[occ] == (128, 128, 128, 255)).all() and before[occ][:, :3].any()
        ctx.bounce()
        assert np.array_equal(level0(ctx), before) and ctx.last_step_count() == 0
