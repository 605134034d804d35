"""GPU: the two forms in which the default trace kernel's texel-buffer loads reach a mip level (csrc/vct_trace.hip ChainRef).

  chain form   one buffer resource per wave over the whole chain, the level's byte offset in the load's scalar offset
               operand -- what a context takes whose levels all start below 4 GiB
  level form   a resource per level and fetch -- what a 1024^3 chain takes (tests/test_gpu_configs.py config 5), and any
               context created under VCT_LEVEL_DESCRIPTORS=1 (environment switches)

Both read the same addresses through the same conversion, so every case asks the same of both: per-cone step counts and raw
cone vec4s equal to the CPU oracle's bit for bit (debug outputs, as tests/test_gpu_parity.py compares them), and frames
that are byte for byte the same between the forms.  Short chains (voxel_dim 16 and 64), so that every level -- the ones of
8 texels and of 1 included -- sits at a non-zero offset of its own and a 64 x 64 frame reaches them: the noise volume and a
voxelized triangle scene, GL_REPEAT and clamp, the whole frame (the kernel with issue priority) and a launch of one tile
row (the one without), the anisotropic chains, and a chain after the second bounce.  The frame is half coherent (the
cooperative block fetch) and half random pixels (the per-lane gather).

The chain form exists for the default kernel's plain GL_REPEAT launches only, with and without issue priority.  In clamp
mode and with the anisotropic chains both contexts run the same kernels, as they do for the bounce march itself: there
the comparison between the forms' frames says nothing, and what the case checks is the oracle comparison -- that a
context which MAY take the chain form (step tables, parameters, dispatch) still gives the oracle's bits where it does
not.  Which form a launch took is read from vct_get_stage_counts [2] (stage_counts()["texel_resource"]: 2 one resource
per wave, 1 one per level) and asserted in every case, so a context that fell back without being asked fails here.  The
last case is vct_create's texel self-test, whose count includes the reads through non-zero scalar offsets."""
import os

import numpy as np
import pytest

import synth
import vctpkg
import voxcases

pytestmark = pytest.mark.gpu

W = H = 64
FORMS = ("chain", "level")


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


def make_ctx(vct, form, V, **kw):
    """A 64 x 64 context with debug outputs; form "level": created under VCT_LEVEL_DESCRIPTORS=1 (read at vct_create)."""
    old = os.environ.pop("VCT_LEVEL_DESCRIPTORS", None)
    if form == "level":
        os.environ["VCT_LEVEL_DESCRIPTORS"] = "1"
    try:
        return vct.Context(vct.default_config(voxel_dim=V, width=W, height=H, debug_outputs=1, **kw))
    finally:
        os.environ.pop("VCT_LEVEL_DESCRIPTORS", None)
        if old is not None:
            os.environ["VCT_LEVEL_DESCRIPTORS"] = old


def mixed_gbuffer(V, seed):
    """Upper half: a coherent floor patch on which a tile spans about a voxel; lower half: independent random pixels."""
    extent = 0.5 * (150.0 / V) * W / 8.0
    planes = synth.coherent_gbuffer(W, H, seed=seed, extent=extent)
    rnd = synth.random_gbuffer(W * H, seed=seed + 1, discard_frac=0.05)
    planes[:, W * H // 2:] = rnd[:, W * H // 2:]
    return planes


def oracle_params(oracle, ctx, V):
    cfg = ctx.current_config()
    return oracle.default_params(V, G=cfg.grid_world_size, max_distance=cfg.max_distance, max_alpha=cfg.max_alpha,
                                 tan_diffuse=cfg.tan_diffuse, tan_specular=cfg.tan_specular, shininess=cfg.shininess,
                                 ambient_factor=cfg.ambient_factor, wrap_repeat=cfg.wrap_repeat)


def check_bits(ctx, ref, rows=None):
    sel = slice(None) if rows is None else slice(rows[0] * 8 * W, rows[1] * 8 * W)
    assert np.array_equal(ctx.steps()[sel], ref["steps"][sel]), "per-cone step counts differ"
    assert np.array_equal(ctx.cones()[sel].view(np.uint32), ref["cones"][sel].view(np.uint32)), "raw cones are not bit-identical"


PER_LEVEL, PER_WAVE = 1, 2          # stage_counts()["texel_resource"]


def trace_both_forms(vct, oracle, V, prepare, reference, row=3, chain_kernels=True, **kw):
    """Every form: whole frame and one tile row against `reference(ctx)` (the oracle's result, computed once); then the
    forms' frames against each other.  chain_kernels: the configuration has kernels of the chain form, so the context
    that may take them must report that it did."""
    ref = None
    frames = {}
    for form in FORMS:
        with make_ctx(vct, form, V, **kw) as ctx:
            planes = prepare(ctx)
            if ref is None:
                ref = reference(ctx, planes)
            want_form = PER_WAVE if form == "chain" and chain_kernels else PER_LEVEL
            full = ctx.trace(planes).copy()                       # whole frame: the kernel with issue priority
            assert ctx.stage_counts()["texel_resource"] == want_form, form
            check_bits(ctx, ref)
            assert ctx.last_step_count() == ref["total_steps"]
            part = ctx.trace(planes, rows=(row, row + 1)).copy()  # an eighth of the frame: the kernel without
            assert ctx.stage_counts()["texel_resource"] == want_form, form
            check_bits(ctx, ref, rows=(row, row + 1))
            assert np.array_equal(part[row * 8:row * 8 + 8], full[row * 8:row * 8 + 8])
            frames[form] = full
    assert frames["chain"].tobytes() == frames["level"].tobytes(), "the frame differs between the descriptor forms"
    assert (frames["chain"].reshape(-1, 4) == ref["rgba16f"]).mean() > 0.999
    return ref


@pytest.mark.parametrize("wrap", [1, 0], ids=["repeat", "clamp"])
@pytest.mark.parametrize("V", [16, 64])
def test_noise_volume(vct, oracle, V, wrap):
    """max_distance 150: the diffuse table runs to the coarsest levels, the specular one stays long on the fine ones."""
    chain = oracle.build_mips(synth.noise_volume(V, seed=5, occupancy=0.1))

    def prepare(ctx):
        ctx.upload_chain(chain)
        return mixed_gbuffer(V, seed=3)

    def reference(ctx, planes):
        return oracle.trace(oracle_params(oracle, ctx, V), chain, planes, nthreads=8, want_cones=True)

    ref = trace_both_forms(vct, oracle, V, prepare, reference, chain_kernels=bool(wrap), wrap_repeat=wrap, max_distance=150.0)
    assert ref["steps"][:, :6].max() >= 4 and ref["steps"][:, 6].max() > ref["steps"][:, :6].max()


def test_voxelized_scene(vct, oracle):
    """A triangle scene voxelized, lit and mipped on the GPU: the chain the trace reads is the one the pipeline built."""
    V = 64
    pos, mat, alb = voxcases.random_scene(300, seed=33)
    l0 = oracle.voxelize_conservative(oracle.default_params(V), oracle.make_scene(pos, mat, alb))
    chain = oracle.build_mips(l0)

    def prepare(ctx):
        ctx.upload_triangles(pos, mat, alb)
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        assert np.array_equal(ctx.download_chain(), chain)
        return mixed_gbuffer(V, seed=9)

    def reference(ctx, planes):
        return oracle.trace(oracle_params(oracle, ctx, V), chain, planes, nthreads=8, want_cones=True)

    trace_both_forms(vct, oracle, V, prepare, reference)


def test_anisotropic_chains(vct, oracle):
    """config.anisotropic_mips (bench.py --anisotropic): levels >= 1 come from the six directional chains."""
    V = 16
    l0 = synth.noise_volume(V, seed=5, occupancy=0.2)
    chain, aniso = oracle.build_mips(l0), oracle.build_mips_aniso(l0)

    def prepare(ctx):
        ctx.upload_volume(l0)
        ctx.build_mips()
        assert np.array_equal(ctx.download_aniso(), aniso)
        return mixed_gbuffer(V, seed=6)

    def reference(ctx, planes):
        return oracle.trace_aniso(oracle_params(oracle, ctx, V), chain, aniso, planes, nthreads=8, want_cones=True)

    trace_both_forms(vct, oracle, V, prepare, reference, chain_kernels=False, anisotropic_mips=1, max_distance=150.0)


def test_two_bounces(vct, oracle):
    """vct_bounce, then the screen trace through the bounce-1 chain (the context's second chain allocation)."""
    V = 16
    pos, mat, alb = voxcases.random_scene(300, seed=33)
    p = oracle.default_params(V)
    l0, want_alb, want_nrm = oracle.voxelize_conservative_attr(p, oracle.make_scene(pos, mat, alb))
    chain0 = oracle.build_mips(l0)
    l1, want_steps = oracle.bounce(p, chain0, want_alb, want_nrm, nthreads=8)
    chain1 = oracle.build_mips(l1)
    assert (l1 != l0).any()

    def prepare(ctx):
        ctx.upload_triangles(pos, mat, alb)
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        ctx.bounce()
        assert ctx.last_step_count() == want_steps
        assert np.array_equal(ctx.download_chain(), chain1)
        return mixed_gbuffer(V, seed=12)

    def reference(ctx, planes):
        return oracle.trace(oracle_params(oracle, ctx, V), chain1, planes, nthreads=8, want_cones=True)

    trace_both_forms(vct, oracle, V, prepare, reference, voxel_attributes=1)


def test_selftest_counts_the_offset_reads(vct):
    """vct_create gates on the texel self-test; the count a context reports covers the zero-offset conversion of all 256
    byte values in every channel and the same texels read through two non-zero scalar offsets (two levels of a chain, the
    first up to its last texel below the second)."""
    for form in FORMS:
        with make_ctx(vct, form, 16) as ctx:
            assert ctx.selftest_texel_buffer() == 0
