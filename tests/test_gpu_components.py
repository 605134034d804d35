"""GPU: lighting components (the reference's Show* switches, include/vct.h VCT_SHOW_*) and per-component outputs
(VCT_AOV_*) of the trace kernel, against the numpy restatement (tests/components_ref.py) applied to the oracle's cones."""
import os
import subprocess

import numpy as np
import pytest

import components_ref as cr
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM, LIGHT = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)
ALL_AOV = cr.AOV_INDIRECT_DIFFUSE | cr.AOV_INDIRECT_SPECULAR | cr.AOV_DIRECT


@pytest.fixture(scope="module")
def vct():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import vctpkg
    return vctpkg.load()


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def seeded(oracle):
    """64^3 chain, 256x192 random G-buffer with discarded pixels, and the oracle's trace with raw cones."""
    V, w, h = 64, 256, 192
    chain = oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.06))
    planes = synth.random_gbuffer(w * h, seed=21, discard_frac=0.05)
    p = oracle.default_params(V, camera_pos=CAM, light_dir=LIGHT)
    ref = oracle.trace(p, chain, planes, nthreads=8, want_cones=True)
    return dict(V=V, w=w, h=h, chain=chain, planes=planes, params=p, ref=ref)


def _ctx(vct, s, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=s["V"], width=s["w"], height=s["h"], **kw))
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    ctx.upload_chain(s["chain"])
    return ctx


def _f16(u16):
    return np.asarray(u16, np.uint16).reshape(-1, 4)


def _ulp_diff(a, b):
    """|a - b| in fp16 ulps of the bit patterns (same-sign values; the outputs here are >= 0)."""
    return np.abs(_f16(a).astype(np.int32) - _f16(b).astype(np.int32))


def _assert_frame_matches(vct, frame, want32, what):
    """An RGBA16F frame against the restatement's fp32 frame rounded to fp16: relative L2 and fp16 values equal."""
    want16 = cr.to_f16_bits(want32)
    assert synth.rel_l2(vct.half_to_float(_f16(frame)), vct.half_to_float(want16)) <= 1e-4, what
    assert (_f16(frame) == want16).mean() >= 0.999, what


def _restated(s, mask, aov=0):
    p = s["params"]
    return cr.composite(s["planes"], cr.masked_cones(s["ref"]["cones"], mask, aov), CAM, LIGHT, p.ambient_factor,
                        p.shininess, mask)


def test_default_unchanged_with_outputs_on_64(vct, seeded):
    with _ctx(vct, seeded) as ctx:
        base = ctx.trace(seeded["planes"])
        steps = ctx.last_step_count()
        ctx.set_aov_outputs(ALL_AOV)
        assert ctx.lighting_components() == vct.SHOW_ALL
        with_aov = ctx.trace(seeded["planes"])
        assert np.array_equal(base, with_aov)
        assert ctx.last_step_count() == steps == seeded["ref"]["total_steps"]
        ctx.set_aov_outputs(0)
        assert np.array_equal(ctx.trace(seeded["planes"]), base)


def test_default_unchanged_with_outputs_on_atrium_1080p(vct):
    from voxel_cone_tracing_amd import scene as sc
    V, w, h, S = 256, 1920, 1080, 4096
    light = (0.0, 1.0, 0.25)
    cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
    with vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S)) as ctx:
        ctx.upload_scene(sc.Scene(sc.ATRIUM, 1.0, 1234))
        ctx.set_camera_position(tuple(cam.position))
        ctx.set_light_direction(light)
        ctx.render_shadow_map(sc.light_view_proj(light))
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        ctx.render_gbuffer(sc.camera_view_proj(cam, w, h))
        base = ctx.trace_current()
        steps = ctx.last_step_count()
        ctx.set_aov_outputs(ALL_AOV)
        assert np.array_equal(ctx.trace_current(), base)
        assert ctx.last_step_count() == steps
        # the outputs of the full frame are consistent with the frame: discarded pixels zero, direct alpha 1 elsewhere
        gb = ctx.download_gbuffer()
        alive = gb[18] >= 0.5
        d = _f16(ctx.download_aov(vct.AOV_DIRECT))
        assert (d[~alive] == 0).all() and (d[alive, 3] == 0x3c00).all()


def test_every_mask_against_restatement(vct, seeded):
    ref = seeded["ref"]
    alive = seeded["planes"][18] >= 0.5
    with _ctx(vct, seeded, debug_outputs=1) as ctx:
        for mask in range(32):
            ctx.set_lighting_components(mask)
            assert ctx.lighting_components() == mask
            frame = ctx.trace(seeded["planes"])
            want = _restated(seeded, mask)
            _assert_frame_matches(vct, frame, want["rgba32f"], mask)
            # raw cones: marched groups bit-equal to the oracle's, skipped ones zero with 0 steps
            dif, spc = cr.marched_groups(mask)
            cones, st = ctx.cones(), ctx.steps()
            want_cones = cr.masked_cones(ref["cones"], mask)
            assert np.array_equal(cones[alive], want_cones[alive]), mask
            want_steps = ref["steps"].copy()
            if not dif:
                want_steps[:, :6] = 0
            if not spc:
                want_steps[:, 6] = 0
            assert np.array_equal(st, want_steps), mask
            assert ctx.last_step_count() == cr.marched_steps(ref["steps"], mask), mask
        ctx.set_lighting_components(cr.SHOW_DIFFUSE | cr.SHOW_SPECULAR)
        ctx.trace(seeded["planes"])
        assert ctx.last_step_count() == 0
        ctx.set_lighting_components(cr.SHOW_SPECULAR | cr.SHOW_INDIRECT_SPECULAR)
        ctx.trace(seeded["planes"])
        assert ctx.last_step_count() == int(ref["steps"][:, 6].astype(np.int64).sum())


@pytest.mark.parametrize("mask", [cr.SHOW_ALL, cr.SHOW_DIFFUSE | cr.SHOW_SPECULAR, 0])
def test_outputs_are_raw_components(vct, seeded, mask):
    ref = seeded["ref"]
    alive = seeded["planes"][18] >= 0.5
    want = _restated(seeded, cr.SHOW_ALL)
    with _ctx(vct, seeded) as ctx:
        ctx.set_lighting_components(mask)
        ctx.set_aov_outputs(ALL_AOV)
        frame = ctx.trace(seeded["planes"])
        _assert_frame_matches(vct, frame, _restated(seeded, mask, ALL_AOV)["rgba32f"], mask)
        isp = _f16(ctx.download_aov(vct.AOV_INDIRECT_SPECULAR))
        idf = _f16(ctx.download_aov(vct.AOV_INDIRECT_DIFFUSE))
        dr = _f16(ctx.download_aov(vct.AOV_DIRECT))
    want_spec = cr.to_f16_bits(ref["cones"][:, 6, :])
    assert np.array_equal(isp[alive], want_spec[alive])
    want_ind = cr.to_f16_bits(cr.gather(ref["cones"]))
    du = _ulp_diff(idf[alive], want_ind[alive])
    assert du.max() <= 1 and (du == 0).mean() >= 0.9999
    dd = _ulp_diff(dr[alive], cr.to_f16_bits(want["direct"])[alive])
    assert dd.max() <= 1
    for o in (isp, idf, dr):
        assert (o[~alive] == 0).all()


def _scene_ctx(vct, V=64, w=128, h=128, S=512, **kw):
    from voxel_cone_tracing_amd import scene as sc
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S, **kw))
    ctx.upload_scene(sc.Scene(sc.CORNELL))
    cam = sc.default_camera(position=(0.0, 0.0, 58.0), yaw=-90.0)
    light = (0.0, 1.0, 0.25)
    ctx.set_camera_position(tuple(cam.position))
    ctx.set_light_direction(light)
    return ctx, sc.light_view_proj(light), sc.camera_view_proj(cam, w, h)


MASK = cr.SHOW_DIFFUSE | cr.SHOW_INDIRECT_SPECULAR | cr.SHOW_AMBIENT_OCCLUSION


def _outputs(vct, ctx):
    return [ctx.download_aov(b) for b in (vct.AOV_INDIRECT_DIFFUSE, vct.AOV_INDIRECT_SPECULAR, vct.AOV_DIRECT)]


def test_paths_agree(vct):
    ctx, lvp, vp = _scene_ctx(vct)
    with ctx:
        ctx.render_shadow_map(lvp)
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        ctx.render_gbuffer(vp)
        planes = ctx.download_gbuffer()
        ctx.set_lighting_components(MASK)
        ctx.set_aov_outputs(ALL_AOV)
        # vct_trace (host G-buffer)
        f_trace = ctx.trace(planes)
        o_trace = _outputs(vct, ctx)
        assert (planes[18] >= 0.5).mean() > 0.5
        assert not np.array_equal(o_trace[0], np.zeros_like(o_trace[0]))
        # vct_render_gbuffer + vct_trace_resident
        ctx.render_gbuffer(vp)
        ctx.trace_resident(); ctx.synchronize()
        assert np.array_equal(ctx.download_frame(), f_trace)
        assert all(np.array_equal(a, b) for a, b in zip(_outputs(vct, ctx), o_trace))
        # vct_gi_pass (whole pass, the same light and camera)
        ctx.gi_pass(lvp, vp); ctx.synchronize()
        assert np.array_equal(ctx.download_frame(), f_trace)
        assert all(np.array_equal(a, b) for a, b in zip(_outputs(vct, ctx), o_trace))
        # vct_set_footprint_records(ctx, 1): same frame, same outputs
        ctx.set_footprint_records(True)
        ctx.build_mips()
        assert np.array_equal(ctx.trace(planes), f_trace)
        assert all(np.array_equal(a, b) for a, b in zip(_outputs(vct, ctx), o_trace))
        ctx.set_footprint_records(False)
        ctx.build_mips()
        # vct_trace_slab: the slab's rows written, the others untouched (fresh, zeroed outputs)
        ctx.set_aov_outputs(0)
        ctx.set_aov_outputs(ALL_AOV)
        slab = ctx.trace(planes, rows=(3, 9))
        r0, r1 = 3 * 8, 9 * 8
        assert np.array_equal(slab[r0:r1], f_trace[r0:r1])
        for a, b in zip(_outputs(vct, ctx), o_trace):
            assert np.array_equal(a[r0:r1], b[r0:r1])
            assert not a[:r0].any() and not a[r1:].any()
        ctx.trace_gbuffer_rows(0, 16)            # the whole frame again (resident traces repeat the last rows)
        # two frame slots: per-slot outputs, frames bit-identical to one slot
        ctx.set_frames_in_flight(2)
        ptrs = []
        for slot in (0, 1):
            ctx.select_frame_slot(slot)
            ctx.render_gbuffer(vp)
            ctx.trace_gbuffer_rows(0, 16)
            ptrs.append(ctx.aov_device(vct.AOV_DIRECT))
        ctx.synchronize()
        for slot in (0, 1):
            ctx.select_frame_slot(slot)
            assert np.array_equal(ctx.download_frame(), f_trace)
            assert all(np.array_equal(a, b) for a, b in zip(_outputs(vct, ctx), o_trace))
        assert ptrs[0][0] != ptrs[1][0] and ptrs[0][1] == ptrs[1][1] == 128 * 128 * 8
        ctx.set_aov_outputs(vct.AOV_DIRECT)          # reallocated for both slots
        ctx.select_frame_slot(0)
        ctx.trace_gbuffer_rows(0, 16); ctx.synchronize()
        assert np.array_equal(ctx.download_aov(vct.AOV_DIRECT), o_trace[2])
        ctx.set_frames_in_flight(1)


def test_anisotropic_mips(vct):
    ctx, lvp, vp = _scene_ctx(vct, anisotropic_mips=1, debug_outputs=1)
    with ctx:
        ctx.render_shadow_map(lvp)
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        ctx.render_gbuffer(vp)
        planes = ctx.download_gbuffer()
        base = ctx.trace(planes)
        cones = ctx.cones()
        ctx.set_aov_outputs(ALL_AOV)
        assert np.array_equal(ctx.trace(planes), base)              # SHOW_ALL + outputs: the default frame
        alive = planes[18] >= 0.5
        isp = _f16(ctx.download_aov(vct.AOV_INDIRECT_SPECULAR))
        assert np.array_equal(isp[alive], cr.to_f16_bits(cones[:, 6, :])[alive])
        ctx.set_lighting_components(MASK)
        frame = ctx.trace(planes)
        want = cr.composite(planes, cr.masked_cones(cones, MASK, ALL_AOV), (0.0, 0.0, 58.0), (0.0, 1.0, 0.25),
                            ctx.cfg.ambient_factor, ctx.cfg.shininess, MASK)
        _assert_frame_matches(vct, frame, want["rgba32f"], MASK)


def test_rejections(vct, seeded):
    with _ctx(vct, seeded) as ctx:
        with pytest.raises(vct.VctError):
            ctx.set_lighting_components(32)
        with pytest.raises(vct.VctError):
            ctx.set_aov_outputs(8)
        with pytest.raises(vct.VctError):
            ctx.download_aov(vct.AOV_DIRECT)                         # not on
        for variant in (1, 2, 3, 4):
            ctx.set_trace_variant(variant)
            with pytest.raises(vct.VctError):
                ctx.set_lighting_components(cr.SHOW_DIFFUSE)
            with pytest.raises(vct.VctError):
                ctx.set_aov_outputs(vct.AOV_DIRECT)
            ctx.set_trace_variant(0)
        ctx.set_lighting_components(cr.SHOW_DIFFUSE)
        for variant in (1, 2, 3, 4):
            with pytest.raises(vct.VctError):
                ctx.set_trace_variant(variant)
        ctx.set_lighting_components(cr.SHOW_ALL)
        ctx.set_aov_outputs(vct.AOV_DIRECT)
        with pytest.raises(vct.VctError):
            ctx.set_trace_variant(3)
        with pytest.raises(vct.VctError):
            ctx.download_aov(vct.AOV_DIRECT | vct.AOV_INDIRECT_DIFFUSE)   # one bit only
        ctx.set_aov_outputs(0)
        ctx.set_trace_variant(0)
        ctx.comm_init(vct.comm_unique_id(), 0, 1)
        with pytest.raises(vct.VctError):
            ctx.set_aov_outputs(vct.AOV_DIRECT)
        ctx.set_lighting_components(MASK)                            # ranks honour the mask
        ctx.comm_destroy()


def _demo(args, env=None):
    exe = os.path.join(ROOT, "voxel-cone-tracing_amd", "vct_demo")
    assert os.path.exists(exe), "build it with `make demo`"
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    return dict(kv.split("=") for kv in out.stdout.strip().split("\n")[-1].split()), out.stdout


def test_facade_demo_show_matches_binding(vct):
    """vct_demo --show indirect-specular,ao hashes to the binding's frame with that mask (the pattern of
    test_gpu_parity.test_facade_demo_matches_binding)."""
    from voxel_cone_tracing_amd import scene as sc
    import raster_oracle
    V, w, h, S = 64, 128, 128, 512
    fields, _ = _demo(["--show", "indirect-specular,ao", "--scene", "procedural:cornell", "--voxels", str(V), "--size",
                       f"{w}x{h}", "--shadow", str(S), "--frames", "1"])
    scene = sc.Scene(sc.CORNELL)
    light = (0.0, 1.0, 0.25)
    depth, light_vp = raster_oracle.shadow_map(sc, scene, light, S)
    cam = sc.default_camera(position=(0.0, 0.0, 58.0))
    planes = raster_oracle.gbuffer(sc, scene, cam, w, h, depth, light_vp)
    with vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S)) as ctx:
        ctx.set_camera_position((0.0, 0.0, 58.0))
        ctx.set_light_direction(light)
        ctx.upload_triangles(scene.pos, scene.material, scene.albedo)
        ctx.upload_shadow_map(depth, light_vp)
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        full = ctx.trace(planes)
        ctx.set_lighting_components(cr.SHOW_INDIRECT_SPECULAR | cr.SHOW_AMBIENT_OCCLUSION)
        frame = ctx.trace(planes)
        assert int(fields["cone_steps"]) == ctx.last_step_count()
    assert not np.array_equal(frame, full)
    hsh = 1469598103934665603
    for v in frame.reshape(-1).tolist():
        hsh = ((hsh ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert fields["fnv1a"] == f"{hsh:016x}"


def test_facade_demo_show_two_ranks_direct_slabs(vct):
    """--gpus 2 (direct slabs, both ranks on device 0) with a mask: rank 0's frame equals the single-process one."""
    args = ["--show", "diffuse,indirect-diffuse,ao", "--scene", "procedural:cornell", "--voxels", "32", "--size", "96x64",
            "--shadow", "256", "--frames", "4"]
    one, _ = _demo(args)
    env = dict(os.environ, VCT_COMM_MODE="direct", VCT_DEMO_SINGLE_DEVICE="1")
    two, txt = _demo(args + ["--gpus", "2"], env=env)
    full, _ = _demo(args[2:])
    assert "gpus=2" in txt and one["fnv1a"] == two["fnv1a"] != full["fnv1a"]
