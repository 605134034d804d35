"""GPU: what the frame slots' shared owners promise, at voxel_dim 16 with frames of at most 20 x 12.

1. The feature / mode matrix of csrc/vct_feature_rules.h from both sides: with the mode in force the feature's setter is
   refused, with the feature attached the mode's setter is refused; after either refusal the getters show what was there
   and a trace gives the frame of before the attempt, bit for bit.  Every pair whose mode has a setter is run here from both
   sides, and every pair whose mode exists in the config only (anisotropic_mips, debug_outputs) from the feature's side, so
   this file relies on no other file for a pair.  A VCT_STATS build is not among the built libraries: its row is held by
   tests/test_feature_rules_host.py alone.  Footprint records have no getter: that a refused vct_set_footprint_records left
   them off is shown by the feature's setter still being accepted.
2. The tiled hand-over (csrc/vct_planes.hip): what is set is what the matching download returns, bit for bit, for the three
   kinds of planes, the four layout x location combinations and frames with one tile, whole tiles, and partial tiles on
   either axis; and with two frames in flight, different contents per slot, set and downloaded in different orders.
3. The timed launches (vct_ctx.h VctTimer): the same five steps for each of the six getters."""
import numpy as np
import pytest

import gloss_ref as gr
import lights_ref as lr
import sky_ref as sr
import synth
import vctpkg
import voxcases
from test_gpu_parity import light_setup

pytestmark = pytest.mark.gpu

f32 = np.float32
V, W, H = 16, 20, 12
CAM, LIGHT = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)
CLASSES = list(gr.CLASSES[:3])
LIGHTS = [lr.point((10.0, -10.0, -20.0), (400.0, 300.0, 200.0), 45.0, 2.0)]
VOLUME = synth.noise_volume(V, seed=7, occupancy=0.3)
PLANES = synth.coherent_gbuffer(W, H)
EMISSION = np.random.default_rng(4).uniform(0.0, 2.0, (3, W * H)).astype(f32)


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return vctpkg.load()


def context(vct, w=W, h=H, **cfg):
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, voxel_attributes=1, **cfg))
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    ctx.upload_volume(VOLUME)
    ctx.build_mips()
    return ctx


def invalid(vct, call, *args):
    with pytest.raises(vct.VctError) as e:
        call(*args)
    assert "(-1)" in str(e.value), str(e.value)      # VCT_ERR_INVALID
    return str(e.value)


def accepted(vct, call, *args):
    try:
        call(*args)
        return True
    except vct.VctError:
        return False


# ---- 1. the matrix, both sides ----------------------------------------------------------------------------------------------
# feature -> (attach, what its getter shows)
FEATURES = {
    "mask": (lambda vct, c: c.set_lighting_components(vct.SHOW_ALL & ~vct.SHOW_SPECULAR), lambda vct, c: c.lighting_components()),
    "aov": (lambda vct, c: c.set_aov_outputs(vct.AOV_DIRECT), lambda vct, c: accepted(vct, c.aov_device, vct.AOV_DIRECT)),
    "rate2": (lambda vct, c: c.set_diffuse_rate(2), lambda vct, c: c.diffuse_rate()[0]),
    "emission": (lambda vct, c: c.set_pixel_emission(EMISSION), lambda vct, c: accepted(vct, c.download_pixel_emission)),
    "gloss": (lambda vct, c: c.set_gloss_classes(CLASSES), lambda vct, c: c.get_gloss_classes()[0].tobytes()),
    "sky": (lambda vct, c: c.set_sky(sr.SH), lambda vct, c: (c.sky()[0].tobytes(), c.sky()[2])),
    "lights": (lambda vct, c: c.set_lights(LIGHTS), lambda vct, c: [bytes(l) for l in c.lights()]),
    "two_frames": (lambda vct, c: c.set_frames_in_flight(2), lambda vct, c: c.frames_in_flight()[0]),
}
# mode with a setter -> (set, what shows it)
MODES = {
    "variant": (lambda vct, c: c.set_trace_variant(1), lambda vct, c: c.current_config().trace_variant),
    "variant4": (lambda vct, c: c.set_trace_variant(4), lambda vct, c: c.current_config().trace_variant),
    "cells": (lambda vct, c: c.set_footprint_records(True), None),
    "comm": (lambda vct, c: c.comm_init(vct.comm_unique_id(), 0, 1), lambda vct, c: accepted(vct, c.comm_slab)),
}
# the matrix as the setters had it before csrc/vct_feature_rules.h, written out
SETTER_PAIRS = [("mask", "variant"), ("aov", "variant"), ("aov", "comm"), ("rate2", "variant"), ("rate2", "cells"),
                ("rate2", "comm"), ("emission", "variant"), ("gloss", "variant"), ("gloss", "cells"), ("sky", "variant"),
                ("sky", "cells"), ("lights", "variant"), ("two_frames", "variant4")]
CONFIG_PAIRS = [("rate2", "anisotropic_mips"), ("gloss", "anisotropic_mips"), ("sky", "anisotropic_mips"),
                ("two_frames", "debug_outputs")]


def frame(ctx):
    return ctx.trace(PLANES)


def refused_with_nothing_changed(vct, ctx, attempt, getters):
    before = [g(vct, ctx) for g in getters]
    want = frame(ctx)
    invalid(vct, attempt, vct, ctx)
    assert [g(vct, ctx) for g in getters] == before
    assert np.array_equal(frame(ctx), want)


@pytest.mark.parametrize("feature,mode", SETTER_PAIRS, ids=[f"{f}-{m}" for f, m in SETTER_PAIRS])
def test_a_pair_of_the_matrix_is_refused_from_both_sides(vct, feature, mode):
    attach, shows_feature = FEATURES[feature]
    set_mode, shows_mode = MODES[mode]
    getters = [shows_feature] + ([shows_mode] if shows_mode else [])
    with context(vct) as ctx:                       # the mode in force, then the feature
        set_mode(vct, ctx)
        refused_with_nothing_changed(vct, ctx, attach, getters)
    with context(vct) as ctx:                       # the feature attached, then the mode
        attach(vct, ctx)
        refused_with_nothing_changed(vct, ctx, set_mode, getters)
        attach(vct, ctx)                            # (footprint records: still off, or this would be refused)


@pytest.mark.parametrize("feature,mode", CONFIG_PAIRS, ids=[f"{f}-{m}" for f, m in CONFIG_PAIRS])
def test_a_pair_with_a_config_only_mode_is_refused_by_the_feature(vct, feature, mode):
    attach, shows_feature = FEATURES[feature]
    with context(vct, **{mode: 1}) as ctx:
        refused_with_nothing_changed(vct, ctx, attach, [shows_feature])
    with context(vct) as ctx:                       # ... and by nothing else: without the mode the feature attaches
        attach(vct, ctx)


def test_pairs_outside_the_matrix_go_together(vct):
    """Some of the pairs the matrix does not list, as the setters had them: lights, emission and a mask with footprint
    records and on a rank; every feature but two frames with debug_outputs; two frames with variants 1 .. 3."""
    with context(vct) as ctx:
        ctx.set_footprint_records(True)
        ctx.comm_init(vct.comm_unique_id(), 0, 1)
        for f in ("lights", "emission", "mask"):
            FEATURES[f][0](vct, ctx)
        frame(ctx)
    with context(vct, debug_outputs=1) as ctx:
        for f in ("mask", "aov", "rate2", "emission", "gloss", "sky", "lights"):
            FEATURES[f][0](vct, ctx)
        frame(ctx)
    with context(vct) as ctx:
        ctx.set_frames_in_flight(2)
        for variant in (1, 2, 3, 0):
            ctx.set_trace_variant(variant)
            frame(ctx)


# ---- 2. the hand-over, round trip -------------------------------------------------------------------------------------------
def tiled(a, w, h):
    """linear [n, h*w] -> tiled [tile][n][64], zeros outside the frame."""
    n, tx, ty = a.shape[0], (w + 7) // 8, (h + 7) // 8
    full = np.zeros((n, ty * 8, tx * 8), a.dtype)
    full[:, :h, :w] = a.reshape(n, h, w)
    return np.ascontiguousarray(full.reshape(n, ty, 8, tx, 8).transpose(1, 3, 0, 2, 4).reshape(tx * ty, n, 64))


def contents(kind, w, h, seed):
    r = np.random.default_rng(seed)
    if kind == "gloss":
        return r.integers(0, 256, (1, w * h), dtype=np.uint8)
    bits = r.integers(0, 2 ** 32, ({"gbuffer": 23, "emission": 3}[kind], w * h), dtype=np.uint64).astype(np.uint32)
    return bits.view(f32)                           # every bit pattern, NaNs included: a hand-over moves bits


def hand_over(vct, ctx, kind, arg, layout):
    if kind == "gbuffer":
        ctx.trace(arg, rows=(0, 0), layout=layout)  # binds the G-buffer and launches no march
    elif kind == "emission":
        ctx.set_pixel_emission(arg, layout)
    else:
        ctx.set_pixel_gloss(arg, layout)


def download(ctx, kind):
    got = {"gbuffer": ctx.download_gbuffer, "emission": ctx.download_pixel_emission, "gloss": ctx.download_pixel_gloss}[kind]()
    return got.reshape(-1).view(np.uint8)


def on_device(ctx, a):
    """A torch tensor with a's bytes, filled on the context's (selected slot's) stream."""
    import torch
    with torch.cuda.stream(torch.cuda.ExternalStream(ctx.stream())):
        return torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to("cuda", non_blocking=False)


WAYS = [("linear", "host"), ("tiled", "host"), ("linear", "device"), ("tiled", "device")]


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (9, 17), (20, 12)], ids=["1x1", "8x8", "9x17", "20x12"])
@pytest.mark.parametrize("kind", ["gbuffer", "emission", "gloss"])
def test_what_is_set_is_what_the_download_returns(vct, kind, w, h):
    with context(vct, w=w, h=h) as ctx:
        if kind == "gloss":
            ctx.set_gloss_classes(CLASSES)
        for seed, (layout, where) in enumerate(WAYS):
            a = contents(kind, w, h, 10 + seed)
            src = tiled(a, w, h) if layout == "tiled" else a
            keep = on_device(ctx, src) if where == "device" else None
            arg = keep.data_ptr() if where == "device" else (src if kind != "gloss" else src.reshape(-1))
            hand_over(vct, ctx, kind, arg, vct.GB_TILED if layout == "tiled" else vct.GB_LINEAR)
            assert np.array_equal(download(ctx, kind), a.reshape(-1).view(np.uint8)), (layout, where)
            ctx.synchronize()
            del keep


@pytest.mark.parametrize("kind", ["gbuffer", "emission", "gloss"])
def test_two_slots_share_the_staging_and_keep_their_contents(vct, kind):
    """Slot 0, slot 1, slot 0 again are set through the one linear staging buffer and downloaded in the other order."""
    with context(vct) as ctx:
        if kind == "gloss":
            ctx.set_gloss_classes(CLASSES)
        ctx.set_frames_in_flight(2)
        a0, a1, a2 = (contents(kind, W, H, 20 + k) for k in range(3))
        for slot, a in ((0, a0), (1, a1), (0, a2)):
            ctx.select_frame_slot(slot)
            hand_over(vct, ctx, kind, a if kind != "gloss" else a.reshape(-1), vct.GB_LINEAR)
        for slot, a in ((1, a1), (0, a2), (1, a1)):
            ctx.select_frame_slot(slot)
            assert np.array_equal(download(ctx, kind), a.reshape(-1).view(np.uint8)), slot


# ---- 3. the timed launches --------------------------------------------------------------------------------------------------
def lit_context(vct):
    """A mesh under a shadow map with a light attached: every vct_inject_light runs the lights' voxel kernel."""
    pos, mat, alb = voxcases.random_scene(300, 7)
    depth, vp = light_setup(64, 3)
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=W, height=H, voxel_attributes=1))
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    ctx.upload_triangles(pos, mat, alb)
    ctx.upload_shadow_map(depth, vp)
    ctx.set_lights(LIGHTS)
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    return ctx


def gbuffer_inputs():
    g = PLANES
    return dict(position=np.ascontiguousarray(g[0:3].T), normal=np.ascontiguousarray(g[12:15].T),
                albedo=np.ascontiguousarray(np.vstack([g[15:18], g[18:19]]).T))


POINTS = np.ascontiguousarray(np.vstack([PLANES[0:3], PLANES[3:6], PLANES[6:9], PLANES[9:12]]).T[:40], f32)
IDENTITY = np.eye(4, dtype=f32).reshape(16)
# getter -> (the launch it times, its getter); every launch runs on the selected slot
TIMED = {
    "trace": (lambda c: c.trace(PLANES), lambda c: c.last_trace_ms()),
    "voxel_view": (lambda c: c.render_voxels(IDENTITY), lambda c: c.last_voxel_view_ms()),
    "point_query": (lambda c: c.gather_points(POINTS), lambda c: c.last_point_query_ms()),
    "gbuffer_import": (lambda c: c.import_gbuffer(**gbuffer_inputs()), lambda c: c.last_gbuffer_import_ms()),
    "lights_pixels": (lambda c: c.trace(PLANES), lambda c: c.last_lights_ms()[1]),
}


@pytest.mark.parametrize("what", list(TIMED))
def test_a_timed_launch_and_its_getter(vct, what):
    launch, ms = TIMED[what]
    with (lit_context(vct) if what == "lights_pixels" else context(vct)) as ctx:
        ctx.set_frames_in_flight(2)
        invalid(vct, ms, ctx)                       # never ran
        launch(ctx)
        assert ms(ctx) > 0
        ctx.set_trace_timing(False)
        launch(ctx)
        invalid(vct, ms, ctx)                       # ran with timing off
        ctx.set_trace_timing(True)
        launch(ctx)
        assert ms(ctx) > 0
        ctx.select_frame_slot(1)
        invalid(vct, ms, ctx)                       # the other slot has a timer of its own: never ran there
        ctx.set_trace_timing(False)
        launch(ctx)
        invalid(vct, ms, ctx)
        ctx.select_frame_slot(0)
        assert ms(ctx) > 0                          # ... and slot 0's result is untouched by slot 1's launches


def test_the_voxel_half_of_the_lights_timer_is_context_state(vct):
    with lit_context(vct) as ctx:                   # (its inject_light ran with timing on)
        ctx.set_frames_in_flight(2)
        invalid(vct, ctx.last_lights_ms)            # no composite launch on this slot yet
        ctx.trace(PLANES)
        assert ctx.last_lights_ms()[0] > 0 and ctx.last_lights_ms()[1] > 0
        ctx.set_trace_timing(False)
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        invalid(vct, ctx.last_lights_ms)            # the voxel kernel ran with timing off; the pixel half alone does not do
        ctx.set_trace_timing(True)
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        assert ctx.last_lights_ms()[0] > 0
        ctx.select_frame_slot(1)                    # the voxel half is the context's: slot 1 needs only a launch of its own
        invalid(vct, ctx.last_lights_ms)
        ctx.trace(PLANES)
        assert ctx.last_lights_ms()[0] > 0 and ctx.last_lights_ms()[1] > 0
        ctx.set_lights(None)                        # detached: both halves forgotten
        ctx.set_lights(LIGHTS)
        invalid(vct, ctx.last_lights_ms)
