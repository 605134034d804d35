"""CPU: tests/frame_ref.py, the composer of the feature references, is no second definition.  With exactly one feature on
it returns what that feature's own reference module returns, bit for bit, on the scene that feature's GPU test file uses;
with nothing on it returns the oracle's trace.  (What several features give together has no reference but the composer:
tests/test_gpu_feature_combinations.py holds the kernels to it.)"""
import os

import numpy as np
import pytest

import components_ref as cr
import diffuse_rate_ref as drr
import emission_ref as er
import frame_ref as fr
import gbcases as gc
import gloss_ref as gr
import lights_ref as lr
import sky_ref as sr
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
V, W, H = 32, 20, 12                          # tests/test_gpu_sky.py, tests/test_gpu_gloss.py
CAM, LIGHT = gc.CAM, gc.LIGHT
MASKS = [cr.SHOW_DIFFUSE | cr.SHOW_SPECULAR, cr.SHOW_SPECULAR | cr.SHOW_INDIRECT_SPECULAR, cr.SHOW_INDIRECT_DIFFUSE,
         cr.SHOW_AMBIENT_OCCLUSION | cr.SHOW_DIFFUSE, cr.SHOW_ALL & ~cr.SHOW_INDIRECT_SPECULAR]      # test_gpu_diffuse_rate.MASKS
ALL_AOV = cr.AOV_INDIRECT_DIFFUSE | cr.AOV_INDIRECT_SPECULAR | cr.AOV_DIRECT


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def dense(oracle):
    """test_gpu_sky's "dense" scene: a 30 % noise volume under a random G-buffer with discarded pixels."""
    chain = oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.3))
    planes = synth.random_gbuffer(W * H, seed=21, discard_frac=0.1)
    p = oracle.default_params(V, camera_pos=CAM, light_dir=LIGHT)
    return dict(chain=chain, planes=planes, p=p, ref=oracle.trace(p, chain, planes, nthreads=4, want_cones=True), cache={})


def compose(oracle, s, w=W, h=H, **what):
    return fr.frame_ref(oracle, s["p"], s["chain"], s["planes"], w, h, fr.attached(**what), s["cache"])


def test_nothing_attached_is_the_oracles_trace(oracle, dense):
    got, ref = compose(oracle, dense), dense["ref"]
    assert same(got["steps"], ref["steps"]) and same(got["cones"], ref["cones"]) and got["total_steps"] == ref["total_steps"]
    assert same(got["rgba32f"], ref["rgba32f"]) and same(got["frame32"], ref["rgba32f"]) and same(got["frame16"], ref["rgba16f"])
    assert got["lit"] is None and got["marched"] is None and got["outputs"] == {} and got["sel"].all()
    assert np.array_equal(got["live"], dense["planes"][18] >= 0.5)


def test_gloss_classes_alone(oracle, dense):
    classes = list(gr.CLASSES[:3])
    plane = gr.checkerboard(W, H, 3, in_frame_extra=200)
    want = gr.trace(oracle, dense["p"], dense["chain"], dense["planes"], classes, plane)
    got = compose(oracle, dense, classes=classes, gloss_plane=plane)
    for key in ("steps", "cones", "rgba32f"):
        assert same(got[key], want[key]), key
    assert same(got["frame16"], want["rgba16f"]) and got["total_steps"] == want["total_steps"]
    assert same(got["shininess"], lr.class_shininess(plane, classes))
    assert not same(got["cones"], dense["ref"]["cones"])


def test_sky_alone(oracle, dense):
    want = sr.trace(oracle, dense["p"], dense["chain"], dense["planes"], sr.SH)
    got = compose(oracle, dense, sky=sr.SH)
    for key in ("steps", "cones", "rgba32f"):
        assert same(got[key], want[key]), key
    assert same(got["frame16"], want["rgba16f"]) and got["total_steps"] == want["total_steps"]
    assert not same(got["cones"], dense["ref"]["cones"])


@pytest.mark.parametrize("mask", MASKS)
def test_lighting_components_alone(oracle, dense, mask):
    ref, p = dense["ref"], dense["p"]
    for aov in (0, ALL_AOV):
        cones = cr.masked_cones(ref["cones"], mask, aov)
        want = cr.composite(dense["planes"], cones, CAM, LIGHT, p.ambient_factor, p.shininess, mask)
        got = compose(oracle, dense, mask=mask, aov=aov)
        assert same(got["cones"], cones) and same(got["rgba32f"], want["rgba32f"])
        assert same(got["frame16"], cr.to_f16_bits(want["rgba32f"]))
        assert got["total_steps"] == cr.marched_steps(ref["steps"], mask, aov)
        dif, spc = cr.marched_groups(mask, aov)
        assert got["steps"][:, :6].any() == dif and got["steps"][:, 6].any() == spc
        if aov:
            assert same(got["outputs"][cr.AOV_INDIRECT_DIFFUSE], want["ind"])
            assert same(got["outputs"][cr.AOV_INDIRECT_SPECULAR], want["spec_cone"])
            assert same(got["outputs"][cr.AOV_DIRECT], want["direct"])


def test_outputs_alone_leave_the_frame_as_it_is(oracle, dense):
    got, ref = compose(oracle, dense, aov=ALL_AOV), dense["ref"]
    assert same(got["rgba32f"], ref["rgba32f"]) and same(got["cones"], ref["cones"])
    live = got["live"]
    assert same(got["outputs"][cr.AOV_INDIRECT_SPECULAR][live], ref["cones"][live, 6])
    assert same(got["outputs"][cr.AOV_INDIRECT_DIFFUSE][live], cr.gather(ref["cones"])[live])


def test_diffuse_rate_2_alone(oracle):
    """test_gpu_diffuse_rate's "mixed" case, at a size a CPU test affords."""
    w, h = 40, 24
    planes = drr.mixed_gbuffer(w, h)
    chain = oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.06))
    cam, light = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)
    p = oracle.default_params(V, camera_pos=cam, light_dir=light)
    ref = oracle.trace(p, chain, planes, nthreads=4, want_cones=True)
    s = dict(chain=chain, planes=planes, p=p, cache={})
    for mask, aov in ((cr.SHOW_ALL, 0), (MASKS[4], cr.AOV_INDIRECT_DIFFUSE), (MASKS[0], 0)):
        want = drr.restate(planes, w, h, f32(p.G) / f32(V), ref, cam, light, p.ambient_factor, p.shininess, mask, aov)
        got = compose(oracle, s, w, h, rate=2, mask=mask, aov=aov)
        for key in ("steps", "cones", "rgba32f", "marched"):
            assert same(got[key], want[key]), (mask, key)
        assert got["total_steps"] == want["total_steps"] and same(got["frame16"], cr.to_f16_bits(want["rgba32f"]))
        if aov:
            assert same(got["outputs"][cr.AOV_INDIRECT_DIFFUSE], want["ind"])
    full = compose(oracle, s, w, h)
    assert 0 < want["cls"]["marched"].sum() < full["live"].sum()


@pytest.fixture(scope="module")
def emitter(oracle):
    """The emitter-only set-up of test_gpu_lights.py and test_gpu_emission.py: shadow plane 0, specular planes 0."""
    w, h = 61, 43
    chain = oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.06))
    planes = synth.random_gbuffer(w * h, seed=21, discard_frac=0.05)
    planes[22] = 0.0
    planes[19:22] = 0.0
    r = np.random.default_rng(8)
    E = (r.normal(size=(3, w * h)) * r.choice([0.0, 0.5, 3.0, 1e4], size=(1, w * h))).astype(f32)
    cam, light = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)
    p = oracle.default_params(V, camera_pos=cam, light_dir=light)
    lights = [lr.point((10.0, 0.0, -20.0), (400.0, 300.0, 200.0), 60.0, 2.0),
              lr.spot((-40.0, 30.0, 20.0), (900.0, 900.0, 500.0), 80.0, 1.5, (1.0, -0.5, -0.3), 0.9, 0.3)]
    return dict(w=w, h=h, chain=chain, planes=planes, p=p, E=E, cam=cam, light=light, lights=lights, cache={},
                ref=oracle.trace(p, chain, planes, nthreads=4, want_cones=True))


def test_emission_planes_alone(oracle, emitter):
    s = emitter
    got = compose(oracle, s, s["w"], s["h"], emission=s["E"])
    want16 = er.frame(s["ref"]["rgba32f"], s["planes"], s["E"])
    assert same(got["frame16"], want16) and same(got["lit"], s["E"]) and same(got["rgba32f"], s["ref"]["rgba32f"])
    assert same(got["frame32"], want16.view(np.float16).astype(f32))
    assert same(got["cones"], s["ref"]["cones"]) and got["total_steps"] == s["ref"]["total_steps"]


def test_lights_alone(oracle, emitter):
    s = emitter
    lit = lr.lit_planes(s["planes"], s["lights"], s["cam"], s["p"].shininess)
    assert (lit[:, s["planes"][18] >= 0.5] > 0).any(0).sum() >= 100
    got = compose(oracle, s, s["w"], s["h"], lights=s["lights"])
    assert same(got["lit"], lit) and same(got["frame16"], er.frame(s["ref"]["rgba32f"], s["planes"], lit))
    # ... which is test_gpu_lights.test_frame_bit_for_bit's statement: the restated composite of the cones, plus the planes
    rgba = cr.composite(s["planes"], s["ref"]["cones"], s["cam"], s["light"], s["p"].ambient_factor, s["p"].shininess)["rgba32f"]
    assert same(got["frame16"], er.frame(rgba, s["planes"], lit))
    both = compose(oracle, s, s["w"], s["h"], lights=s["lights"], emission=s["E"])
    lit_E = lr.lit_planes(s["planes"], s["lights"], s["cam"], s["p"].shininess, E=s["E"])
    assert same(both["lit"], lit_E) and same(both["frame16"], er.frame(s["ref"]["rgba32f"], s["planes"], lit_E))


def test_a_row_range_selects_and_counts(oracle, dense):
    got = compose(oracle, dense, rows=(1, 2))
    y = np.arange(W * H) // W
    assert np.array_equal(got["sel"], (y >= 8) & (y < 16))
    assert got["total_steps"] == int(dense["ref"]["steps"][got["sel"]].astype(np.int64).sum())
    strided = compose(oracle, dense, rows=(0, 2), row_stride=2)
    assert np.array_equal(strided["sel"], y < 8)
