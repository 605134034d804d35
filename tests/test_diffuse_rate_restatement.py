"""CPU: the half-rate diffuse gather (include/vct.h vct_set_diffuse_rate) -- its symbols and constants through the
layers, and the numpy restatement (tests/diffuse_rate_ref.py) against components_ref before any GPU test leans on it."""
import os

import numpy as np
import pytest

import components_ref as cr
import diffuse_rate_ref as dr
import synth
import vctpkg
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM, LIGHT = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)


def test_symbols_and_constants_through_the_layers():
    vct = vctpkg.load()
    for n in ("vct_set_diffuse_rate", "vct_get_diffuse_rate"):
        assert n in vct.ABI_SYMBOLS and hasattr(vct.lib(), n), n
    assert hasattr(vct.Context, "set_diffuse_rate") and hasattr(vct.Context, "diffuse_rate")
    facade = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "host", "Voxel_Cone_Tracing.h")).read()
    assert "int DiffuseRate = 1;" in facade and "vct_set_diffuse_rate(ctx, DiffuseRate)" in facade
    assert "--diffuse-rate" in open(os.path.join(ROOT, "voxel-cone-tracing_amd", "host", "demo_main.cpp")).read()
    hdr = dr.header_constants(os.path.join(ROOT, "include", "vct.h"))
    assert hdr == {"VCT_DIFFUSE_RATE_NORMAL_COS2": float(dr.NORMAL_COS2), "VCT_DIFFUSE_RATE_PLANE_TOL": float(dr.PLANE_TOL)}


@pytest.fixture(scope="module")
def mixed():
    V, w, h = 32, 48, 40
    chain = pyoracle.build_mips(synth.noise_volume(V, seed=5, occupancy=0.08))
    planes = dr.mixed_gbuffer(w, h)
    p = pyoracle.default_params(V, camera_pos=CAM, light_dir=LIGHT)
    ref = pyoracle.trace(p, chain, planes, nthreads=4, want_cones=True)
    return dict(w=w, h=h, vs=np.float32(p.G) / np.float32(V), planes=planes, p=p, ref=ref)


def _restate(s, mask=cr.SHOW_ALL, aov=0):
    return dr.restate(s["planes"], s["w"], s["h"], s["vs"], s["ref"], CAM, LIGHT, s["p"].ambient_factor, s["p"].shininess, mask, aov)


def test_marched_pixels_are_the_full_rate_composite(mixed):
    got = _restate(mixed)
    cls = got["cls"]
    for name in ("anchor", "fill"):
        assert cls[name].any(), name
    assert (cls["W"][~cls["marched"] & cls["alive"]] > 0).all() and not (cls["anchor"] & cls["fill"]).any()
    full = cr.composite(mixed["planes"], mixed["ref"]["cones"], CAM, LIGHT, mixed["p"].ambient_factor, mixed["p"].shininess)
    m = got["marched"] | ~cls["alive"]
    assert np.array_equal(got["rgba32f"][m], full["rgba32f"][m])
    assert np.array_equal(got["ind"][m], full["ind"][m])
    # interpolated pixels: a convex combination of anchors' gathers, so inside their range -- and not all equal to their own
    interp = cls["alive"] & ~cls["marched"]
    assert interp.any() and not np.array_equal(got["ind"][interp], full["ind"][interp])
    assert got["total_steps"] < mixed["ref"]["total_steps"]
    # every anchor position and the quad without a sample occur (mixed_gbuffer plants them)
    assert set(np.unique(cls["code"])) == {0, 1, 2, 3, dr.NO_ANCHOR}


def test_interpolation_of_equal_samples_is_that_sample(mixed):
    """S / W with all four candidates holding one value v is v wherever 9v, 12v, 15v and 16v are exact: integers here."""
    cls = dr.classify(mixed["planes"], mixed["w"], mixed["h"], mixed["vs"])
    cones = np.zeros((mixed["w"] * mixed["h"], 7, 4), np.float32)
    cones[:, 0, :] = 4.0                                       # gather = 0.25 * 4 = 1 exactly
    ind = dr.gather_rate2(cones, cls)
    assert np.array_equal(ind[cls["alive"]], np.ones_like(ind[cls["alive"]]))


def test_unrelated_neighbours_all_fill():
    """(Unrelated neighbours still pass the acceptance test by chance, about once in 200 pixels at this voxel size; size
    and seed are ones where none does.)"""
    w, h = 24, 16
    planes = synth.random_gbuffer(w * h, seed=1, discard_frac=0.1)
    cls = dr.classify(planes, w, h, np.float32(150.0) / np.float32(32))
    assert cls["anchor"].any()
    assert np.array_equal(cls["fill"], cls["alive"] & ~cls["anchor"])
    assert np.array_equal(cls["marched"], cls["alive"])


def test_skip_rule_marches_nothing(mixed):
    got = _restate(mixed, cr.SHOW_DIFFUSE | cr.SHOW_SPECULAR)
    assert not got["marched"].any() and got["total_steps"] == 0
    got = _restate(mixed, cr.SHOW_SPECULAR | cr.SHOW_INDIRECT_SPECULAR)
    assert not got["marched"].any() and got["total_steps"] == int(mixed["ref"]["steps"][:, 6].astype(np.int64).sum())
