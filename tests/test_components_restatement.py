"""CPU: the numpy restatement of the lighting-component composite (tests/components_ref.py) against the oracle, before
any GPU test leans on it, and the VCT_SHOW_* / VCT_AOV_* values of include/vct.h against the binding's."""
import os

import numpy as np
import pytest

import components_ref as cr
import synth
import vctpkg
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(kind):
    V = 32
    chain = pyoracle.build_mips(synth.noise_volume(V, seed=5, occupancy=0.08))
    if kind == "random":
        planes = synth.random_gbuffer(48 * 40, seed=9, discard_frac=0.1)
    else:
        planes = synth.coherent_gbuffer(48, 40, seed=4)
    p = pyoracle.default_params(V, camera_pos=(3.0, 4.0, -2.0), light_dir=(0.2, 1.0, 0.3))
    return p, chain, planes


@pytest.mark.parametrize("kind", ["random", "coherent"])
def test_restatement_show_all_is_the_oracle_composite(kind):
    p, chain, planes = _inputs(kind)
    ref = pyoracle.trace(p, chain, planes, nthreads=4, want_cones=True)
    got = cr.composite(planes, ref["cones"], tuple(p.camera_pos), tuple(p.light_dir), p.ambient_factor, p.shininess,
                       cr.SHOW_ALL)
    assert synth.rel_l2(got["rgba32f"], ref["rgba32f"]) <= 1e-6
    assert (cr.to_f16_bits(got["rgba32f"]) == ref["rgba16f"]).mean() >= 0.999
    assert (got["ind"][~got["alive"]] == 0).all() and (got["direct"][~got["alive"]] == 0).all()


def test_restatement_masks_select_terms():
    p, chain, planes = _inputs("coherent")
    ref = pyoracle.trace(p, chain, planes, nthreads=4, want_cones=True)
    args = (planes, ref["cones"], tuple(p.camera_pos), tuple(p.light_dir), p.ambient_factor, p.shininess)
    none = cr.composite(*args, mask=0)["rgba32f"]
    alb = planes[15:18].T
    assert np.allclose(none[:, :3], np.float32(p.ambient_factor) * alb, rtol=1e-6)     # ambient alone, occlusion 1
    # a group no term reads does not change the frame when its cones are zeroed (the skip rule)
    for mask in range(32):
        a = cr.composite(*args, mask=mask)["rgba32f"]
        b = cr.composite(planes, cr.masked_cones(ref["cones"], mask), *args[2:], mask=mask)["rgba32f"]
        assert np.array_equal(a, b), mask


def test_skip_rule_step_counts():
    steps = np.array([[1, 2, 3, 4, 5, 6, 7]], np.uint8)
    assert cr.marched_steps(steps, cr.SHOW_DIFFUSE | cr.SHOW_SPECULAR) == 0
    assert cr.marched_steps(steps, cr.SHOW_SPECULAR | cr.SHOW_INDIRECT_SPECULAR) == 7
    assert cr.marched_steps(steps, cr.SHOW_ALL) == 28
    assert cr.marched_steps(steps, cr.SHOW_AMBIENT_OCCLUSION) == 21
    assert cr.marched_steps(steps, 0, cr.AOV_INDIRECT_SPECULAR) == 7


def test_header_constants_match_binding():
    vct = vctpkg.load()
    hdr = cr.header_constants(os.path.join(ROOT, "include", "vct.h"))
    names = ["SHOW_DIFFUSE", "SHOW_INDIRECT_DIFFUSE", "SHOW_SPECULAR", "SHOW_INDIRECT_SPECULAR", "SHOW_AMBIENT_OCCLUSION",
             "SHOW_ALL", "AOV_INDIRECT_DIFFUSE", "AOV_INDIRECT_SPECULAR", "AOV_DIRECT"]
    for n in names:
        assert hdr["VCT_" + n] == getattr(vct, n) == getattr(cr, n), n
    assert set(hdr) == {"VCT_" + n for n in names}
    for n in ("vct_set_lighting_components", "vct_get_lighting_components", "vct_set_aov_outputs", "vct_download_aov",
              "vct_get_aov_device"):
        assert n in vct.ABI_SYMBOLS and hasattr(vct.lib(), n)
