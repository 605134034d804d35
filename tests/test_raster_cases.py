"""The CPU side of the adversarial raster cases (tests/geomcases.py) -- no GPU: the inputs are proven here before a
GPU sees them.

1. Every case reaches the decision points it is named for (the float64 classifier's counts against the case's stated
   minimum), the CPU checker rasterises it, and gives no non-finite value.
2. The CPU checker (oracle/vct_oracle_raster.cpp) against the independent float64 ray caster (tests/raster_f64.py):
   outside the left-out set (at most 2 % of the frame, asserted) the covered mask and the visible triangle are
   identical, world position and shadow-map depth within the bars.  Measured checker-vs-ray-caster errors (positions
   per plane as a fraction of the scene extent, depth as a fraction of the depth range) and the bars = 4 x measured
   (never below 4 x 2^-23) have ONE source, the table raster_f64.RC_MEASURED; DESIGN.md 4.1 prints the same table and
   test_design_md_shows_the_measured_table keeps the two from drifting apart.
   The GPU test (test_gpu_raster_edges.py) holds the library to the same bars; they do not come from the GPU.
3. Watertightness without any reference: a rectangle as 2 triangles and as 280 covers the same pixels, each once.
"""
import numpy as np
import pytest

import geomcases
import raster_f64
import raster_oracle


@pytest.mark.parametrize("name", geomcases.CASE_NAMES)
def test_case_reaches_its_decision_points_and_the_checker_draws_it(name):
    case = geomcases.get_case(name)
    cls = geomcases.check_minimum(case)
    print(name, {k: v for k, v in cls["counts"].items() if v})
    for mips in ((True, False) if case.textures else (True,)):
        depth, planes = raster_oracle.case_reference(case, mips)
        assert np.isfinite(depth).all() and np.isfinite(planes).all()
        assert ((depth >= 0.0) & (depth <= 1.0)).all()
        covered = (planes[18] >= 0.5).reshape(case.h, case.w)
        # the classifier counts coverage without the depth range and the alpha test: the checker can only show less
        assert not (covered & (cls["cover_count"] == 0)).any()
        if name not in ("depth_planes", "single_triangle_1x1") and not case.textures:
            assert np.array_equal(covered, cls["cover_count"] > 0)
    if case.aligned and not case.textures:
        # exact inputs: a pixel exactly one triangle claims shows that triangle
        own = geomcases.owner_of(planes, case.w, case.h)
        once = (cls["cover_count"] == 1) & covered
        for y, x in np.argwhere(once)[:: max(1, once.sum() // 200)]:
            assert own[y, x] in cls["pix_tris"][(y, x)], geomcases.verdict(cls, y, x)


@pytest.mark.parametrize("name", raster_f64.RC_NAMES)
def test_checker_against_the_float64_ray_caster(name):
    case = raster_f64.rc_case(name)
    depth, planes = raster_oracle.case_reference(case)
    raster_f64.check_against_ray_caster(name, planes, depth, "checker")


def test_ray_caster_scenes_are_not_empty():
    for name in raster_f64.RC_NAMES:
        (a, skip), _ = raster_f64.rc_truth(name)
        assert ((a["tri"] >= 0) & ~skip).mean() > 0.15, name


def test_checker_is_watertight_on_a_subdivided_rectangle():
    geomcases.check_watertight(lambda case: raster_oracle.case_reference(case)[1])


def test_design_md_shows_the_measured_table():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    for name, ((px, py, pz), d) in raster_f64.RC_MEASURED.items():
        row = f"| {name} | {px:.3g} | {py:.3g} | {pz:.3g} | {d:.3g} |"
        assert row in text, row
