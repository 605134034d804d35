"""CPU: the inputs of tests/test_gpu_point_query.py (tests/pqcases.py) are what they are meant to be, and the reference
module (tests/point_query_ref.py) agrees with itself, before a GPU sees either.  Passes with or without the feature.

What is proven about the sampler path of a wave of 64 consecutive points (csrc/vct_trace.hip sample_level takes the
cooperative 4x4x4 block when every live lane's footprint corner lies within +-1 texel of the anchor lane's on every axis):
  * patch: 16 columns at vs / 4 span 3.75 texels of level 0, so a level-0 sample of a full wave spans 3 or 4 corners and
    CANNOT fit one block -- those samples (the first step's finer level) take the per-lane gather.  Every sample of a
    level >= 2 (five of a cone's eight samples) spans at most 1 corner per axis: it fits whichever lanes are still live,
    whichever of them is the anchor.  Level 1 spans at most 2: it fits when the anchor is in the middle.  At least one of
    the blocks that provably fit holds a non-zero texel, so the LDS gather runs, not only the all-zero short cut.
  * scatter: in every wave, at every step and level below the coarsest two, some sample spans more than 2 corners: no
    block can hold it, the per-lane gather runs.
  * mixed: the same points as patch in another order.
  * edge: every point is inside the point contract; the oracle's gather is NaN for exactly the points declared non-finite,
    each of their cones took one step, and the other points are finite."""
import numpy as np
import pytest

import pqcases as pc
import point_query_ref as pq


@pytest.fixture(scope="module")
def chain(oracle):
    return oracle.build_mips(pc.level0())


def params(oracle, wrap=1):
    return oracle.default_params(pc.V, G=pc.G, max_distance=pc.MAX_DISTANCE, wrap_repeat=wrap)


def test_step_table_restatement(oracle):
    p = params(oracle)
    for tan in (pc.TAN_DIFFUSE, pc.TAN_SPECULAR):
        n, last_lod = oracle.max_steps(p, float(tan))
        tab = pc.step_table(tan)
        assert len(tab) == n
        assert tab[-1][1][0] == int(np.floor(last_lod))
    assert [lv for _, lv in pc.step_table(pc.TAN_DIFFUSE)] == [[0, 1], [1, 2], [2, 3], [3, 4]]


def test_patch_is_served_by_the_cooperative_block(oracle, chain):
    pts = pc.patch()
    assert pts.shape == (256, 12)
    d = np.diff(pts[:16, 0].astype(np.float64))
    assert np.allclose(d, float(pc.VS) / 4, rtol=1e-5) and np.allclose(pts[16, 2] - pts[0, 2], float(pc.VS) / 4, rtol=1e-4)
    rows = pc.wave_spreads(oracle, pts)
    assert {r["wave"] for r in rows} == {0, 1, 2, 3}
    nonzero = 0
    for r in rows:
        if r["level"] == 0:
            assert r["spread"] >= 3, r
        elif r["level"] == 1:
            assert r["spread"] <= 2, r
        else:
            assert r["spread"] <= 1, r
            N = pc.V >> r["level"]
            lv = oracle.level_view(chain, pc.V, r["level"])
            ix = [(r["anchor"][a] - 1 + np.arange(4)) % N for a in range(3)]
            nonzero += bool(lv[np.ix_(ix[2], ix[1], ix[0])].any())
    assert nonzero > 0
    share = np.mean([r["level"] >= 2 for r in rows])
    assert share == 5 / 8          # of a cone's eight level samples


def test_scatter_takes_the_per_lane_gather(oracle):
    pts = pc.scatter()
    assert pts.shape[0] == 256 and (np.abs(pts[:, 0:3]) <= 0.45 * pc.G).all()
    rows = pc.wave_spreads(oracle, pts)
    for r in rows:
        if r["level"] <= 2:
            assert r["spread"] > 2, r
    for w in range(4):
        assert any(r["spread"] > 2 for r in rows if r["wave"] == w)


def test_mixed_is_patch_in_another_order():
    a, b = pc.patch(), pc.mixed()
    assert not np.array_equal(a, b)
    assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])])
    assert np.array_equal(pc.mixed(), b)          # a fixed permutation


@pytest.mark.parametrize("wrap", [1, 0])
def test_edge_classes(oracle, chain, wrap):
    pts, cls = pc.edge()
    assert not pc.exceeds_position_bound(pts).any()
    ref = pq.gather(oracle, params(oracle, wrap), chain, pts)
    nan = np.isnan(ref["gather"]).any(1)
    assert np.array_equal(nan, cls == pc.NONFINITE)
    assert nan.sum() >= 40 and (~nan).sum() >= 40
    assert np.isfinite(ref["gather"][~nan]).all()
    # a non-finite start or frame: at least one cone took its one step and returned NaN
    assert ((ref["steps"][nan] == 1) & np.isnan(ref["cones"][nan]).all(2)).any(1).all()
    # the last float inside the bound is there, and one float further is outside
    P = pts[:, 0:3].astype(np.float64)
    far = np.abs(P[np.isfinite(P)]).max()
    assert far > (pc.gc.LIMIT_GRIDS * pc.G) * (1 - 1e-6)
    cones = pc.edge_cones()
    reach = np.maximum(1.0, np.nan_to_num(np.linalg.norm(cones[:, 6:9].astype(np.float64), axis=1), nan=1.0, posinf=1.0))
    assert not pc.exceeds_position_bound(cones, reach).any()
    assert (cones[:, 6:9] == 0).all(1).sum() >= 8          # zero directions, +0 and -0


@pytest.mark.parametrize("wrap", [1, 0])
@pytest.mark.parametrize("name", pc.CASES)
def test_the_two_oracle_routes_agree(oracle, chain, name, wrap):
    """oracle.cone along cone i's direction, formed in fp32 as cone_dir forms it, is column i of oracle.trace."""
    p = params(oracle, wrap)
    pts = pc.get(name)[::5]
    ref = pq.gather(oracle, p, chain, pts)
    dirs = pq.cone_dirs(oracle, pts)
    for i in range(6):
        one = pq.cones(oracle, p, chain, pq.cone_points_of(pts, dirs[:, i]), float(pc.TAN_DIFFUSE))
        pq.assert_floats_match(one["cone"], ref["cones"][:, i], f"{name} cone {i}")
        assert np.array_equal(one["steps"], ref["steps"][:, i]), f"{name} cone {i}: steps"
    assert ref["total_steps"] == int(ref["steps"].astype(np.int64).sum())


def test_take_repeats_cyclically():
    pts = pc.patch()
    assert np.array_equal(pc.take(pts, 257)[256], pts[0]) and pc.take(pts, 63).shape == (63, 12)
    assert pc.SIZES == (1, 63, 64, 65, 257)
