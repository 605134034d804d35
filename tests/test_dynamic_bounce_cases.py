"""CPU: the premises of tests/test_gpu_dynamic_bounce.py, from the oracle alone -- what the second bounce over the
dynamic mesh (tests/dynbouncecases.py) has to show at each scene, so that the GPU comparisons cannot pass vacuously.  The
figures in the comments are the oracle's; the assertions hold them as "at least"."""
import numpy as np
import pytest

import dynbouncecases as db
import dyncases as dc

V = dc.V


@pytest.fixture(scope="module")
def layers(oracle):
    w = dict(S=dc.layer(oracle, *dc.static_scene()))
    for k, C in (("A", dc.A), ("B", dc.B)):
        w[k] = dc.layer(oracle, *dc.dynamic_mesh(C))
    w["det"] = db.detached(oracle, w["S"])
    return w


@pytest.mark.parametrize("k, dyn_min, static_min", [("A", 540, 1398), ("B", 521, 1102)])
def test_object_positions(oracle, layers, k, dyn_min, static_min):
    """A: 99,071 steps expected, 99,060 with the static attributes only, 540 voxels differ, all dynamic; detached 84,359
    steps and 1,398 static voxels differ from it.  B: 98,400 / 98,457 / 84,359; 521 dynamic and 1,102 static voxels."""
    S3, D3 = layers["S"], layers[k]
    d = D3[0][..., 3] > 0
    want, steps = db.expected(oracle, D3, S3)
    wrong, wrong_steps = db.static_attributes(oracle, D3, S3)
    det, det_steps = layers["det"]
    diff = db.differing(want, wrong)
    static_moved = db.differing(want, det) & ~d
    occupied = int((dc.merge(D3[0], S3[0])[..., 3] > 0).sum())
    print(k, steps, wrong_steps, det_steps, int(diff.sum()), int((diff & d).sum()), int(static_moved.sum()), occupied)
    assert steps != wrong_steps and steps > det_steps + 10_000
    assert int(diff.sum()) >= dyn_min and not (diff & ~d).any()      # the owner's attributes matter, in dynamic voxels only
    assert int(static_moved.sum()) >= static_min                     # static voxels see the mover
    assert occupied < V ** 3 // 8                                    # the list form: k_bounce_march


def test_the_two_positions_differ(oracle, layers):
    a, _ = db.expected(oracle, layers["A"], layers["S"])
    b, _ = db.expected(oracle, layers["B"], layers["S"])
    n = int(db.differing(a, b).sum())
    print(n)
    assert n >= 2379
    # bricks only the object occupies, at either place: what it leaves has to come out clean
    for k, own in (("A", 3), ("B", 6)):
        assert dc.non_degeneracy(layers[k][0], layers["S"][0])["dynamic_only_bricks"] >= own


def test_the_big_object(oracle, layers):
    """512 dynamic bricks, 229 of them without a static slot; 177,541 occupied voxels (the list holds 32,768); one dynamic
    voxel with a zero normal; brick 0 dynamic; 2,216,734 steps against 2,042,392 with the static attributes."""
    S3 = layers["S"]
    D3 = dc.layer(oracle, *dc.big_triangles())
    d = D3[0][..., 3] > 0
    n = dc.non_degeneracy(D3[0], S3[0])
    occupied = int((dc.merge(D3[0], S3[0])[..., 3] > 0).sum())
    zero = int((d & db.zero_normal(D3[2])).sum())
    _, steps = db.expected(oracle, D3, S3)
    _, wrong_steps = db.static_attributes(oracle, D3, S3)
    print(n, occupied, zero, steps, wrong_steps)
    assert n["dynamic_bricks"] == (V // 8) ** 3 and n["dynamic_only_bricks"] >= 229
    assert occupied >= 177_541 > V ** 3 // 8                         # k_bounce_bricks<.., DYN> serves the overflow
    assert zero >= 1
    assert dc.bricks(d)[0, 0, 0]
    assert steps >= wrong_steps + 100_000


def test_dense_16(oracle):
    """3,901 of 4,096 voxels occupied (the list holds 512); 55 dynamic voxels across all 8 bricks; 27,730 steps against
    27,728 with the static attributes."""
    v = 16
    S3 = dc.layer(oracle, *db.dense16_static(), V=v)
    D3 = dc.layer(oracle, *dc.dynamic_mesh(dc.A), V=v)
    d = D3[0][..., 3] > 0
    p = oracle.default_params(v, G=dc.G)
    occupied = int((dc.merge(D3[0], S3[0])[..., 3] > 0).sum())
    want, steps = db.expected(oracle, D3, S3, p=p)
    wrong, wrong_steps = db.static_attributes(oracle, D3, S3, p=p)
    print(occupied, int(d.sum()), int(dc.bricks(d).sum()), steps, wrong_steps, int(db.differing(want, wrong).sum()))
    assert occupied >= 3901 > v ** 3 // 8
    assert int(d.sum()) >= 55 and int(dc.bricks(d).sum()) == 8
    assert steps != wrong_steps and int(db.differing(want, wrong).sum()) >= 10


# ---- the grids and march forms of tests/test_gpu_dynamic_features.py --------------------------------------------------------------
@pytest.mark.parametrize("v, differ_min", [(8, 10), (16, 50), (128, 1000)])
def test_other_grid_sizes(oracle, v, differ_min):
    """dyncases' world at A on 8^3 / 16^3 / 128^3: 12 / 55 / 1,311 voxels tell whose attributes shade the layer, and the step
    counts differ at all three sizes.  128^3 has 4,096 bricks: brick indices beyond 9 bits."""
    p = oracle.default_params(v, G=dc.G)
    S3, D3 = dc.layer(oracle, *dc.static_scene(), V=v), dc.layer(oracle, *dc.dynamic_mesh(dc.A), V=v)
    want, steps = db.expected(oracle, D3, S3, p=p)
    wrong, wrong_steps = db.static_attributes(oracle, D3, S3, p=p)
    n = int(db.differing(want, wrong).sum())
    print(v, n, steps, wrong_steps)
    assert n >= differ_min and steps != wrong_steps
    assert (v // 8) ** 3 > 512 or v < 64


@pytest.mark.parametrize("wrap", [1, 0])
@pytest.mark.parametrize("scene", ["world64", "dense16"])
def test_max_alpha_097_shows_in_the_bounce(oracle, layers, scene, wrap):
    """max_alpha 0.97 (1 - max_alpha < 2^-5: the IEEE-divide march): the bounce differs from the default constants' and
    still tells whose attributes shade the layer, in both wrap forms."""
    v = 64 if scene == "world64" else 16
    if scene == "world64":
        S3, D3 = layers["S"], layers["A"]
    else:
        S3, D3 = dc.layer(oracle, *db.dense16_static(), V=v), dc.layer(oracle, *dc.dynamic_mesh(dc.A), V=v)
        assert int((dc.merge(D3[0], S3[0])[..., 3] > 0).sum()) > v ** 3 // 8
    assert np.float32(1.0) - np.float32(0.97) < np.float32(2.0 ** -5)
    p = oracle.default_params(v, G=dc.G, wrap_repeat=wrap, max_alpha=0.97)
    want, steps = db.expected(oracle, D3, S3, p=p)
    wrong, wrong_steps = db.static_attributes(oracle, D3, S3, p=p)
    default, default_steps = db.expected(oracle, D3, S3, p=oracle.default_params(v, G=dc.G, wrap_repeat=wrap))
    print(scene, wrap, steps, wrong_steps, int(db.differing(want, wrong).sum()), int(db.differing(want, default).sum()))
    assert steps != wrong_steps and db.differing(want, wrong).sum() >= (300 if v == 64 else 10)
    # few cones of the sparse world pass alpha 0.95: the limit shows in the step count and in a handful of voxels
    assert steps > default_steps and db.differing(want, default).sum() >= 10
