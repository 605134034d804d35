"""CPU: the premises of tests/test_gpu_dynamic_skin.py, checked on the CPU oracle where there is no GPU -- the influences
of tests/dynskincases.py are as described, skin_ref pins the operation order, a single full weight is the rigid transform,
every pose is inside the vertex contract and fits (or, where meant, exceeds) the capacities the GPU tests pass, and the bad
matrices remove some triangles and leave others."""
import numpy as np
import pytest

import dyncases as dc
import dynpartcases as dp
import dynskincases as ds


def posed(ntri, name):
    pos, mat, alb = ds.mesh(ntri)
    return ds.skin_ref(pos, *ds.influences(ntri), ds.pose(name)), mat, alb


def test_the_influences_are_as_described():
    for ntri in ds.SIZES:
        bone, weight = ds.influences(ntri)
        assert bone.dtype == np.int32 and weight.dtype == np.float32 and bone.shape == weight.shape == (ntri, 3, 4)
        assert bone.min() >= 0 and bone.max() < ds.UNNAMED and np.isfinite(weight).all()
        assert not ds.names(bone, ds.UNNAMED).any()
        # a slot with weight 0 points at the corner's first bone, which carries weight
        unused = weight == 0
        assert (bone[unused] == np.broadcast_to(bone[..., :1], bone.shape)[unused]).all() and (weight[..., 0] != 0).all()
    bone, weight = ds.influences(150)
    wave = slice(0, 64)
    kinds = (weight[wave] != 0).sum(-1)
    assert set(np.unique(kinds).tolist()) == {1, 2, 4}
    # triangles of the first wave whose three corners use three different bone sets
    sets = [[frozenset(bone[t, v][weight[t, v] != 0].tolist()) for v in range(3)] for t in range(64)]
    assert sum(len(set(s)) == 3 for s in sets) >= 20
    sums = weight.astype(np.float64).sum(-1)
    assert abs(sums[ds.SUM_09] - 0.9) < 1e-6 and abs(sums[ds.SUM_11] - 1.1) < 1e-6
    assert weight[ds.NEGATIVE].tolist() == [1.25, -0.25, 0.0, 0.0] and (weight < 0).sum() == 1
    others = np.ones(sums.shape, bool)
    for k in (ds.SUM_09, ds.SUM_11):
        others[k] = False
    assert np.abs(sums[others] - 1.0).max() < 1e-6
    assert all(ds.names(bone, k).sum() >= 10 for k in range(5))


@pytest.mark.parametrize("ntri", ds.SIZES)
def test_a_fused_skin_would_differ_on_every_non_identity_pose(ntri):
    """Without this the operation order would not be pinned (here 424 and 411 of 1350 coordinates at 150 triangles, 2 and 3
    of 9 for the single triangle).  On the identity pose every product is w * 1 or w * 0, exact, and the two agree."""
    pos = ds.mesh(ntri)[0]
    bone, weight = ds.influences(ntri)
    for name in ("P1", "P2"):
        a, b = ds.skin_ref(pos, bone, weight, ds.pose(name)), ds.skin_fused(pos, bone, weight, ds.pose(name))
        assert (a.view(np.uint32) != b.view(np.uint32)).sum() >= (1 if ntri == 1 else 10), (ntri, name)
        assert np.allclose(a, b, rtol=1e-4, atol=1e-2), (ntri, name)
    assert (ds.skin_ref(pos, bone, weight, ds.pose("P1")) != pos).any()


def test_one_full_weight_is_the_rigid_transform():
    """Weights (1, 0, 0, 0) and finite matrices: B = ((1 * M0 + 0 * M1) + 0 * M2) + 0 * M3 has M0's values, so the corner is
    dynpartcases.transform_ref's -- compared with ==, which takes -0 and +0 as equal: the sign of a zero may differ
    (-0 + 0 * M1[j] is +0 where the product is +0)."""
    pos = ds.mesh(150)[0]
    r = np.random.default_rng(5)
    lead = r.integers(0, ds.NBONES, 150).astype(np.int32)                  # one bone per triangle, as a part
    bone = r.integers(0, ds.NBONES, (150, 3, 4)).astype(np.int32)          # the other slots name any bone, weight 0
    bone[..., 0] = lead[:, None]
    weight = np.zeros((150, 3, 4), np.float32)
    weight[..., 0] = 1.0
    for name in ds.POSES:
        got, want = ds.skin_ref(pos, bone, weight, ds.pose(name)), dp.transform_ref(pos, lead, ds.pose(name))
        assert (got == want).all(), name


@pytest.mark.parametrize("ntri", ds.SIZES)
def test_every_pose_is_inside_the_contract_and_fits_the_capacity(oracle, ntri):
    need = {}
    for name in ds.POSES + ("PX",):
        pos, mat, alb = posed(ntri, name)
        assert ds.in_contract(pos).all(), (ntri, name)
        D = dc.layer(oracle, pos, mat, alb)[0]
        need[name] = int(dc.bricks(D[..., 3] > 0).sum())
        assert need[name] >= 1
    assert all(need[name] <= ds.MAX_BRICKS for name in ds.POSES), need
    if ntri == 150:
        assert need["P0"] <= ds.SMALL_CAPACITY and need["PX"] == ds.SMALL_CAPACITY + ds.OVER, need
        # the poses differ from one another in the layer
        L = [dc.layer(oracle, *posed(150, name))[0] for name in ds.POSES]
        assert all((L[a] != L[b]).any(-1).sum() >= 100 for a, b in ((0, 1), (0, 2), (1, 2)))


def test_the_mirrored_bone_mirrors():
    M = ds.pose_f64("P2")
    dets = [np.linalg.det(M[k, :, :3]) for k in range(ds.NBONES)]
    assert dets[0] < 0 and all(d > 0.99 for d in dets[1:])


def test_the_bad_matrices_remove_some_triangles_and_leave_others(oracle):
    pos, mat, alb = ds.mesh(150)
    bone, weight = ds.influences(150)
    out = ds.skin_ref(pos, bone, weight, ds.bad_matrices())
    gone = ds.names(bone, ds.NAN_BONE) | ds.names(bone, ds.INF_BONE)
    assert np.array_equal(~ds.in_contract(out), gone) and 1 <= gone.sum() < 150 and (~gone).sum() >= 20
    keep = ~gone
    assert np.array_equal(out[keep].view(np.uint32), ds.skin_ref(pos, bone, weight, ds.pose("P1"))[keep].view(np.uint32))
    assert (dc.layer(oracle, out[keep], mat[keep], alb)[0][..., 3] > 0).sum() >= 50


def test_a_zero_weight_on_a_bad_bone_removes_the_triangle():
    """dynskincases.zero_weight_case: the definition evaluates all four terms, and 0 * NaN -- like 0 * inf -- is NaN."""
    pos = ds.mesh(150)[0]
    bone, weight, t, m = ds.zero_weight_case()
    assert weight[t, 2, 3] == 0 and bone[t, 2, 3] == ds.UNNAMED and ds.names(bone, ds.UNNAMED).sum() == 1
    out = ds.skin_ref(pos, bone, weight, m)
    assert np.array_equal(~ds.in_contract(out), np.arange(150) == t)
    m[ds.UNNAMED, 0] = np.float32(np.inf)
    assert np.array_equal(~ds.in_contract(ds.skin_ref(pos, bone, weight, m)), np.arange(150) == t)
