"""CPU: the premises of tests/test_gpu_dynamic_emission.py, checked on the CPU oracle where there is no GPU -- with the
table of tests/dynemiscases.py the scenes of tests/dyncases.py at 64^3 saturate, add two non-zero terms, average several
materials in one voxel and keep voxels without any emission, so that a comparison with D' = D + DEm cannot pass vacuously."""
import numpy as np
import pytest

import dyncases as dc
import dynemiscases as de


@pytest.fixture(scope="module")
def static(oracle):
    return dc.layer(oracle, *dc.static_scene())[0]


# (dynamic voxels, D + DEm saturates, both terms non-zero, means of several materials, all-zero DEm) as the oracle counts them
FIGURES = {"A": (540, 374, 390, 10, 150), "B": (521, 352, 370, 11, 151)}


@pytest.mark.parametrize("name", ["A", "B"])
def test_positions_are_not_degenerate_for_the_emission_rule(oracle, static, name):
    pos, mat, alb = dc.dynamic_mesh(getattr(dc, name))
    D = dc.layer(oracle, pos, mat, alb)[0]
    DEm = de.dem(oracle, pos, mat)
    n = de.assert_non_degenerate(D, DEm)
    print(name, n)
    want = FIGURES[name]
    assert (n["dynamic_voxels"], n["saturating"], n["both"], n["mixed_values"], n["zero_emission"]) == want, n
    # the same fragments: DEm is occupied exactly where D is, and D' keeps D's alpha
    Dp = de.add(D, DEm)
    assert np.array_equal(Dp[..., 3], D[..., 3]) and (Dp != D).any(-1).sum() >= 300
    assert np.array_equal(Dp[(DEm[..., :3] == 0).all(-1)], D[(DEm[..., :3] == 0).all(-1)])
    # the emitters meet the static mesh: the merged chain differs from merge(D, S) in voxels both meshes occupy
    shared = (D[..., 3] > 0) & (static[..., 3] > 0)
    assert shared.sum() >= 30 and (dc.merge(Dp, static) != dc.merge(D, static)).any(-1).sum() >= 300
    # the shadow map does not enter DEm: the layer changes under a map, DEm is formed without one by definition
    assert (DEm[..., :3] > 0).any(-1).sum() >= 350


def test_a_table_on_one_material_lights_fewer_voxels(oracle):
    pos, mat, alb = dc.dynamic_mesh(dc.A)
    all_, one = de.dem(oracle, pos, mat, de.EM), de.dem(oracle, pos, mat, de.ONE)
    lit_all, lit_one = (all_[..., :3] > 0).any(-1), (one[..., :3] > 0).any(-1)
    assert lit_one.sum() >= 100 and (lit_all & ~lit_one).sum() >= 100 and not (lit_one & ~lit_all).any()


def test_big_triangles_are_not_degenerate_for_the_emission_rule(oracle):
    pos, mat, alb = dc.big_triangles()
    D = dc.layer(oracle, pos, mat, alb)[0]
    DEm = de.dem(oracle, pos, mat)
    n = de.non_degeneracy(D, DEm)
    print("big", n)
    assert n["same_alpha"] and n["dynamic_voxels"] == 177219, n
    assert n["saturating"] >= 100000 and n["both"] >= 100000 and n["mixed_values"] >= 500, n
    assert (n["saturating"], n["both"], n["mixed_values"]) == (128025, 149506, 586), n


# ---- the other grid sizes of tests/test_gpu_dynamic_features.py -----------------------------------------------------------------
# v: ((D' != D) voxels, D + DEm saturates, the ONE table's D' differs from EM's) at A, the bounds the GPU tests assert
GRID_FIGURES = {8: (10, 9, 9), 16: (40, 30, 36), 128: (917, 907, 485)}


@pytest.mark.parametrize("v", sorted(GRID_FIGURES))
def test_other_grid_sizes_are_not_degenerate_for_the_emission_rule(oracle, v):
    """One brick (8^3), eight bricks (16^3) and 128^3: fewer voxels than at 64^3, still saturating ones and a table on one
    material that shows.  At 128^3 the bounds of assert_non_degenerate hold as they stand."""
    pos, mat, alb = dc.dynamic_mesh(dc.A)
    D = dc.layer(oracle, pos, mat, alb, V=v)[0]
    DEm, one = de.dem(oracle, pos, mat, V=v), de.dem(oracle, pos, mat, de.ONE, V=v)
    assert D.shape == DEm.shape == (v, v, v, 4)
    n = de.non_degeneracy(D, DEm)
    Dp, Dq = de.add(D, DEm), de.add(D, one)
    figures = (int((Dp != D).any(-1).sum()), n["saturating"], int((Dq != Dp).any(-1).sum()))
    print(v, figures, n)
    assert n["same_alpha"] and all(f >= lo for f, lo in zip(figures, GRID_FIGURES[v])), (figures, n)
    if v == 128:
        de.assert_non_degenerate(D, DEm)
