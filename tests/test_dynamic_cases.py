"""CPU: the premises of tests/test_gpu_dynamic.py, checked on the CPU oracle where there is no GPU -- the scenes of
tests/dyncases.py are not degenerate for the merge rule level0 = where(D.a > 0, D, S)."""
import numpy as np
import pytest

import dyncases as dc
import voxcases
from test_gpu_parity import light_setup


@pytest.fixture(scope="module")
def static(oracle):
    return dc.layer(oracle, *dc.static_scene())


@pytest.mark.parametrize("name", ["A", "B"])
def test_positions_are_not_degenerate(oracle, static, name):
    S = static[0]
    D, Da, Dn = dc.layer(oracle, *dc.dynamic_mesh(getattr(dc, name)))
    n = dc.assert_non_degenerate(D, S)
    # the figures of the two positions: several hundred dynamic voxels in about a dozen bricks, a few
    # of them dynamic-only, and well over a hundred static-only voxels inside the shared bricks
    assert 400 <= n["dynamic_voxels"] <= 700 and n["both_differ"] >= 30, n
    assert n["dynamic_only_bricks"] >= 3 and n["shared_bricks"] >= 5 and n["static_only_in_shared"] >= 140, n
    assert n["dynamic_bricks"] == n["dynamic_only_bricks"] + n["shared_bricks"]
    # attributes are occupied exactly where the layer is
    assert np.array_equal(Da[..., 3] == 255, D[..., 3] > 0) and np.array_equal(Dn[..., 3] == 255, D[..., 3] > 0)
    merged = dc.merge(D, S)
    assert (merged != S).any() and (merged != D).any()
    assert np.array_equal(merged[D[..., 3] > 0], D[D[..., 3] > 0]) and np.array_equal(merged[D[..., 3] == 0], S[D[..., 3] == 0])


def test_the_two_positions_do_not_share_a_brick(oracle):
    """Moving A -> B leaves every brick of A: the next pass has to clean all of them."""
    DA = dc.layer(oracle, *dc.dynamic_mesh(dc.A))[0]
    DB = dc.layer(oracle, *dc.dynamic_mesh(dc.B))[0]
    assert not (dc.bricks(DA[..., 3] > 0) & dc.bricks(DB[..., 3] > 0)).any()
    # B fits the default capacity reserved at A (twice A's bricks, at least 64)
    assert dc.bricks(DB[..., 3] > 0).sum() <= max(64, 2 * dc.bricks(DA[..., 3] > 0).sum())


def test_the_shadow_map_changes_the_layer(oracle):
    depth, vp = light_setup(128, 9)
    pos, mat, alb = dc.dynamic_mesh(dc.A)
    lit = dc.layer(oracle, pos, mat, alb)[0]
    shadowed = dc.layer(oracle, pos, mat, alb, depth=depth, vp=vp)[0]
    assert np.array_equal(lit[..., 3], shadowed[..., 3]) and (lit != shadowed).any(-1).sum() >= 100


@pytest.mark.parametrize("name", list(voxcases.EDGE_CASES))
def test_edge_cases_as_dynamic_meshes_occupy_something(oracle, name):
    pos, mat, alb, ms, G, V = voxcases.EDGE_CASES[name]()
    L = dc.layer(oracle, pos, mat, alb, ms, G, V)[0]
    assert (L[..., 3] > 0).any()
    assert pos.shape[0] <= 1 << 20 and mat.max() < alb.shape[0]
