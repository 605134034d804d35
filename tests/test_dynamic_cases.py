"""CPU: the premises of tests/test_gpu_dynamic.py and tests/test_gpu_dynamic_forms.py, checked on the CPU oracle where
there is no GPU -- the scenes of tests/dyncases.py are not degenerate for the merge rule level0 = where(D.a > 0, D, S)."""
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


# ---- the premises of tests/test_gpu_dynamic_forms.py ----------------------------------------------------------------------
def test_the_plain_voxelizer_gives_the_attribute_voxelizer_s_level_0(oracle):
    """A context without voxel attributes is held against voxelize_conservative: the same level 0 as element 0 of
    voxelize_conservative_attr, for every mesh the forms file attaches, without a shadow map and under the raised one."""
    from test_gpu_dynamic import RAISED, shadow_maps
    depth, vp = shadow_maps()[RAISED]
    meshes = dict(static=dc.static_scene(), A=dc.dynamic_mesh(dc.A), B=dc.dynamic_mesh(dc.B), big=dc.big_triangles())
    for name, m in meshes.items():
        for kw in ({}, dict(depth=depth, vp=vp)):
            assert np.array_equal(dc.layer_plain(oracle, *m, **kw), dc.layer(oracle, *m, **kw)[0]), (name, sorted(kw))
    for name in ("whole_grid_and_a_crowded_brick", "degenerate_triangles"):
        pos, mat, alb, ms, G, V = voxcases.EDGE_CASES[name]()
        assert np.array_equal(dc.layer_plain(oracle, pos, mat, alb, ms, G, V), dc.layer(oracle, pos, mat, alb, ms, G, V)[0]), name


def test_big_triangles_outnumber_the_workgroups_of_the_big_kernel(oracle, static):
    """By the library's own box rule (dc.box_candidates restates tri_candidates): 557 triangles go to k_dyn_big, whose grid
    is capped at 512 workgroups, so its grid-stride loop takes a second trip several workgroups wide; 43 stay with
    k_dyn_tris.  The layer occupies every brick of the 64^3 grid."""
    pos, mat, alb = dc.big_triangles()
    cnt = dc.box_candidates(pos)
    big, small = int((cnt > dc.VOX_BIG).sum()), int(((cnt > 0) & (cnt <= dc.VOX_BIG)).sum())
    assert big >= 530 and small >= 20, (big, small)
    D = dc.layer(oracle, pos, mat, alb)[0]
    n = dc.non_degeneracy(D, static[0])
    assert n["dynamic_bricks"] == (dc.V // 8) ** 3 == 512 and n["dynamic_voxels"] >= 170000 and n["both_differ"] >= 2000, n
    assert n["shared_bricks"] >= 200 and n["static_only_in_shared"] >= 300, n
    # moved by +300 in x: another layer, still mostly big triangles
    moved = pos.reshape(-1, 3, 3).copy()
    moved[..., 0] += np.float32(300.0)
    moved = moved.reshape(-1, 9)
    assert int((dc.box_candidates(moved) > dc.VOX_BIG).sum()) >= 530
    Dm = dc.layer(oracle, moved, mat, alb)[0]
    assert (Dm != D).any(-1).sum() >= 100000 and dc.non_degeneracy(Dm, static[0])["both_differ"] >= 2000


def test_the_box_rule_on_hand_made_triangles():
    """dc.box_candidates on boxes known by construction (V = 64, G = 150, model scale 0.05: a voxel is 46.875 model units)."""
    u = 46.875
    tri = lambda a, b: np.array([a[0], a[1], a[2], b[0], a[1], a[2], a[0], b[1], b[2]], np.float32) * np.float32(u)
    pos = np.stack([tri((0.25, 0.25, 0.25), (3.75, 2.75, 1.75)),          # voxels 32..35 x 32..34 x 32..33
                    tri((0.25, 0.25, 0.25), (0.25, 0.25, 0.25)),          # a point: no normal
                    tri((40.0, 0.25, 0.25), (50.0, 2.75, 0.25)),          # beyond +x
                    tri((-40.0, -40.0, 0.5), (40.0, 40.0, 0.5))])         # the whole grid in x and y, clipped
    assert dc.box_candidates(pos).tolist() == [4 * 3 * 2, 0, 0, 64 * 64 * 1]


GRID_FIGURES = {8: ((1, 9, 0), (1, 5, 0)), 16: ((8, 17, 0), (1, 13, 0)), 128: ((55, 36, 38), (49, 39, 36)),
                256: ((172, 38, 147), (178, 49, 155))}       # V -> (bricks, both_differ, dynamic-only bricks) at A and at B


@pytest.mark.parametrize("v", list(GRID_FIGURES))
def test_other_grid_sizes_are_not_degenerate(oracle, v):
    """The scenes at 8^3 (one brick), 16^3 (eight), 128^3 and 256^3 (brick indices beyond 9 bits): at the large grids the
    conditions of 64^3; at the small ones no brick can be dynamic-only, and the two meshes still meet and differ."""
    S = dc.layer(oracle, *dc.static_scene(), V=v)[0]
    for name, want in zip("AB", GRID_FIGURES[v]):
        D = dc.layer(oracle, *dc.dynamic_mesh(getattr(dc, name)), V=v)
        n = dc.non_degeneracy(D[0], S)
        assert (n["dynamic_bricks"], n["both_differ"], n["dynamic_only_bricks"]) == want, (v, name, n)
        if v >= 128:
            dc.assert_non_degenerate(D[0], S)
            assert n["dynamic_bricks"] > 64 or 2 * n["dynamic_bricks"] > 64      # the default capacity is 2 * need, not the floor
        else:
            assert n["both_differ"] >= 5 and n["static_only_in_shared"] >= 50, (v, name, n)
        assert np.array_equal(dc.layer_plain(oracle, *dc.dynamic_mesh(getattr(dc, name)), V=v), D[0])
    DA = dc.layer(oracle, *dc.dynamic_mesh(dc.A), V=v)[0]
    DB = dc.layer(oracle, *dc.dynamic_mesh(dc.B), V=v)[0]
    assert (DA != DB).any()
