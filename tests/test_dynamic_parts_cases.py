"""CPU: the premises of tests/test_gpu_dynamic_parts.py, checked on the CPU oracle where there is no GPU -- the poses of
tests/dynpartcases.py give layers that are not degenerate for the merge rule, differ from one another, move every part,
pin the operation order of the transform, flip the winding of the mirrored part, and fit (or, where meant, exceed) the
capacities the GPU tests pass.  The one-triangle mesh is too small for the merge conditions: it serves the kernel test
alone, and is only required to occupy something."""
import itertools

import numpy as np
import pytest

import dyncases as dc
import dynpartcases as dp
from test_gpu_dynamic import NONE, RAISED, shadow_maps


@pytest.fixture(scope="module")
def maps():
    return shadow_maps()


def posed(ntri, name):
    pos, mat, alb = dp.mesh(ntri)
    return dp.transform_ref(pos, dp.parts(ntri), dp.pose(name)), mat, alb


def test_the_parts_are_as_described():
    for ntri in dp.SIZES:
        part = dp.parts(ntri)
        assert part.dtype == np.int32 and part.shape == (ntri,) and part[0] == dp.LONE
        assert (part == dp.LONE).sum() == 1 and (part == dp.EMPTY).sum() == 0 and part.max() < dp.NPARTS
    part = dp.parts(150)
    assert all((part == k).sum() >= 30 for k in range(3))
    # the parts interleave inside a wave: each of the first 64 triangles' parts 0 .. 2 occurs, and neighbours differ often
    assert set(part[1:64].tolist()) == {0, 1, 2} and (part[1:64] != part[:63]).sum() >= 30
    assert all((dp.parts_all(150) == k).sum() >= 15 for k in range(dp.NPARTS))
    assert abs(dp.BRICK - 8.0 * dc.G / (dc.V * dc.MS)) < 1e-9


def test_the_identity_reproduces_the_rest_bits_and_loses_the_sign_of_zero():
    pos = dp.mesh(150)[0]
    assert np.array_equal(dp.transform_ref(pos, dp.parts(150), dp.pose("P0")).view(np.uint32), pos.view(np.uint32))
    z = np.zeros((1, 9), np.float32)
    z[0, 0] = -0.0
    out = dp.transform_ref(z, np.zeros(1, np.int32), dp.pose("P0"))
    assert np.signbit(z[0, 0]) and not np.signbit(out[0, 0])


@pytest.mark.parametrize("ntri", [150, 300])
@pytest.mark.parametrize("shadow", [NONE, RAISED])
def test_every_pose_is_not_degenerate_and_the_poses_differ(oracle, maps, ntri, shadow):
    depth, vp = maps[shadow]
    S = dc.layer(oracle, *dc.static_scene(), depth=depth, vp=vp)[0]
    L = {}
    for name in dp.POSES:
        L[name] = dc.layer(oracle, *posed(ntri, name), depth=depth, vp=vp)[0]
        n = dc.assert_non_degenerate(L[name], S)
        assert n["dynamic_bricks"] <= dp.MAX_BRICKS, (name, n)
    for a, b in itertools.combinations(dp.POSES, 2):
        assert (L[a] != L[b]).any(-1).sum() >= 100, (a, b)


def test_the_single_triangle_occupies_something_in_every_pose(oracle):
    for name in dp.POSES:
        D = dc.layer(oracle, *posed(1, name))[0]
        assert (D[..., 3] > 0).any(), name


def test_p1_moves_every_part_that_owns_triangles_and_carries_them_a_brick_apart(oracle):
    pos, mat, alb = dp.mesh(150)
    part = dp.parts(150)
    p1 = dp.transform_ref(pos, part, dp.pose("P1"))
    for k in range(dp.NPARTS):
        sel = part == k
        if not sel.any():
            assert k == dp.EMPTY
            continue
        D0 = dc.layer(oracle, pos[sel], mat[sel], alb)[0][..., 3] > 0
        D1 = dc.layer(oracle, p1[sel], mat[sel], alb)[0][..., 3] > 0
        assert D0.any() and D1.any() and not (D0 & D1).any(), k
    t = np.array([mv[2] for mv in dp.P1_MOVES])
    for a, b in itertools.combinations(range(dp.NPARTS), 2):
        assert np.abs(t[a] - t[b]).max() >= dp.BRICK, (a, b)
    R = dp.pose_f64("P1")[:, :, :3]
    for a, b in itertools.combinations(range(dp.NPARTS), 2):
        assert np.abs(R[a] - R[b]).max() > 0.1, (a, b)
    for k in range(dp.NPARTS):
        assert np.allclose(R[k] @ R[k].T, np.eye(3), atol=1e-12) and np.linalg.det(R[k]) > 0.99


def test_a_fused_transform_would_differ():
    """Without this the operation order would not be pinned: at least 10 coordinates of P1 differ between the definition
    and the contracted form (here 127 of 1350 at 150 triangles)."""
    for ntri in (150, 300):
        pos, part = dp.mesh(ntri)[0], dp.parts(ntri)
        a, b = dp.transform_ref(pos, part, dp.pose("P1")), dp.transform_fused(pos, part, dp.pose("P1"))
        assert (a != b).sum() >= 10 and np.allclose(a, b, rtol=1e-4, atol=1e-2), ntri


def test_the_mirrored_part_has_flipped_winding_in_the_view():
    """det < 0 for the mirrored part's matrix in P2, > 0 for every other; and in the view of the draw conditions every
    triangle of the mirrored part in front of the camera is wound the other way round than its surface faces: the
    screen-space signed area has the sign opposite to (L^-T n) . (eye - centroid), n the rest triangle's winding normal --
    while for the rotated part the two signs agree."""
    import vctpkg
    vctpkg.load()
    from voxel_cone_tracing_amd import scene as sc
    w, h = 203, 117
    cam = sc.default_camera(**dp.VIEW)
    vp = np.asarray(sc.camera_view_proj(cam, w, h), np.float64).reshape(4, 4).T          # row-major: clip = vp @ (x, y, z, 1)
    eye = np.asarray(dp.VIEW["position"], np.float64)
    pos, part = dp.mesh(150)[0], dp.parts(150)
    M = dp.pose_f64("P2")
    dets = [np.linalg.det(M[k, :, :3]) for k in range(dp.NPARTS)]
    assert dets[dp.MIRRORED] < 0 and all(d > 0 for k, d in enumerate(dets) if k != dp.MIRRORED)
    p2 = dp.transform_ref(pos, part, dp.pose("P2")).astype(np.float64).reshape(-1, 3, 3) * dc.MS      # world units
    n_rest = dp.winding_normals(pos)
    checked = {}
    for k, agree in ((dp.MIRRORED, -1.0), (dp.ROTATED, 1.0)):
        surf = n_rest[part == k] @ np.linalg.inv(M[k, :, :3])          # rows: (L^-T n)^T
        tri = p2[part == k]
        clip = np.concatenate([tri, np.ones(tri.shape[:2] + (1,))], -1) @ vp.T
        front = (clip[..., 3] > 0.05).all(1)
        ndc = clip[..., :2] / clip[..., 3:4]
        e1, e2 = ndc[:, 1] - ndc[:, 0], ndc[:, 2] - ndc[:, 0]
        area = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        facing = np.einsum("ij,ij->i", surf, eye[None, :] - tri.mean(1))
        ok = front & (np.abs(area) > 1e-9)
        assert ok.sum() >= 10, (k, int(ok.sum()))
        assert (np.sign(area[ok]) == agree * np.sign(facing[ok])).all(), k
        checked[k] = (int(ok.sum()), int((area[ok] > 0).sum()))
    # both windings occur among the mirrored triangles in view: culling decides something
    assert 0 < checked[dp.MIRRORED][1] < checked[dp.MIRRORED][0], checked


def test_the_capacities(oracle):
    """Every pose fits MAX_BRICKS (above); P0 fits SMALL_CAPACITY and P1 exceeds it by 18 bricks."""
    need = {name: int(dc.bricks(dc.layer(oracle, *posed(150, name))[0][..., 3] > 0).sum()) for name in dp.POSES}
    assert need["P0"] <= dp.SMALL_CAPACITY and need["P1"] == dp.SMALL_CAPACITY + 18, need


def test_the_bad_matrices_remove_four_parts_and_leave_the_fifth(oracle):
    pos, mat, alb = dp.mesh(150)
    part = dp.parts_all(150)
    out = dp.transform_ref(pos, part, dp.bad_matrices())
    lim = np.float32(1048576.0) * np.float32(dc.G)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (np.abs(out * np.float32(dc.MS)) <= lim).all(1)
    assert np.array_equal(~inside, part <= 2) and (out[part == 3] == 0).all()
    keep = part == 4
    assert np.array_equal(out[keep], dp.transform_ref(pos, part, dp.pose("P1"))[keep])
    D = dc.layer(oracle, out[keep], mat[keep], alb)[0]
    assert (D[..., 3] > 0).sum() >= 50
    # the oracle itself gives the degenerate triangles of part 3 nothing
    both = keep | (part == 3)
    assert np.array_equal(dc.layer(oracle, out[both], mat[both], alb)[0], D)
