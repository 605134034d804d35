"""CPU: the premises of the corner-normal tests (include/vct.h "dynamic mesh", Normals), held on the restatement
(tests/dynamic_normals_ref.py), the cases (tests/dynnormalcases.py) and the CPU checker, so that the GPU tests
(tests/test_gpu_dynamic_normals.py) cannot pass vacuously."""
import numpy as np
import pytest

import dynamic_normals_ref as nr
import dyndrawcases as ddc
import dynnormalcases as nc
import dynpartcases as dp
import dynskincases as ds

f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_sphere():
    pos, nrm, mat, pal = nc.sphere()
    assert pos.shape == (nc.NTRI, 9) and nrm.shape == (nc.NTRI, 3, 3) and nc.NTRI == 96
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=-1), 1.0, atol=1e-6)
    p = pos.reshape(-1, 3, 3).astype(np.float64)
    face = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.linalg.norm(face, axis=1) > 1.0).all()                                   # no degenerate triangle
    assert ((face[:, None, :] * nrm).sum(-1) > 0).all()                                 # outward winding
    assert ddc.in_contract(pos).all()
    for n in nc.SIZES:
        q = nc.padded(n)
        assert q[0].shape == (n, 9) and q[1].shape == (n, 3, 3) and np.array_equal(q[0][:min(n, 96)], pos[:min(n, 96)])


def test_every_path_is_taken_by_a_listed_corner():
    pos, nrm, _, _ = nc.adversarial()
    (un, ut, ub), own, why = nr.corner_frames(nr.draw_copy(pos), nr.moved_normals(nrm))
    uf, tf, bf = ddc.dynamic_frames(pos)
    assert np.array_equal(bits(uf[nc.FLAT[0]][:3]), bits([0, 0, 1])) and np.array_equal(tf[nc.FLAT[0]][:3], f32([1, 0, 0]))
    seen = set()
    for name, t, c, _, path in nc.CORNERS:
        assert why[t, c] == path, (name, int(why[t, c]), path)
        seen.add(path)
        got = [a.reshape(-1, 3, 3)[t, c] for a in (un, ut, ub)]
        face = [a.reshape(-1, 3, 3)[t, c] for a in (uf, tf, bf)]
        same = all(np.array_equal(bits(g), bits(f)) for g, f in zip(got, face))
        assert same == (path != 0), name                                                # a fallback IS the face frame, bit for bit
    assert seen == {0, 1, 2}
    assert own.sum() >= 3 * nc.NTRI - 8                                                 # every other corner is accepted
    assert np.isfinite(un).all() and np.isfinite(ut).all() and np.isfinite(ub).all()    # nothing unusable reaches a frame


def test_smooth_frames_differ_from_face_frames_at_every_triangle():
    pos, nrm, _, _ = nc.sphere()
    smooth = nr.frames(pos, nrm)
    for a, b in zip(smooth, ddc.dynamic_frames(pos)):
        assert (bits(a) != bits(b)).any(1).all()
    n, t, b = (a.reshape(-1, 3).astype(np.float64) for a in smooth)
    assert np.abs((n * t).sum(1)).max() < 1e-6 and np.abs(np.linalg.norm(t, axis=1) - 1).max() < 1e-6
    assert np.abs(np.cross(n, t) - b).max() < 1e-6


@pytest.mark.parametrize("w,h", ddc.FRAMES)
def test_the_checker_s_planes_change_and_det_stays_away_from_zero(oracle, w, h):
    """The 23 planes of the concatenated mesh with smooth frames against those with face frames; and det = T . (B x N) of
    the interpolated frame, the divisor of the shade kernel's shading normal, at every pixel the sphere owns.  The bound
    0.5 is a premise checked here, not assumed: each corner's (t, b, n) is orthonormal (det 1) and every t comes from ONE
    face tangent, so inside a triangle the three frames differ by the rotation between the corner normals -- at most 52
    degrees on this sphere (45 in longitude at the equator, 24 in latitude, along a quad's diagonal) -- and a convex mix of
    such frames shrinks each vector by at most cos 26 degrees and keeps them near orthogonal; found: 0.82 .. 1.00.  A fresh
    axis choice per corner reaches below 0.1 on the same sphere (test_det_over_every_triangle_of_the_sphere)."""
    static = ddc.static_mesh()
    pos, nrm, mat, pal = nc.sphere()
    faceted = ddc.reference(oracle, ddc.concatenated(static, (pos, mat, pal)), w, h)[1].reshape(23, -1)
    smooth = ddc.reference(oracle, nr.concatenated(static, (pos, mat, pal), nrm), w, h)[1].reshape(23, -1)
    own = ddc.owner_is_dynamic(smooth)
    assert np.array_equal(own, ddc.owner_is_dynamic(faceted)) and own.sum() >= (800 if w == ddc.W else 8), int(own.sum())
    diff = bits(smooth) != bits(faceted)
    assert not diff[:, ~own].any()                                                      # nothing outside the object changes
    assert diff[:, own].any(0).sum() * 2 >= own.sum()
    assert diff[3:6][:, own].any(0).sum() * 2 >= own.sum() and diff[12:15][:, own].any(0).sum() * 2 >= own.sum()
    assert not diff[0:3].any() and not diff[15:19].any()                                # position, colour, coverage: untouched
    N, T, B = (smooth[k:k + 3][:, own].astype(np.float64) for k in (3, 6, 9))
    # (the planes hold the attributes through the model matrix, model_scale * identity here: unit frames come out at 1/16)
    det = (T * np.cross(B, N, axis=0)).sum(0) / ddc.MS ** 3
    print(f"{w}x{h}: {int(own.sum())} pixels, det {det.min():.4f} .. {det.max():.4f}")
    assert det.min() > 0.5


def test_det_over_every_triangle_of_the_sphere():
    """The same bound over a dense grid of convex weights in every triangle: whatever pixel a frame size puts there."""
    pos, nrm, _, _ = nc.sphere()
    n, t, b = (a.reshape(-1, 3, 3).astype(np.float64) for a in nr.frames(pos, nrm))
    k = np.arange(21) / 20.0
    w0, w1 = np.meshgrid(k, k)
    keep = w0 + w1 <= 1.0 + 1e-12
    wts = np.stack([w0[keep], w1[keep], 1.0 - w0[keep] - w1[keep]], 1)                   # [m, 3]
    N, T, B = (np.einsum("mc,tcx->tmx", wts, a) for a in (n, t, b))
    det = (T * np.cross(B, N)).sum(-1)
    assert det.min() > 0.5, det.min()
    # ... and what the Gram-Schmidt tangent is for: a fresh frame construction per corner sends det through 0 somewhere
    import gbuffer_import_ref as gi
    _, t2, b2 = gi.frame(nrm.reshape(-1, 3))
    T2, B2 = (np.einsum("mc,tcx->tmx", wts, a.reshape(-1, 3, 3).astype(np.float64)) for a in (t2, b2))
    assert (T2 * np.cross(B2, N)).sum(-1).min() < 0.1


@pytest.mark.parametrize("name", ["mirror", "scale"])
def test_the_moved_normal_stays_on_the_face_s_side(name):
    pos, nrm, _, _ = nc.sphere()
    m = nc.matrix(name)[None]
    part = nc.one_part(nc.NTRI)
    moved_pos = dp.transform_ref(pos, part, m)
    uf = ddc.dynamic_frames(moved_pos)[0].reshape(-1, 3, 3).astype(np.float64)
    uc = nr.moved_normals(nrm, part=part, m=m).astype(np.float64)
    uc /= np.linalg.norm(uc, axis=-1, keepdims=True)
    assert ((uc * uf).sum(-1) > 0).all()
    _, own, _ = nr.corner_frames(nr.draw_copy(moved_pos), nr.moved_normals(nrm, part=part, m=m))
    assert own.all()


@pytest.mark.parametrize("name", nc.NONDEGENERATE)
def test_the_cofactor_rule_is_the_inverse_transpose_in_direction(name):
    _, nrm, _, _ = nc.sphere()
    m32 = nc.matrix(name)
    A = m32.astype(np.float64).reshape(3, 4)[:, :3]
    want = (np.linalg.inv(A).T * np.linalg.det(A)) @ nrm.reshape(-1, 3).astype(np.float64).T        # [3, n]
    got = nr.moved_normals(nrm, part=nc.one_part(nc.NTRI), m=m32[None]).reshape(-1, 3).astype(np.float64).T
    cos = (want * got).sum(0) / (np.linalg.norm(want, axis=0) * np.linalg.norm(got, axis=0))
    assert (cos > 1.0 - 1e-5).all(), cos.min()


def test_degenerate_matrices_fall_back_and_a_skin_blends_per_corner():
    pos, nrm, _, _ = nc.sphere()
    part = nc.one_part(nc.NTRI)
    for name in ("nan", "tiny"):          # NaN positions leave the contract; a cofactor of 1e-40 is subnormal, its square 0: face frames
        m = nc.matrix(name)[None]
        moved = nr.moved_normals(nrm, part=part, m=m)
        assert np.isnan(moved).any() if name == "nan" else (np.abs(moved) < 1e-37).all() and (moved != 0).any()
        _, own, why = nr.corner_frames(nr.draw_copy(dp.transform_ref(pos, part, m)), moved)
        assert not own.any() and (why == 1).all()
    bone, weight = ds.influences(nc.NTRI)
    m = nc.skin_pose("P1")
    B = nr.blend(bone, weight, m)
    assert B.shape == (nc.NTRI, 3, 12) and (bits(B[:, 0]) != bits(B[:, 1])).any()       # corners of a triangle blend differently
    a = nr.moved_normals(nrm, bone=bone, weight=weight, m=m)
    assert (bits(a) != bits(nrm)).any() and np.array_equal(bits(nr.moved_normals(nrm)), bits(nrm))
    # the drawn skin: under every pose most corners keep a frame of their own, and the sphere stays in view
    bone, weight = nc.smooth_influences()
    for pose in ds.POSES:
        p = ds.skin_ref(pos, bone, weight, nc.skin_pose(pose))
        _, own, _ = nr.corner_frames(nr.draw_copy(p), nr.moved_normals(nrm, bone=bone, weight=weight, m=nc.skin_pose(pose)))
        assert ddc.in_contract(p).all() and own.mean() > 0.8, (pose, own.mean())       # (P2 blends a mirror into rotations)
