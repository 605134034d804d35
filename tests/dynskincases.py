"""The cases of the dynamic-skin tests (include/vct.h "dynamic mesh", Skin), NumPy only: the object of tests/dyncases.py at
A with four bone influences per triangle corner, three poses of one 3 x 4 matrix per bone, and skin_ref, the definition's
arithmetic in float32 with one rounding per product and sum.  tests/test_dynamic_skin_cases.py holds the premises on the
CPU oracle.

Meshes: dyncases.dynamic_mesh(dc.A, ntri) for ntri = 150, 300 (crosses a 256-thread block, ragged last wave) and 1.
Bones: nbones = 6; corners name bones 0 .. 4 (0 .. 2 often, 3 and 4 seldom, so that the bad-matrix case leaves triangles
to compare); no corner names bone 5.
Influences (seeded): per corner 1, 2 or 4 non-zero weights on distinct bones, normalised to 1 in float64 and rounded once;
a slot that is not used has weight 0 and points at the corner's first bone -- one that is in use, as the header advises.
Three corners are then rewritten where the mesh has them: triangle 1 corner 2 sums to 0.9, triangle 2 corner 0 to 1.1, and
triangle 3 corner 1 is (1.25, -0.25, 0, 0) on bones 0 and 1.
Poses: P0 identity; P1 per bone a different rotation about the object's centre and a translation of 100 .. 200 model units
(the object stretches where corners follow different bones); P2 bone 0 mirrored in x and scaled by 0.5, the others as in P1.
PX is P1 with five times the translations: the over-capacity pose.  Matrices are built in float64 and rounded once."""
import numpy as np

import dyncases as dc
import dynpartcases as dp

f32 = np.float32
NBONES = 6
UNNAMED = 5
SIZES = (150, 300, 1)
MAX_BRICKS = 64                # what the GPU tests pass to set_dynamic_mesh: every pose of every size fits (premise)
SMALL_CAPACITY = 16            # ... and what the over-capacity test passes: P0 fits, PX needs OVER more (premise)
OVER = 50
VIEW, LIGHT = dp.VIEW, dp.LIGHT
BONE_P = (0.3, 0.3, 0.25, 0.1, 0.05)      # how often a corner's influence names bone 0 .. 4
NAN_BONE, INF_BONE = 3, 4                  # the bones that get a bad matrix in bad_matrices()
SUM_09, SUM_11, NEGATIVE = (1, 2), (2, 0), (3, 1)      # (triangle, corner) of the rewritten corners

P1_MOVES = (((0.0, 0.0, 1.0), 25.0, (150.0, 100.0, 0.0)),
            ((1.0, 1.0, 0.0), -30.0, (-120.0, 90.0, 60.0)),
            ((0.0, 1.0, 0.5), 40.0, (20.0, -140.0, -30.0)),
            ((1.0, 0.0, 0.0), 15.0, (-100.0, -80.0, 120.0)),
            ((0.3, 0.2, 1.0), 35.0, (0.0, 0.0, 180.0)),
            ((0.0, 1.0, 0.0), 90.0, (300.0, 300.0, 300.0)))


def mesh(ntri):
    return dc.dynamic_mesh(dc.A, ntri)


def influences(ntri, seed=29):
    """(bone int32 [ntri, 3, 4], weight float32 [ntri, 3, 4]) as described above."""
    r = np.random.default_rng(seed)
    bone = np.zeros((ntri, 3, 4), np.int32)
    weight = np.zeros((ntri, 3, 4), np.float64)
    for t in range(ntri):
        for v in range(3):
            n = int(r.choice((1, 2, 4), p=(0.3, 0.4, 0.3)))
            b = r.choice(5, size=n, replace=False, p=BONE_P)
            w = r.uniform(0.1, 1.0, n)
            bone[t, v, :] = b[0]
            bone[t, v, :n] = b
            weight[t, v, :n] = w / w.sum()
    if ntri > SUM_09[0]:
        weight[SUM_09] *= 0.9
    if ntri > SUM_11[0]:
        weight[SUM_11] *= 1.1
    if ntri > NEGATIVE[0]:
        bone[NEGATIVE] = (0, 1, 0, 0)
        weight[NEGATIVE] = (1.25, -0.25, 0.0, 0.0)
    return bone, np.ascontiguousarray(weight.astype(f32))


def pose_f64(name):
    """float64 [NBONES, 3, 4]"""
    if name == "P0":
        return np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), (NBONES, 1, 1))
    scale = 5.0 if name == "PX" else 1.0
    m = np.stack([dp.about(dp.rotation(ax, deg), scale * np.asarray(t)) for ax, deg, t in P1_MOVES])
    if name == "P2":
        m[0] = dp.about(np.diag([-0.5, 0.5, 0.5]), P1_MOVES[0][2])
    else:
        assert name in ("P1", "PX"), name
    return m


def pose(name):
    """float32 [NBONES, 12]: the rows of each bone's matrix, rounded once."""
    return np.ascontiguousarray(pose_f64(name).astype(f32).reshape(NBONES, 12))


POSES = ("P0", "P1", "P2")


def _gather(rest, bone, weight, m, dtype):
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 3, 3).astype(dtype)
    M = np.ascontiguousarray(m, f32).reshape(-1, 12)[np.asarray(bone).reshape(-1, 3, 4)].astype(dtype)      # [ntri, 3, 4 slots, 12]
    w = np.ascontiguousarray(weight, f32).reshape(-1, 3, 4, 1).astype(dtype)
    return rest, M, w


def skin_ref(rest, bone, weight, m):
    """The definition: per corner B[j] = ((w0 * M0[j] + w1 * M1[j]) + w2 * M2[j]) + w3 * M3[j], then
    p'_r = ((B[4r] * x + B[4r+1] * y) + B[4r+2] * z) + B[4r+3], every product and sum rounded to float32; all four terms
    always, so 0 * inf and 0 * NaN give NaN."""
    rest, M, w = _gather(rest, bone, weight, m, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = [(w[:, :, k] * M[:, :, k]).astype(f32) for k in range(4)]
        B = (((t[0] + t[1]).astype(f32) + t[2]).astype(f32) + t[3]).astype(f32).reshape(-1, 3, 3, 4)          # [ntri, corner, row, 4]
        x, y, z = (rest[:, :, None, k] for k in range(3))
        a, b, c, d = (B[..., k] for k in range(4))
        out = (((a * x).astype(f32) + (b * y).astype(f32)).astype(f32) + (c * z).astype(f32)).astype(f32) + d
    assert out.dtype == f32
    return np.ascontiguousarray(out.reshape(-1, 9))


def skin_fused(rest, bone, weight, m):
    """What a contracting compiler would make of the same expressions: every `+ p * q` a fused multiply-add, formed in
    float64 (the product of two float32 is exact there) and rounded once.  NOT the definition: the premise is that it
    differs from skin_ref, so that the tests pin the operation order."""
    rest, M, w = _gather(rest, bone, weight, m, np.float64)
    r = lambda v: v.astype(f32).astype(np.float64)
    B = r(w[:, :, 0] * M[:, :, 0])
    for k in (1, 2, 3):
        B = r(w[:, :, k] * M[:, :, k] + B)
    B = B.reshape(-1, 3, 3, 4)
    x, y, z = (rest[:, :, None, k] for k in range(3))
    t = r(B[..., 0] * x)
    t = r(B[..., 1] * y + t)
    t = r(B[..., 2] * z + t)
    return np.ascontiguousarray((t + B[..., 3]).astype(f32).reshape(-1, 9))


def names(bone, k):
    """bool [ntri]: the triangles with a corner that names bone k in any slot."""
    return (np.asarray(bone).reshape(-1, 12) == k).any(1)


def bad_matrices():
    """float32 [NBONES, 12]: P1 with a NaN element in NAN_BONE's matrix and an infinity in INF_BONE's."""
    m = pose("P1").copy()
    m[NAN_BONE, 5] = f32(np.nan)
    m[INF_BONE, 3] = f32(np.inf)
    return m


def zero_weight_case(ntri=150):
    """(bone, weight, t, matrices): the influences with the UNNAMED bone in the last slot of the last corner of triangle t
    -- the first triangle behind the rewritten corners whose slot has weight 0 anyway -- and P1 with a NaN in that bone's
    matrix.  The definition evaluates all four terms, 0 * NaN is NaN: exactly triangle t leaves the vertex contract."""
    bone, weight = influences(ntri)
    t = next(t for t in range(4, ntri) if weight[t, 2, 3] == 0)
    bone[t, 2, 3] = UNNAMED
    m = pose("P1").copy()
    m[UNNAMED, 0] = f32(np.nan)
    return bone, weight, t, m


def in_contract(pos):
    """bool [ntri]: the device-side vertex contract, !(|v * model_scale| <= 2^20 * G) for no coordinate."""
    lim = f32(1048576.0) * f32(dc.G)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.abs(np.asarray(pos, f32).reshape(-1, 9) * f32(dc.MS)) <= lim).all(1)
