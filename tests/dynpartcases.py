"""The cases of the dynamic-parts tests (include/vct.h "dynamic mesh", Parts), NumPy only: the object of tests/dyncases.py
at A split into rigid parts, three poses of one 3 x 4 matrix per part, and transform_ref, the definition's arithmetic in
float32 with one rounding per product and sum.  tests/test_dynamic_parts_cases.py holds the premises on the CPU oracle.

Meshes: dyncases.dynamic_mesh(dc.A, ntri) for ntri = 150, 300 (crosses a 256-thread block, ragged last wave) and 1.
Parts: nparts = 5 -- indices drawn from {0, 1, 2} with a seeded rng, so parts interleave inside a wave; triangle 0 alone in
part 3; part 4 owns nothing.
Poses: P0 identity; P1 per part a different rotation about the object's centre and a translation that carries the parts
at least one brick (375 model units) apart; P2 part 0 mirrored in x and scaled by 0.5, part 1 under another rotation, the
others as in P1.  Matrices are built in float64 and rounded once."""
import numpy as np

import dyncases as dc

f32 = np.float32
NPARTS = 5
SIZES = (150, 300, 1)
BRICK = 375.0                  # model units per 8^3 brick at 64^3: 8 * G / (V * model_scale)
CENTRE = np.asarray(dc.A, np.float64)
MAX_BRICKS = 64                # what the GPU tests pass to set_dynamic_mesh: every pose of every size fits (premise)
SMALL_CAPACITY = 16            # ... and what the over-capacity test passes: P0 fits, P1 needs 18 more (premise)
# the view of the draw conditions: camera position, yaw, pitch (scene.default_camera) and the light direction, world units
VIEW = dict(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
LIGHT = (0.0, 1.0, 0.25)
MIRRORED, ROTATED, LONE, EMPTY = 0, 1, 3, 4

# P1: (axis, degrees, translation) per part -- the translations differ pairwise by more than a brick in some coordinate
P1_MOVES = (((0.0, 0.0, 1.0), 35.0, (700.0, 500.0, 100.0)),
            ((1.0, 1.0, 0.0), -50.0, (-600.0, 450.0, 300.0)),
            ((0.0, 1.0, 0.5), 110.0, (100.0, -700.0, -150.0)),
            ((1.0, 0.0, 0.0), 20.0, (-500.0, -400.0, 600.0)),
            ((0.3, 0.2, 1.0), 75.0, (0.0, 0.0, 900.0)))


def mesh(ntri):
    return dc.dynamic_mesh(dc.A, ntri)


def parts(ntri, seed=19):
    """int32 [ntri]: triangle 0 -> part 3, every other triangle -> one of 0, 1, 2; part 4 stays empty."""
    p = np.random.default_rng(seed).integers(0, 3, ntri).astype(np.int32)
    p[0] = LONE
    return p


def rotation(axis, degrees):
    """Rodrigues' rotation matrix, float64 [3, 3]."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def about(L, translation=(0.0, 0.0, 0.0), centre=CENTRE):
    """The 3 x 4 matrix of x -> L (x - centre) + centre + translation, float64."""
    L = np.asarray(L, np.float64)
    return np.concatenate([L, (centre - L @ centre + np.asarray(translation, np.float64))[:, None]], 1)


def pose_f64(name):
    """float64 [NPARTS, 3, 4]"""
    if name == "P0":
        return np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), (NPARTS, 1, 1))
    m = np.stack([about(rotation(ax, deg), t) for ax, deg, t in P1_MOVES])
    if name == "P2":
        m[MIRRORED] = about(np.diag([-0.5, 0.5, 0.5]), P1_MOVES[MIRRORED][2])
        m[ROTATED] = about(rotation((0.2, -1.0, 0.4), 160.0), P1_MOVES[ROTATED][2])
    else:
        assert name == "P1", name
    return m


def pose(name):
    """float32 [NPARTS, 12]: the rows of each part's matrix, rounded once."""
    return np.ascontiguousarray(pose_f64(name).astype(f32).reshape(NPARTS, 12))


POSES = ("P0", "P1", "P2")


def parts_all(ntri, seed=23):
    """int32 [ntri] drawn from all of 0 .. NPARTS-1: the assignment of the bad-matrix test, where four parts get a matrix
    that removes them and the fifth has to leave something to compare."""
    return np.random.default_rng(seed).integers(0, NPARTS, ntri).astype(np.int32)


def transform_ref(rest, part, m):
    """The definition: for every vertex (x, y, z) of a rest triangle of part k, M = m[k], r = 0, 1, 2
    p'_r = ((M[4r] * x + M[4r+1] * y) + M[4r+2] * z) + M[4r+3], every product and sum rounded to float32."""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 3, 3)
    M = np.ascontiguousarray(m, f32).reshape(-1, 3, 4)[np.asarray(part)]          # [ntri, 3, 4]
    x, y, z = (rest[:, :, None, k] for k in range(3))                              # [ntri, 3 vertices, 1]
    a, b, c, d = (M[:, None, :, k] for k in range(4))                              # [ntri, 1, 3 rows]
    with np.errstate(invalid="ignore", over="ignore"):
        out = ((a * x + b * y).astype(f32) + (c * z).astype(f32)).astype(f32) + d
    assert out.dtype == f32
    return np.ascontiguousarray(out.reshape(-1, 9))


def transform_fused(rest, part, m):
    """What a contracting compiler would make of the same expression: fma(c, z, fma(b, y, a * x)) + d, each fma formed in
    float64 (the product of two float32 is exact there) and rounded once.  NOT the definition: the premise is that it
    differs from transform_ref, so that the tests pin the operation order."""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 3, 3)
    M = np.ascontiguousarray(m, f32).reshape(-1, 3, 4)[np.asarray(part)]
    x, y, z = (rest[:, :, None, k].astype(np.float64) for k in range(3))
    a, b, c, d = (M[:, None, :, k].astype(np.float64) for k in range(4))
    t = (a * x).astype(f32).astype(np.float64)
    t = (b * y + t).astype(f32).astype(np.float64)
    t = (c * z + t).astype(f32)
    return np.ascontiguousarray((t + d.astype(f32)).astype(f32).reshape(-1, 9))


def winding_normals(pos):
    """cross(p1 - p0, p2 - p0) per triangle, float64 [ntri, 3]."""
    p = np.asarray(pos, np.float64).reshape(-1, 3, 3)
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def bad_matrices():
    """float32 [NPARTS, 12]: P1 with a NaN element in part 0's matrix, an infinity in part 1's, a scale that leaves the
    vertex contract in part 2's, all zeros for part 3 (every vertex at the origin: no area, no fragment, not skipped);
    part 4 as it was."""
    m = pose("P1").copy()
    m[0, 5] = f32(np.nan)
    m[1, 3] = f32(np.inf)
    m[2] = about(np.eye(3) * 1.0e12).astype(f32).reshape(12)
    m[3] = 0.0
    return m
