"""The cases of the corner-normal tests (include/vct.h "dynamic mesh", Normals), NumPy only.  The restatement of the
definition is tests/dynamic_normals_ref.py; tests/test_dynamic_normals_cases.py holds the premises.

Mover: a UV sphere of 8 segments x 6 bands (96 triangles) with analytic normals, in dyndrawcases' room where its object
stands (eye space, centre CENTRE, radius RADIUS; model units are eye units / MS).  The bands run from POLE to 180 - POLE
degrees of latitude: caps cut off, so that no triangle is degenerate and every triangle has a face frame to differ from.
Winding is outward: the face normal and the analytic normals are on the same side.
padded(ntri): the sphere's triangles repeated in index order up to ntri = 1, 255, 256, 257 (the 256-thread block edge).

Adversarial corners (adversarial()): the sphere followed by two FLAT triangles in the plane z = FLAT_Z facing +z, whose face
frame is exactly u_f = (0, 0, 1), t_f = (1, 0, 0), so that exact cases can be written down.  CORNERS lists each as
(name, triangle, corner, normal, expected path): 0 the corner's own frame, 1 the accept test fails, 2 t_c is all zero.

Matrices (MATRICES): identity, a rotation, the scale (1, 3, 0.25), a mirror, a singular matrix, one with a NaN and a
scale of 1e-20 whose cofactor underflows -- all about the sphere's centre, as parts (one matrix per triangle, cycled) and
as bones (dynskincases.influences, which names bones 0 .. 4 of 6)."""
import numpy as np

import dyndrawcases as ddc
import dynpartcases as dp
import dynskincases as ds

f32 = np.float32
MS = ddc.MS
CENTRE = np.array([1.0, 0.8, -10.0])          # eye space
RADIUS = 2.4
SEGMENTS, BANDS, POLE = 8, 6, 18.0
NTRI = 2 * SEGMENTS * BANDS
SIZES = (1, 255, 256, 257)
FLAT_Z = -7.0
CENTRE_MODEL = CENTRE / MS


def sphere():
    """(pos [96, 9] f32 model space, nrm [96, 3, 3] f32 analytic, material int32, palette)"""
    th = np.radians(np.linspace(POLE, 180.0 - POLE, BANDS + 1))
    ph = np.radians(np.arange(SEGMENTS + 1) * 360.0 / SEGMENTS)
    d = lambda i, j: np.array([np.sin(th[i]) * np.cos(ph[j]), np.cos(th[i]), np.sin(th[i]) * np.sin(ph[j])])
    tris = []
    for i in range(BANDS):
        for j in range(SEGMENTS):
            a, b, c, e = d(i, j), d(i + 1, j), d(i + 1, j + 1), d(i, j + 1)
            tris += [[a, b, c], [a, c, e]]
    n = np.asarray(tris)                                        # [96, 3, 3] unit directions
    face = np.cross(n[:, 1] - n[:, 0], n[:, 2] - n[:, 0])
    flip = (face * n.mean(1)).sum(1) < 0
    n[flip] = n[flip][:, [0, 2, 1]]
    pos = ((CENTRE + RADIUS * n) / MS).astype(f32).reshape(-1, 9)
    return np.ascontiguousarray(pos), np.ascontiguousarray(n.astype(f32)), (np.arange(NTRI) % 3).astype(np.int32), ddc.PALETTE.copy()


def padded(ntri):
    pos, nrm, mat, pal = sphere()
    idx = np.arange(ntri) % NTRI
    return np.ascontiguousarray(pos[idx]), np.ascontiguousarray(nrm[idx]), np.ascontiguousarray(mat[idx]), pal


FLAT = (NTRI, NTRI + 1)
BIG, TINY = f32(3.0e38), f32(1.0e-30)
CORNERS = (
    ("nan", 3, 0, (np.nan, 0.5, 0.5), 1),
    ("+inf", 5, 1, (np.inf, 0.0, 0.0), 1),
    ("-inf", 6, 2, (0.2, -np.inf, 0.1), 1),
    ("zero", 8, 0, (0.0, 0.0, 0.0), 1),
    ("at 90 degrees", FLAT[0], 1, (1.0, 0.0, 0.0), 1),           # d_f == 0 exactly
    ("beyond 90 degrees", FLAT[0], 2, (0.3, 0.0, -1.0), 1),
    ("length overflows", FLAT[1], 0, (0.0, 0.0, BIG), 1),        # BIG * BIG is inf: unit() gives 0
    ("square underflows", FLAT[1], 1, (0.0, 0.0, TINY), 1),      # TINY * TINY is 0: unit() gives 0
    ("parallel to t_f", FLAT[0], 0, (1.0, 0.0, TINY), 2),        # u_c = (1, 0, TINY), d_f = TINY > 0, k = (0, 0, -TINY): t_c = 0
    ("good on the flat", FLAT[1], 2, (0.6, 0.3, 0.7), 0),
)


def adversarial():
    """(pos [98, 9], nrm [98, 3, 3], material, palette): the sphere, then the two FLAT triangles, with CORNERS written in."""
    pos, nrm, mat, pal = sphere()
    flat = np.array([[[3.6, 2.2, FLAT_Z], [4.6, 2.2, FLAT_Z], [4.1, 3.0, FLAT_Z]],
                     [[3.6, -1.0, FLAT_Z], [4.6, -1.0, FLAT_Z], [4.1, -0.2, FLAT_Z]]]) / MS
    pos = np.concatenate([pos, flat.astype(f32).reshape(2, 9)])
    nrm = np.concatenate([nrm, np.tile(np.array([0.0, 0.0, 1.0], f32), (2, 3, 1))])
    for _, t, c, v, _ in CORNERS:
        nrm[t, c] = np.asarray(v, f32)
    mat = np.concatenate([mat, np.array([0, 1], np.int32)])
    return np.ascontiguousarray(pos), np.ascontiguousarray(nrm), mat, pal


def _about(L, move=(0.0, 0.0, 0.0)):
    return dp.about(np.asarray(L, np.float64), np.asarray(move, np.float64), centre=CENTRE_MODEL)


def matrices_f64():
    """name -> float64 [3, 4]"""
    rot = dp.rotation((0.3, 1.0, 0.2), 35.0)
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.5, 0.0, 1.0]])
    nan = _about(rot)
    nan[1, 2] = np.nan
    return {"identity": _about(np.eye(3)), "rotation": _about(rot, (8.0, 4.0, -6.0)), "scale": _about(np.diag([1.0, 3.0, 0.25])),
            "mirror": _about(np.diag([-1.0, 1.0, 1.0])), "singular": _about(singular), "nan": nan,
            "tiny": _about(np.eye(3) * 1e-20)}


NONDEGENERATE = ("identity", "rotation", "scale", "mirror")
MATRICES = tuple(matrices_f64())


def matrix(name):
    return np.ascontiguousarray(matrices_f64()[name].astype(f32).reshape(12))


def table(shift=0):
    """float32 [7, 12]: MATRICES rotated by `shift` places, for parts(ntri) -- over 7 shifts every triangle meets every matrix."""
    names = MATRICES[shift % len(MATRICES):] + MATRICES[:shift % len(MATRICES)]
    return np.ascontiguousarray(np.stack([matrix(n) for n in names]))


def parts(ntri):
    return (np.arange(ntri) % len(MATRICES)).astype(np.int32)


def one_part(ntri):
    return np.zeros(ntri, np.int32)


def bone_table(shift=0):
    """float32 [NBONES, 12]: six of MATRICES as bones, rotated by `shift`; dynskincases.influences names bones 0 .. 4."""
    return np.ascontiguousarray(table(shift)[:ds.NBONES])


def skin_pose(name):
    """dynskincases' poses brought to the room: the same rotations (and P2's mirrored, halved bone 0) about the sphere's
    centre, the translations at a tenth -- 10 .. 20 model units, about one eye unit -- so that the skinned sphere stays in
    view.  float32 [NBONES, 12]."""
    if name == "P0":
        return ds.pose("P0")
    m = np.stack([_about(dp.rotation(ax, deg), 0.1 * np.asarray(t)) for ax, deg, t in ds.P1_MOVES])
    if name == "P2":
        m[0] = _about(np.diag([-0.5, 0.5, 0.5]), 0.1 * np.asarray(ds.P1_MOVES[0][2]))
    return np.ascontiguousarray(m.astype(f32).reshape(ds.NBONES, 12))


def smooth_influences(ntri=NTRI):
    """Influences for the DRAWN skin: per corner bones (0, 1, 2, 0) weighted by the corner's height on the sphere, so that
    corners sharing a vertex move together and the skinned surface stays closed.  (bone int32, weight f32) [ntri, 3, 4]."""
    pos = padded(ntri)[0].reshape(-1, 3, 3)
    h = np.clip((pos[..., 1].astype(np.float64) - (CENTRE_MODEL[1] - RADIUS / MS)) / (2 * RADIUS / MS), 0.0, 1.0)
    w = np.stack([np.clip(1 - 2 * h, 0, 1), 1 - np.abs(2 * h - 1), np.clip(2 * h - 1, 0, 1), np.zeros_like(h)], -1)
    bone = np.tile(np.array([0, 1, 2, 0], np.int32), (ntri, 3, 1))
    return np.ascontiguousarray(bone), np.ascontiguousarray(w.astype(f32))
