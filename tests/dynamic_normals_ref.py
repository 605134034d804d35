"""The definition of include/vct.h "dynamic mesh", Normals, in NumPy with every operation rounded to float32 (all arrays are
float32, so each product, sum and difference rounds once, in the written order): the cofactor matrix of a 3 x 4 matrix,
the moved corner normal n' = C n for no mover, parts and a skin, and the per-corner frame on the face frame of the draw
copy.  unit() and the face frame are gbuffer_import_ref's, the skin's blend is dynskincases' arithmetic."""
import numpy as np

import dyndrawcases as ddc
import dynskincases as ds
import gbuffer_import_ref as gi

f32 = np.float32
_quiet = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


def _cross(a, b):
    """a x b, each component p * q - r * s in the face normal's component order"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(f32)


def cofactor(m):
    """C [..., 3, 3] of matrices m [..., 12]: C_0 = A_1 x A_2, C_1 = A_2 x A_0, C_2 = A_0 x A_1, A_r the rows' first three."""
    A = np.ascontiguousarray(m, f32).reshape(m.shape[:-1] + (3, 4))[..., :3]
    with np.errstate(**_quiet):
        return np.stack([_cross(A[..., 1, :], A[..., 2, :]), _cross(A[..., 2, :], A[..., 0, :]), _cross(A[..., 0, :], A[..., 1, :])], -2)


def apply_cofactor(C, n):
    """n'_r = ((C_r.x * n.x + C_r.y * n.y) + C_r.z * n.z) for C [..., 3, 3] and n [..., 3]"""
    n = np.ascontiguousarray(n, f32)
    with np.errstate(**_quiet):
        out = (C[..., 0] * n[..., None, 0] + C[..., 1] * n[..., None, 1]) + C[..., 2] * n[..., None, 2]
    assert out.dtype == f32
    return out


def blend(bone, weight, m):
    """B [ntri, 3, 12] of the header's Skin: ((w0 * M0[j] + w1 * M1[j]) + w2 * M2[j]) + w3 * M3[j], all four terms always."""
    M = np.ascontiguousarray(m, f32).reshape(-1, 12)[np.asarray(bone).reshape(-1, 3, 4)]
    w = np.ascontiguousarray(weight, f32).reshape(-1, 3, 4, 1)
    with np.errstate(**_quiet):
        t = [w[:, :, k] * M[:, :, k] for k in range(4)]
        B = ((t[0] + t[1]) + t[2]) + t[3]
    ones = np.ones((B.shape[0], 3, 3), f32)          # the very blend skin_ref moves with: both move (1, 1, 1) to the same bits
    assert B.dtype == f32 and np.array_equal(ds.skin_ref(ones, bone, weight, m), _rows(B, ones).reshape(-1, 9), equal_nan=True)
    return B


def _rows(B, p):
    B = B.reshape(-1, 3, 3, 4)
    with np.errstate(**_quiet):
        return ((B[..., 0] * p[:, :, None, 0] + B[..., 1] * p[:, :, None, 1]) + B[..., 2] * p[:, :, None, 2]) + B[..., 3]


def moved_normals(nrm, part=None, bone=None, weight=None, m=None):
    """n' [ntri, 3, 3]: nrm as given with no matrices; through the part's cofactor; or through the corner's blended B's."""
    n = np.ascontiguousarray(nrm, f32).reshape(-1, 3, 3)
    if m is None:
        return n.copy()
    if part is not None:
        C = cofactor(np.ascontiguousarray(m, f32).reshape(-1, 12)[np.asarray(part)])          # [ntri, 3, 3]
        return apply_cofactor(C[:, None], n)
    return apply_cofactor(cofactor(blend(bone, weight, m)), n)


def corner_frames(draw_pos, moved):
    """((nrm, tan, bit) [ntri, 9] each, own [ntri, 3], why [ntri, 3]) of draw-copy positions and moved normals.
    why: 0 the corner took its own frame, 1 the accept test !(d_f > 0) sent it to the face frame, 2 an all-zero t_c did."""
    uf, tf, bf = (a.reshape(-1, 3, 3) for a in ddc.dynamic_frames(draw_pos))
    n = np.ascontiguousarray(moved, f32).reshape(-1, 3, 3)
    with np.errstate(**_quiet):
        uc = gi.unit(n.reshape(-1, 3)).reshape(-1, 3, 3)
        df = (uc[..., 0] * uf[..., 0] + uc[..., 1] * uf[..., 1]) + uc[..., 2] * uf[..., 2]
        accept = df > 0
        d = (uc[..., 0] * tf[..., 0] + uc[..., 1] * tf[..., 1]) + uc[..., 2] * tf[..., 2]
        k = tf - uc * d[..., None]
        tc = gi.unit(k.reshape(-1, 3)).reshape(-1, 3, 3)
        has_t = ~(tc == 0).all(-1)
        bc = _cross(uc, tc)
    assert uc.dtype == tc.dtype == bc.dtype == df.dtype == f32
    own = accept & has_t
    why = np.where(own, 0, np.where(accept, 2, 1))
    pick = lambda c, f: np.ascontiguousarray(np.where(own[..., None], c, f).reshape(-1, 9), f32)
    return (pick(uc, uf), pick(tc, tf), pick(bc, bf)), own, why


def draw_copy(pos):
    """The draw copy: a triangle outside the vertex contract as nine zeros."""
    p = np.ascontiguousarray(pos, f32).reshape(-1, 9).copy()
    p[~ddc.in_contract(p)] = 0.0
    return p


def frames(pos, nrm, part=None, bone=None, weight=None, m=None, rest=None):
    """The frames vct_download_dynamic_frames returns: pos the layer's current positions; with matrices m, nrm is in the
    space of the rest positions and pos is what they were moved to."""
    return corner_frames(draw_copy(pos), moved_normals(nrm, part, bone, weight, m))[0]


def concatenated(static, dyn, nrm, specular=ddc.SPECULAR, **mover):
    """dyndrawcases.concatenated with the appended triangles carrying the corner frames of nrm."""
    cat = ddc.concatenated(static, dyn, specular)
    ns = static[0].shape[0]
    fr = frames(dyn[0], nrm, **mover)
    new = tuple(np.concatenate([a[:ns], b]) for a, b in zip(cat[4], fr))
    return cat[:4] + (new,)
