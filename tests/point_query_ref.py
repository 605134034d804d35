"""Reference of the point queries (include/vct.h "point queries"), built from the existing oracle only.

Gather: the points become pixels of a 23-plane G-buffer -- planes 0-11 the point's position, normal, tangent, bitangent,
plane 18 (albedo.a) = 1, every other plane as synth.random_gbuffer fills it -- and oracle.trace(..., want_cones=True)
marches them: cones and steps are its columns 0-5, the gather is components_ref.gather of those cones.
Cone: oracle.cone(p, chain, position, normal, direction, tan) per point.

cone_dirs restates csrc/vct_trace.hip cone_frame + cone_dir in fp32 NumPy (every operation rounded on its own, in the
kernel's order); tests/test_point_query_cases.py pins it by holding oracle.cone along those directions to oracle.trace."""
import numpy as np

import components_ref as cr
import synth

f32 = np.float32


def planes_of(points, seed=11):
    """[23, n] G-buffer whose pixel i is gather point i."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 12)
    g = synth.random_gbuffer(pts.shape[0], seed=seed)
    g[0:12] = pts.T
    g[18] = 1.0
    return np.ascontiguousarray(g, f32)


def gather(oracle, p, chain, points, nthreads=8):
    """dict(gather [n, 4], cones [n, 6, 4], steps uint8 [n, 6], total_steps) of the gather points [n, 12]."""
    ref = oracle.trace(p, chain, planes_of(points), nthreads=nthreads, want_cones=True)
    cones = np.ascontiguousarray(ref["cones"][:, :6])
    steps = np.ascontiguousarray(ref["steps"][:, :6])
    with np.errstate(all="ignore"):
        ind = cr.gather(cones)
    return dict(gather=ind, cones=cones, steps=steps, total_steps=int(steps.astype(np.int64).sum()))


def cones(oracle, p, chain, points, tan_half):
    """dict(cone [n, 4], steps [n], total_steps) of the cone points [n, 9]."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 9)
    out = np.zeros((pts.shape[0], 4), f32)
    steps = np.zeros(pts.shape[0], np.int64)
    for i, r in enumerate(pts):
        out[i], steps[i] = oracle.cone(p, chain, r[0:3], r[3:6], r[6:9], tan_half)
    return dict(cone=out, steps=steps, total_steps=int(steps.sum()))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cone_dirs(oracle, points):
    """[n, 6, 3] fp32: the six diffuse cone directions of gather points [n, 12], as cone_frame + cone_dir form them."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 12)
    N, T, B = ([pts[:, k + c] for c in range(3)] for k in (3, 6, 9))
    dirs, _ = oracle.cone_constants()
    out = np.zeros((pts.shape[0], 6, 3), f32)
    with np.errstate(all="ignore"):
        c0, c1, c2 = _cross(B, N), _cross(N, T), _cross(T, B)
        inv_det = f32(1.0) / _dot(T, c0)
        k0, k1, k2 = ([c[a] * inv_det for a in range(3)] for c in (c0, c1, c2))
        for i in range(6):
            dx, dy, dz = (f32(v) for v in dirs[i])
            d = [(k0[a] * dx + k1[a] * dy) + k2[a] * dz for a in range(3)]
            ln = np.sqrt(_dot(d, d))
            for a in range(3):
                out[:, i, a] = d[a] / ln
    return out


def cone_points_of(points, dirs):
    """[n, 9] cone points: position and normal of gather points [n, 12] with directions [n, 3]."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 12)
    return np.ascontiguousarray(np.concatenate([pts[:, 0:6], np.asarray(dirs, f32).reshape(-1, 3)], axis=1), f32)


def u32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_floats_match(got, want, what):
    """Bit patterns equal, except that NaN equals NaN (sign and payload of a NaN differ between x86 and gfx950)."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in different places"
    bad = u32(got)[~nan] != u32(want)[~nan]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} floats are not bit-identical"
