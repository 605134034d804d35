"""The reference of sky light (include/vct.h "sky light"), formed from the CPU oracle as it is.

The oracle returns a cone's colour and occlusion but not the alpha its march ended with.  It does not need to: tri_sample,
texture_lod and the march treat the four channels with identical operations (cr = fmaf(oma, vc[0], cr) and
alpha = fmaf(oma, vc[3], alpha)), so a second oracle run on a copy of the chain whose red byte is replaced by its alpha
byte at every texel of every level has, as its red cone component, the first run's final alpha -- bit for bit
(tests/test_sky_restatement.py holds the two runs to each other).  trace() runs the oracle twice, forms
T = fmaxf(1 - alpha, 0) per cone, restates the cone directions (point_query_ref.cone_dirs for the six diffuse cones, the
helpers of components_ref for the specular one), evaluates the sky with the chain of the header -- fma emulated in fp64 as
components_ref._fma does -- adds it to the first run's cones and composites with components_ref.composite.
Test infrastructure: NumPy + the oracle, no GPU."""
import numpy as np

import components_ref as cr
import point_query_ref as pq

f32 = np.float32
# K_i of the orthonormal real basis over 1, y, z, x, xy, yz, 3z^2-1, xz, x^2-y^2
K = np.array([0.28209479177387814, 0.4886025119029199, 0.4886025119029199, 0.4886025119029199, 1.0925484305920792,
              1.0925484305920792, 0.31539156525252005, 1.0925484305920792, 0.5462742152960396], np.float64)
# the sky the tests light with: all nine coefficients non-zero, and the blue channel negative around -y (the clamp)
SH = np.array([[1.2, 1.0, 0.7], [0.5, 0.45, 1.3], [-0.2, 0.15, 0.1], [0.3, -0.25, 0.2], [0.1, 0.2, -0.15],
               [-0.12, 0.1, 0.22], [0.25, -0.2, 0.18], [0.14, 0.16, -0.1], [-0.3, 0.28, 0.12]], f32)


def fold(sh):
    """poly[i][c] = (float)(K_i * (double)sh[i][c])."""
    return (K[:, None] * np.asarray(sh, f32).reshape(9, 3).astype(np.float64)).astype(f32)


def eval_dirs(poly, d):
    """Sky radiance [n, 3] of directions d [n, 3]: the chain of include/vct.h "sky light" in fp32, fmaxf as np.fmax."""
    poly = np.asarray(poly, f32).reshape(9, 3)
    d = np.asarray(d, f32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    one = np.ones_like(x)
    with np.errstate(all="ignore"):
        terms = [None, y, z, x, x * y, y * z, cr._fma(f32(3.0) * z, z, -one), x * z, cr._fma(x, x, -(y * y))]
        out = np.zeros((d.shape[0], 3), f32)
        for c in range(3):
            s = np.full_like(x, poly[0, c])
            for i in range(1, 9):
                s = cr._fma(np.full_like(x, poly[i, c]), terms[i], s)
            out[:, c] = np.fmax(s, f32(0.0))
    return out


def eval_textbook(sh, d):
    """The real spherical-harmonic series of `sh` at unit directions d, in float64, unclamped: [n, 3] and the largest
    absolute term per direction and channel [n, 3]."""
    sh = np.asarray(sh, f32).reshape(9, 3).astype(np.float64)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    basis = np.stack([np.ones_like(x), y, z, x, x * y, y * z, 3.0 * z * z - 1.0, x * z, x * x - y * y], axis=1) * K[None, :]
    terms = basis[:, :, None] * sh[None, :, :]
    return terms.sum(1), np.abs(terms).max(1)


def alpha_chain(chain):
    """The chain with the red byte of every texel of every level replaced by its alpha byte."""
    c = np.array(chain, np.uint8, copy=True).reshape(-1, 4)
    c[:, 0] = c[:, 3]
    return c.reshape(np.asarray(chain).shape)


def directions(oracle, planes, cam):
    """[npix, 7, 3] fp32: the normalised directions the march of a pixel's seven cones uses."""
    g = np.asarray(planes, f32)
    out = np.zeros((g.shape[1], 7, 3), f32)
    out[:, :6] = pq.cone_dirs(oracle, g[0:12].T)
    with np.errstate(all="ignore"):
        P, N = [g[0], g[1], g[2]], [g[12], g[13], g[14]]
        E = cr._normalize([f32(cam[0]) - P[0], f32(cam[1]) - P[1], f32(cam[2]) - P[2]])       # trace.fs:181
        R = cr._normalize(cr._reflect([E[0] * f32(-1.0), E[1] * f32(-1.0), E[2] * f32(-1.0)], N))   # :217
    for a in range(3):
        out[:, 6, a] = R[a]
    return out


def add_sky(cones, alpha, dirs, poly, on):
    """cones [..., 4] with rgb_c = fmaf(T, sky_c(d), rgb_c), T = fmaxf(1 - alpha, 0), where `on`; the rest as given."""
    cones = np.array(cones, f32, copy=True)
    shape = cones.shape
    c = cones.reshape(-1, 4)
    a = np.asarray(alpha, f32).reshape(-1)
    sky = eval_dirs(poly, np.asarray(dirs, f32).reshape(-1, 3))
    on = np.asarray(on, bool).reshape(-1)
    with np.errstate(all="ignore"):
        T = np.fmax(f32(1.0) - a, f32(0.0)).astype(f32)
        for k in range(3):
            c[on, k] = cr._fma(T, sky[:, k], c[:, k])[on]
    return c.reshape(shape)


def oracle_runs(oracle, p, chain, planes, nthreads=4):
    """(the oracle's trace with cones, the same on alpha_chain(chain)): the second run's red is the first one's alpha."""
    return (oracle.trace(p, chain, planes, nthreads=nthreads, want_cones=True),
            oracle.trace(p, alpha_chain(chain), planes, nthreads=nthreads, want_cones=True))


def from_runs(oracle, p, planes, runs, sh, mask=cr.SHOW_ALL, aov=0):
    """The sky frame from oracle_runs' pair: dict(rgba32f, rgba16f, steps, cones, total_steps, alpha [npix, 7])."""
    ref, ref_a = runs
    g = np.asarray(planes, f32)
    cam = [float(v) for v in p.camera_pos]
    light = [float(v) for v in p.light_dir]
    alive = ~(g[18] < f32(0.5))
    alpha = np.ascontiguousarray(ref_a["cones"][:, :, 0])
    dif, spc = cr.marched_groups(mask, aov)
    cones = cr.masked_cones(ref["cones"], mask, aov)
    steps = np.array(ref["steps"], np.uint8, copy=True)
    on = np.repeat(alive[:, None], 7, axis=1)            # a discarded pixel keeps the zero cone,
    on[:, :6] &= dif                                      # a group the mask skips is not marched and gets no sky
    on[:, 6] &= spc
    if not dif:
        steps[:, :6] = 0
    if not spc:
        steps[:, 6] = 0
    poly = fold(sh)
    cones = add_sky(cones, alpha, directions(oracle, g, cam), poly, on)
    comp = cr.composite(g, cones, cam, light, p.ambient_factor, p.shininess, mask)
    rgba32f, rgba16f = comp["rgba32f"], cr.to_f16_bits(comp["rgba32f"])
    if mask == cr.SHOW_ALL:
        # the frame is a function of the planes and the cones: a pixel none of whose cones the sky changed is the oracle's
        # own pixel (components_ref.composite restates the oracle's composite to 1e-6, not bit for bit: powf)
        same = (cones.view(np.uint32) == np.asarray(ref["cones"], f32).view(np.uint32)).all((1, 2))
        rgba32f[same] = ref["rgba32f"][same]
        rgba16f[same] = ref["rgba16f"][same]
    return dict(rgba32f=rgba32f, rgba16f=rgba16f, steps=steps, cones=cones,
                total_steps=int(steps.astype(np.int64).sum()), alpha=alpha, comp=comp)


def trace(oracle, p, chain, planes, sh, nthreads=4, mask=cr.SHOW_ALL, aov=0):
    """pyoracle.trace(..., want_cones=True) twice, then the sky: the dict shape of gloss_ref.select."""
    return from_runs(oracle, p, planes, oracle_runs(oracle, p, chain, planes, nthreads), sh, mask, aov)


def gather(oracle, p, chain, points, sh, nthreads=4):
    """vct_gather_points with a sky: dict(gather, cones [n, 6, 4], steps [n, 6], total_steps) of gather points [n, 12]."""
    planes = pq.planes_of(points)
    ref, ref_a = oracle_runs(oracle, p, chain, planes, nthreads)
    dirs = pq.cone_dirs(oracle, points)
    cones = add_sky(ref["cones"][:, :6], ref_a["cones"][:, :6, 0], dirs, fold(sh), np.ones(dirs.shape[:2], bool))
    steps = np.ascontiguousarray(ref["steps"][:, :6])
    with np.errstate(all="ignore"):
        ind = cr.gather(cones)
    return dict(gather=ind, cones=cones, steps=steps, total_steps=int(steps.astype(np.int64).sum()))


def cones(oracle, p, chain, points, tan_half, sh):
    """vct_cone_points with a sky: dict(cone [n, 4], steps [n], total_steps, alpha [n]) of cone points [n, 9]."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 9)
    ref = pq.cones(oracle, p, chain, pts, tan_half)
    ref_a = pq.cones(oracle, p, alpha_chain(chain), pts, tan_half)
    alpha = np.ascontiguousarray(ref_a["cone"][:, 0])
    cone = add_sky(ref["cone"], alpha, pts[:, 6:9], fold(sh), np.ones(pts.shape[0], bool))
    return dict(cone=cone, steps=ref["steps"], total_steps=ref["total_steps"], alpha=alpha)
