"""The scenes of the dynamic-mesh tests (include/vct.h "dynamic mesh"), NumPy only, and the expected chain built from the
CPU oracle: the dynamic mesh voxelized alone (D) wins per voxel over the static one (S), level0 = where(D.a > 0, D, S).

Static: voxcases.random_scene(300, seed=33) at 64^3 (at 32^3 its wall touches all 64 bricks, so no brick would be
dynamic-only).  Dynamic: 150 small triangles, centres uniform within +-250 model units of a point C, vertices normal with
sigma 25 around the centre, 3 materials; C = A and C = B are the two positions of the moving object."""
import numpy as np

import voxcases

V, G, MS = 64, 150.0, 0.05
A = (0.0, 0.0, 200.0)
B = (900.0, -700.0, 400.0)
NTRI, NMAT = 150, 3


def config(vct, V=V, G=G, ms=MS, **kw):
    kw = dict(dict(voxel_dim=V, width=8, height=8, debug_outputs=1, voxel_attributes=1, model_scale=ms, grid_world_size=G), **kw)
    return vct.default_config(**kw)


def static_scene():
    return voxcases.random_scene(300, seed=33)


def offsets(ntri=NTRI, seed=71):
    """Triangles around the origin, [ntri, 3, 3] float64: the object; dynamic_mesh moves it."""
    r = np.random.default_rng(seed)
    c = r.uniform(-250.0, 250.0, (ntri, 1, 3))
    return c + r.normal(scale=25.0, size=(ntri, 3, 3))


def materials(ntri=NTRI, seed=72):
    r = np.random.default_rng(seed)
    return r.integers(0, NMAT, ntri).astype(np.int32), r.uniform(0.1, 1.0, (NMAT, 4)).astype(np.float32)


def dynamic_mesh(C, ntri=NTRI):
    """(pos [ntri, 9] f32, material, albedo) of the object at C."""
    mat, alb = materials(ntri)
    pos = (offsets(ntri) + np.asarray(C, np.float64)[None, None, :]).astype(np.float32).reshape(-1, 9)
    return pos, mat, alb


def big_triangles(ntri=600, seed=5):
    """(pos, material, albedo) of an object of large triangles: centres uniform within +-400 model units, vertices normal
    with sigma 900 around them (the grid spans +-1500).  Nearly every box exceeds VCT_VOX_BIG voxels at 64^3, more of them
    than k_dyn_big's grid has workgroups; the layer occupies every brick of the grid."""
    r = np.random.default_rng(seed)
    c = r.uniform(-400.0, 400.0, (ntri, 1, 3))
    pos = (c + r.normal(scale=900.0, size=(ntri, 3, 3))).astype(np.float32).reshape(-1, 9)
    mat, alb = materials(ntri)
    return pos, mat, alb


def crowd(ntri=200_000, seed=91):
    """(offsets [ntri, 3, 3] float64, material, albedo) of an object of very many small triangles: centres uniform within
    +-600 model units, vertices normal with sigma 8.  At 128^3 none is big and the object touches a few hundred bricks:
    long enough on the GPU that the host's next call arrives while k_dyn_tris runs (tests/test_gpu_pipeline_features.py)."""
    r = np.random.default_rng(seed)
    off = r.uniform(-600.0, 600.0, (ntri, 1, 3)) + r.normal(scale=8.0, size=(ntri, 3, 3))
    return (off,) + materials(ntri)


def placed(off, C):
    """Positions [ntri, 9] float32 of the object `off` moved to C."""
    return (off + np.asarray(C, np.float64)[None, None, :]).astype(np.float32).reshape(-1, 9)


VOX_BIG = 4096         # VCT_VOX_BIG (csrc/vct_voxelize.hip)


def box_candidates(pos, ms=MS, G=G, V=V):
    """tri_candidates of csrc/vct_voxelize.hip per triangle, int64 [ntri]: setup_tri's clipped bounding box, operation for
    operation in fp32 (one rounding per product, quotient and sum: the library is built without contraction) -- 0 for a
    triangle whose voxel-space normal is zero or NaN or whose box misses the grid, else the voxels of the box.  A triangle
    goes to k_dyn_big when this exceeds VOX_BIG."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.asarray(pos, f).reshape(-1, 3, 3) * f(ms)
        g = (w / f(G) + f(0.5)) * f(V)
        e0, e1 = g[:, 1] - g[:, 0], g[:, 2] - g[:, 1]
        n = np.stack([e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1], e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2],
                      e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]], 1)
        valid = ~((n == 0).all(1) | np.isnan(n).any(1))
        lo = np.maximum(np.floor(g.min(1)).astype(np.int64), 0)
        hi = np.minimum(np.floor(g.max(1)).astype(np.int64), V - 1)
    ext = hi - lo + 1
    return np.where(valid & (ext > 0).all(1), ext.prod(1), 0)


def layer_plain(oracle, pos, mat, alb, ms=MS, G=G, V=V, depth=None, vp=None):
    """Level 0 of a mesh alone from the voxelizer without attributes: the layer of a context with voxel_attributes = 0."""
    p = oracle.default_params(V, G=G)
    return oracle.voxelize_conservative(p, oracle.make_scene(pos, mat, alb, ms, shadow_depth=depth, light_vp=vp))


def layer(oracle, pos, mat, alb, ms=MS, G=G, V=V, depth=None, vp=None):
    """(level 0, albedo, normal) of a mesh alone: what download_dynamic_voxels returns for it."""
    p = oracle.default_params(V, G=G)
    return oracle.voxelize_conservative_attr(p, oracle.make_scene(pos, mat, alb, ms, shadow_depth=depth, light_vp=vp))


def merge(D, S):
    return np.where((D[..., 3] > 0)[..., None], D, S)


def bricks(mask):
    """[V/8, V/8, V/8] bool: bricks with a set voxel."""
    n = mask.shape[0] // 8
    return mask.reshape(n, 8, n, 8, n, 8).any(axis=(1, 3, 5))


def non_degeneracy(D, S):
    """The counts that keep a merged-chain comparison from passing vacuously."""
    d, s = D[..., 3] > 0, S[..., 3] > 0
    bd, bs = bricks(d), bricks(s)
    shared = np.repeat(np.repeat(np.repeat(bd & bs, 8, 0), 8, 1), 8, 2)
    return dict(dynamic_voxels=int(d.sum()),
                both_differ=int((d & s & (D != S).any(-1)).sum()),
                dynamic_only_bricks=int((bd & ~bs).sum()),
                shared_bricks=int((bd & bs).sum()),
                dynamic_bricks=int(bd.sum()),
                static_only_in_shared=int((s & ~d & shared).sum()))


def assert_non_degenerate(D, S):
    n = non_degeneracy(D, S)
    assert n["both_differ"] >= 10 and n["dynamic_only_bricks"] >= 1 and n["shared_bricks"] >= 1 and \
        n["static_only_in_shared"] >= 1, n
    return n
