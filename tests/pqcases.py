"""Inputs of the point-query tests (include/vct.h "point queries"): the chain and four families of points, NumPy only.

    patch     a 16 x 16 lattice on a gently curved floor, spacing vs / 4, row-major: a lightmap.  Spatially ordered.
    scatter   points uniform in +-0.45 G with random frames: nothing two lanes of a wave could share.
    mixed     `patch` shuffled by a fixed permutation: what VCT_QUERY_SORT_CELLS is for.
    edge      the adversarial positions and frames of tests/gbcases.py restated as points, plus NaN and +-inf in every field.

footprints() restates where csrc/vct_trace.hip sample_level puts a lane's trilinear footprint, so that
tests/test_point_query_cases.py can say which sampler path a wave of 64 consecutive points takes before a GPU sees it."""
import numpy as np

import gbcases as gc
import point_query_ref as pq

f32 = np.float32
V, G, MAX_DISTANCE = 32, 150.0, 75.0
VS = f32(G) / f32(V)
MODEL_SCALE = f32(0.05)
TAN_DIFFUSE, TAN_SPECULAR = f32(0.577), f32(0.07)
FINITE, NONFINITE = "finite", "nonfinite"
CASES = ("patch", "scatter", "mixed", "edge")
SIZES = (1, 63, 64, 65, 257)          # the wave boundary on both sides


def level0():
    import synth
    return synth.noise_volume(V, occupancy=0.12)


def config(**kw):
    return dict(voxel_dim=V, width=8, height=8, grid_world_size=G, max_distance=MAX_DISTANCE, **kw)


def _pack(P, n, t, b):
    return np.ascontiguousarray(np.concatenate([P, n * MODEL_SCALE, t * MODEL_SCALE, b * MODEL_SCALE], axis=1), f32)


def patch(origin=(-9.0, -20.0, 4.0)):
    j, i = np.meshgrid(np.arange(16, dtype=np.float64), np.arange(16, dtype=np.float64), indexing="ij")
    x = origin[0] + i.ravel() * float(VS) / 4
    z = origin[2] + j.ravel() * float(VS) / 4
    y = origin[1] + 3.0 * np.sin(x * 0.05) * np.cos(z * 0.04)
    dydx = 3.0 * 0.05 * np.cos(x * 0.05) * np.cos(z * 0.04)
    dydz = -3.0 * 0.04 * np.sin(x * 0.05) * np.sin(z * 0.04)
    n = np.stack([-dydx, np.ones_like(x), -dydz], axis=1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    t = np.stack([np.ones_like(x), dydx, np.zeros_like(x)], axis=1)
    t -= n * (t * n).sum(1, keepdims=True)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return _pack(np.stack([x, y, z], axis=1), n, t, np.cross(n, t))


def scatter(n=256, seed=5):
    r = np.random.default_rng(seed)
    P = r.uniform(-0.45 * G, 0.45 * G, (n, 3))
    nn = r.normal(size=(n, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    h = np.where(np.abs(nn[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = np.cross(h, nn)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return _pack(P, nn, t, np.cross(nn, t))


def mixed(seed=9):
    p = patch()
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(p.shape[0])])


def _env():
    env = gc.Env(G)
    env.vs = VS                      # gbcases' own grid is 16^3: the texel and limit specs take the voxel size from here
    return env


def exceeds_position_bound(points, reach=1.0):
    """The point contract of include/vct.h in float64: finite position and normal, and
    |P| + |N| vs + max_distance * max(1, |direction|) > LIMIT * G on some axis (reach = max(1, |direction|))."""
    g = np.asarray(points, np.float64)
    lhs = np.abs(g[:, 0:3]) + np.abs(g[:, 3:6]) * (G / V) + MAX_DISTANCE * np.asarray(reach, np.float64).reshape(-1, 1)
    with np.errstate(invalid="ignore"):
        return np.isfinite(g[:, 0:6]).all(1) & (lhs > gc.LIMIT_GRIDS * G).any(1)


def edge():
    """(points [n, 12], cls [n]).  cls says whether the start point and all six directions are finite (the oracle's
    gather is then finite) or the point is one whose cones take one step and return NaN; gbcases declares the class of its
    specs from the arithmetic, the non-finite fields below are non-finite by construction."""
    env = _env()
    base = patch()[0]
    pts, cls = [], []
    specs = gc._positions(env, False) + gc._tangent_frames(env, False) + gc._frame_scales(env, False)
    for spec in specs:
        px = np.zeros(23, f32)
        px[0:12] = base
        px[12:15], px[18] = [0, 1, 0], 1.0
        with np.errstate(all="ignore"):
            c = spec(px)
        pts.append(px[0:12].copy())
        cls.append(FINITE if c == gc.FINITE else NONFINITE)
    for k in range(12):
        for v in (gc.NAN, gc.INF, -gc.INF):
            p = base.copy()
            p[k] = v
            pts.append(p)
            cls.append(NONFINITE)
    return np.ascontiguousarray(np.stack(pts), f32), np.array(cls, object)


def edge_cones():
    """Cone points [n, 9] for the single-cone query: unit, short and zero directions from ordinary and edge positions,
    and NaN / +-inf in the direction."""
    pts, _ = edge()
    base = patch()
    rows = []
    for i, d in enumerate([(0.0, 1.0, 0.0), (0.6, 0.8, 0.0), (0.3, 0.4, 0.0), (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0),
                           (0.0, 0.25, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0)]):
        for src in (base[17 * i], base[255 - i], pts[i], pts[20 + i]):
            rows.append(np.concatenate([src[0:6], np.array(d, f32)]))
    for k in range(3):
        for v in (gc.NAN, gc.INF, -gc.INF):
            d = np.array([0.0, 1.0, 0.0], f32)
            d[k] = v
            rows.append(np.concatenate([base[3][0:6], d]))
    for p in pts[::3]:
        rows.append(np.concatenate([p[0:6], np.array([0.0, 1.0, 0.0], f32)]))
    return np.ascontiguousarray(np.stack(rows), f32)


def get(name):
    if name == "edge":
        return edge()[0]
    return {"patch": patch, "scatter": scatter, "mixed": mixed}[name]()


def take(points, n):
    """n points: the first n, the list repeated cyclically where it is shorter."""
    return np.ascontiguousarray(points[np.arange(n) % points.shape[0]])


# ---- where the sampler puts a footprint --------------------------------------------------------------------------------
def step_table(tan_half):
    """[(dist, [levels])] of trace.fs:90-104 for this grid: the levels a step samples (one, or two when it blends)."""
    out = []
    maxl = int(np.log2(V))
    dist = VS
    while dist < f32(MAX_DISTANCE):
        diameter = max(VS, f32(2.0) * f32(tan_half) * dist)
        lod = f32(np.log2(diameter / VS))
        if not lod > 0:
            levels = [0]
        else:
            lam = min(lod, f32(maxl))
            lo = int(np.floor(lam))
            levels = [lo] if lam == lo else [lo, min(lo + 1, maxl)]
        out.append((dist, levels))
        dist = f32(dist + diameter)
    return out


def footprints(points, dirs, dist, level):
    """int64 [n, 3]: (i0, j0, k0), the lower corner of each point's trilinear footprint at `level` for the sample at
    start + dir * dist -- csrc/vct_trace.hip VCT_MARCH_STEP + sample_level in fp32 (unfolded: the GL_REPEAT fold and the
    clamp come after the cooperative test)."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 12)
    d = np.asarray(dirs, f32).reshape(-1, 3)
    N = f32(V >> level)
    half_G = f32(G) * f32(0.5)
    out = np.zeros((pts.shape[0], 3), np.int64)
    for a in range(3):
        start = pts[:, a] + pts[:, 3 + a] * VS
        p = start + d[:, a] * f32(dist)
        u = (p / half_G) * f32(0.5) + f32(0.5)
        out[:, a] = np.floor(u * N - f32(0.5)).astype(np.int64)
    return out


def wave_spreads(oracle, points, tan_half=TAN_DIFFUSE):
    """For every wave of 64 consecutive points, cone, march step and sampled level: dict(wave, cone, step, level,
    spread = the largest per-axis range of the lanes' footprint corners, anchor = the corner of lane 27 -- the sampler's
    anchor while that lane marches -- or of the wave's last lane)."""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 12)
    dirs = pq.cone_dirs(oracle, pts)
    rows = []
    for s, (dist, levels) in enumerate(step_table(tan_half)):
        for level in levels:
            for c in range(6):
                fp = footprints(pts, dirs[:, c], dist, level)
                for w in range(0, pts.shape[0], 64):
                    q = fp[w:w + 64]
                    rows.append(dict(wave=w // 64, cone=c, step=s, level=level, spread=int((q.max(0) - q.min(0)).max()),
                                     anchor=q[min(27, q.shape[0] - 1)]))
    return rows
