"""An independent float64 answer to "which surface does this pixel see, and where": a NumPy ray caster that shares
nothing with the rasterisers' algorithm (no clipping, no snapping, no edge functions).  Test infrastructure.

For every pixel centre a ray is un-projected through the inverse view-projection (NDC z = -1 to +1), intersected
with every triangle (Moeller-Trumbore, float64), back faces skipped, and the hit with the smallest NDC depth inside
[0, 1) kept: triangle index, world position, depth.

Where the rasteriser may legitimately answer differently -- and the pixels compare() therefore leaves out:

* delta (edge distance).  Coverage is decided on window coordinates snapped to 1/256 pixel: a vertex moves at most
  2^-9 pixel per axis, sqrt(2) * 2^-9 in the plane, and a point of an edge is a convex combination of its two
  end points, so the edge moves by no more than that anywhere.  Before the snap the window coordinate is an fp32
  result of about eight rounded operations (three products and sums of the transform, the reciprocal of w, the
  viewport scale and bias): at most 8 * 2^-24 relative, per axis.  Per triangle, with c_max its largest window
  coordinate in magnitude:           delta_t = sqrt(2) * (2^-9 + 8 * 2^-24 * c_max).
  Inside a 200-pixel frame the second term is 1e-4 pixel; a near-clipped triangle that projects to 4e5 pixels gets
  0.27 pixel.  A pixel is left out when its centre is within delta_t of an edge of the clipped polygon of any
  front-facing triangle t (edges of zero-area and back-facing triangles decide nothing).
* epsilon (depth ties).  fp32 depth in [0.5, 1) has a spacing of 2^-24; the barycentric chain (two divisions, three
  products, two sums, the 0.5 * z + 0.5 of each vertex) stays within 16 of them = 2^-20, and the 24-bit shadow map
  adds 2^-25.  The snap tilts each surface: its depth at a fixed pixel moves by at most |grad z| * delta_t.
  A pixel is left out when the two nearest hits a, b satisfy
        |z_a - z_b| <= 2^-20 + |grad z_a| * delta_a + |grad z_b| * delta_b.
"""
import numpy as np

import geomcases

DEPTH_EPS0 = 2.0 ** -20


def _matrix(vp):
    return np.asarray(vp, np.float32).reshape(4, 4).T.astype(np.float64)


def world_triangles(pos, model_scale):
    return (np.asarray(pos, np.float32).reshape(-1, 3, 3) * np.float32(model_scale)).astype(np.float64)


def cast(pos, model_scale, vp, w, h):
    """Returns dict(tri [h,w] int (-1: nothing), pos [h,w,3], depth [h,w] (1.0: nothing), second [h,w] depth of the
    second-nearest hit (inf: none), tri2 [h,w])."""
    M = _matrix(vp)
    Minv = np.linalg.inv(M)
    hand = np.sign(np.linalg.det(M))
    T = world_triangles(pos, model_scale)
    py, px = np.mgrid[0:h, 0:w]
    nx, ny = (px + 0.5) * 2.0 / w - 1.0, (py + 0.5) * 2.0 / h - 1.0
    ones = np.ones_like(nx)

    def unproject(z):
        q = np.stack([nx, ny, z * ones, ones], -1) @ Minv.T
        return q[..., :3] / q[..., 3:4]
    o = unproject(-1.0).reshape(-1, 3)
    d = unproject(1.0).reshape(-1, 3) - o
    npx = w * h
    best = np.full(npx, np.inf)
    second = np.full(npx, np.inf)
    tri = np.full(npx, -1, np.int64)
    tri2 = np.full(npx, -1, np.int64)
    P = np.zeros((npx, 3))
    for t, (a, b, c) in enumerate(T):
        e1, e2 = b - a, c - a
        n = np.cross(e1, e2)
        if not np.isfinite(n).all() or not n.any():
            continue
        pvec = np.cross(d, e2)
        det = pvec @ e1
        facing = -det * hand                      # det = -d . (e1 x e2); the projective map keeps or flips orientation
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - a
            u = (tv * pvec).sum(1) * inv
            qv = np.cross(tv, e1)
            v = (d * qv).sum(1) * inv
            s = (qv @ e2) * inv
        hit = (facing > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (s >= 0) & (s <= 1)
        idx = np.nonzero(hit)[0]
        if idx.size == 0:
            continue
        X = o[idx] + d[idx] * s[idx, None]
        cl = X @ M[:, :3].T + M[:, 3]
        z = cl[:, 2] / cl[:, 3] * 0.5 + 0.5
        ok = (cl[:, 3] > 0) & (z >= 0.0) & (z < 1.0)
        idx, X, z = idx[ok], X[ok], z[ok]
        nearer = z < best[idx]
        # second-nearest bookkeeping
        i1 = idx[nearer]
        second[i1] = best[i1]; tri2[i1] = tri[i1]
        i2 = idx[~nearer]
        m2 = z[~nearer] < second[i2]
        second[i2[m2]] = z[~nearer][m2]; tri2[i2[m2]] = t
        best[i1] = z[nearer]; tri[i1] = t; P[i1] = X[nearer]
    depth = np.where(tri >= 0, best, 1.0)
    return dict(tri=tri.reshape(h, w), pos=P.reshape(h, w, 3), depth=depth.reshape(h, w),
                second=second.reshape(h, w), tri2=tri2.reshape(h, w))


def _seg_dist(X, Y, p, q):
    dx, dy = q - p
    L2 = dx * dx + dy * dy
    if L2 == 0.0:
        return np.hypot(X - p[0], Y - p[1])
    t = np.clip(((X - p[0]) * dx + (Y - p[1]) * dy) / L2, 0.0, 1.0)
    return np.hypot(X - (p[0] + t * dx), Y - (p[1] + t * dy))


def left_out(pos, model_scale, vp, w, h, rc):
    """Boolean [h,w]: the pixels where the 1/256 snap or fp32 depth may legitimately decide differently."""
    _, polys = geomcases.clip_polygons(pos, model_scale, vp)
    n = len(polys)
    delta = np.zeros(n)
    grad = np.zeros(n)
    out = np.zeros((h, w), bool)
    cy, cx = np.mgrid[0:h, 0:w] + 0.5
    for t, poly in enumerate(polys):
        if len(poly) < 3 or not (poly[:, 3] > 1e-20).all():
            continue
        ndc = poly[:, :3] / poly[:, 3:4]
        win = (ndc[:, :2] * 0.5 + 0.5) * np.array([w, h], np.float64)
        z = ndc[:, 2] * 0.5 + 0.5
        area = sum(win[i, 0] * win[(i + 1) % len(win), 1] - win[(i + 1) % len(win), 0] * win[i, 1] for i in range(len(win)))
        delta[t] = np.sqrt(2.0) * (2.0 ** -9 + 8.0 * 2.0 ** -24 * np.abs(win).max())
        if not area > 0.0:                        # back-facing or zero area: its edges decide nothing
            continue
        # depth is affine in window coordinates on the triangle's plane: least squares over the polygon's vertices
        A = np.c_[win - win.mean(0), np.ones(len(win))]
        g = np.linalg.lstsq(A, z, rcond=None)[0]
        grad[t] = np.hypot(g[0], g[1])
        dl = delta[t]
        x0, x1 = max(0, int(np.floor(max(win[:, 0].min() - dl, 0))) - 1), min(w - 1, int(np.ceil(min(win[:, 0].max() + dl, w))) + 1)
        y0, y1 = max(0, int(np.floor(max(win[:, 1].min() - dl, 0))) - 1), min(h - 1, int(np.ceil(min(win[:, 1].max() + dl, h))) + 1)
        if x1 < x0 or y1 < y0:
            continue
        X, Y = cx[y0:y1 + 1, x0:x1 + 1], cy[y0:y1 + 1, x0:x1 + 1]
        near = np.zeros(X.shape, bool)
        for i in range(len(win)):
            near |= _seg_dist(X, Y, win[i], win[(i + 1) % len(win)]) <= dl
        # the far plane is not an edge of the polygon: the line where the surface reaches depth 1 moves with the snap
        # too, and a surface AT depth 0 or 1 is a tie with the range itself (both inside the polygon, widened by delta)
        inside = np.ones(X.shape, bool)
        for i in range(len(win)):
            p, q = win[i], win[(i + 1) % len(win)]
            ln = np.hypot(*(q - p))
            if ln > 0.0:
                inside &= ((q[0] - p[0]) * (Y - p[1]) - (q[1] - p[1]) * (X - p[0])) / ln >= -dl
        zp = g[0] * (X - win[:, 0].mean()) + g[1] * (Y - win[:, 1].mean()) + g[2]
        band = DEPTH_EPS0 + grad[t] * dl
        near |= inside & ((np.abs(zp - 1.0) <= band) | (np.abs(zp) <= band))
        out[y0:y1 + 1, x0:x1 + 1] |= near
    a, b = rc["tri"], rc["tri2"]
    both = (a >= 0) & (b >= 0)
    eps = DEPTH_EPS0 + grad[np.maximum(a, 0)] * delta[np.maximum(a, 0)] + grad[np.maximum(b, 0)] * delta[np.maximum(b, 0)]
    out |= both & (np.abs(rc["second"] - rc["depth"]) <= eps)
    return out


def extent(pos, model_scale):
    """The scene extent errors are stated against: the largest |coordinate| of the scaled mesh."""
    return float(np.abs(world_triangles(pos, model_scale)).max())


def compare(rc, skip, planes, w, h, depth_map=None):
    """Rasteriser output against the ray caster outside `skip`.  Returns dict(cover_mismatch, owner_mismatch (pixel
    counts, must be 0), pos_err (per plane 0, 1, 2: largest |difference| over the compared covered pixels, absolute),
    depth_err (largest |depth_map - depth|, when a depth map of the same camera and frame is given))."""
    p = np.asarray(planes).reshape(23, h, w)
    covered = p[18] >= 0.5
    own = geomcases.owner_of(planes, w, h)
    use = ~skip
    r = dict(cover_mismatch=int(((covered != (rc["tri"] >= 0)) & use).sum()),
             owner_mismatch=int(((own != rc["tri"]) & use).sum()), left_out=float(skip.mean()))
    both = use & covered & (rc["tri"] >= 0) & (own == rc["tri"])
    got = np.moveaxis(p[0:3].astype(np.float64), 0, -1)
    r["pos_err"] = [float(np.abs(got - rc["pos"])[both][:, k].max()) if both.any() else 0.0 for k in range(3)]
    r["first_bad"] = [tuple(int(v) for v in yx) for yx in
                      np.argwhere(((covered != (rc["tri"] >= 0)) | (own != rc["tri"])) & use)[:8]]
    if depth_map is not None:
        dm = np.asarray(depth_map, np.float64).reshape(h, w)
        r["depth_err"] = float(np.abs(dm - rc["depth"])[use].max()) if use.any() else 0.0
    return r


# ---- the scenes of the ray-caster comparison ---------------------------------------------------------------------
# The Cornell box through the host library's perspective camera, and the opaque part of the geomcases scenes.  Not
# among them, because their whole purpose is to put pixels ON the decisions this comparison must leave out: the
# pixel-aligned cases (pixel_grid: 63 % of the frame within delta of an edge, depth_ties: 35 %, single_pixel: its only
# pixel), depth_planes (19 %: surfaces exactly at depth 0 and 1) and the triangles of near_plane_fan whose clipped
# polygon projects beyond 2^16 pixels (delta_t grows to pixels there).  Those are held bit for bit to the checker
# instead (test_gpu_raster_edges.py), and the checker to this ray caster on everything listed here.
RC_NAMES = ["cornell", "near_plane_fan_below16", "slivers", "slivers_200x120", "full_frame_and_small_opaque",
            "alpha_cards_opaque", "single_triangle_17x9", "single_triangle_1x1"]
_RC = {}


def rc_case(name):
    if name in _RC:
        return _RC[name]
    if name == "cornell":
        import vctpkg
        vctpkg.load()
        from voxel_cone_tracing_amd import scene as sc
        s = sc.Scene(0, 1.0, 1234)
        w, h = 160, 100
        cam = sc.default_camera(position=(0.0, 0.0, 58.0))
        c = geomcases.Case("cornell", s.pos, sc.camera_view_proj(cam, w, h), w, h, 0.05, {}, shadow_size=128,
                           light_vp=sc.light_view_proj((0.0, 1.0, 0.25)))
    elif name == "near_plane_fan_below16":
        fan = geomcases.get_case("near_plane_fan")
        c = fan.subset(~geomcases.classify_case(fan)["beyond16"], name)
    elif name.endswith("_opaque"):
        full = geomcases.get_case(name[:-7])
        c = full.subset(full.opaque, name)
    else:
        c = geomcases.get_case(name)
    _RC[name] = c
    return c


_RC_TRUTH = {}


def rc_truth(name):
    """((ray cast, left-out mask) of the camera frame, the same of the shadow-map frame), cached per case."""
    if name not in _RC_TRUTH:
        c = rc_case(name)
        S = c.shadow_size
        with np.errstate(all="ignore"):
            a = cast(c.pos, c.model_scale, c.vp, c.w, c.h)
            b = cast(c.pos, c.model_scale, c.light_vp, S, S)
        _RC_TRUTH[name] = ((a, left_out(c.pos, c.model_scale, c.vp, c.w, c.h, a)),
                           (b, left_out(c.pos, c.model_scale, c.light_vp, S, S, b)))
    return _RC_TRUTH[name]


def rc_errors(name, planes, depth_map):
    """compare() of a G-buffer and a shadow map of rc_case(name), errors divided by the scene extent (positions;
    depth is already a fraction of the depth range)."""
    c = rc_case(name)
    (a, skip_a), (b, skip_b) = rc_truth(name)
    r = compare(a, skip_a, planes, c.w, c.h)
    ext = extent(c.pos, c.model_scale)
    r["pos_rel"] = [e / ext for e in r["pos_err"]]
    dm = np.asarray(depth_map, np.float64)
    use = ~skip_b
    r["shadow_left_out"] = float(skip_b.mean())
    r["shadow_cover_mismatch"] = int((((dm < 1.0) != (b["tri"] >= 0)) & use).sum())
    r["depth_err"] = float(np.abs(dm - b["depth"])[use].max()) if use.any() else 0.0
    return r


# Measured: the CPU checker (oracle/vct_oracle_raster.cpp) against this ray caster, largest error per case outside the
# left-out set; positions per plane 0 / 1 / 2 as a fraction of the scene extent (largest |coordinate| of the scaled
# mesh), depth as a fraction of the depth range.  The bars are these times 4 (the fp32 rounding of the interpolation
# chain may differ between two correct implementations; the snap itself, which dominates, may not).  The GPU's own error
# is never the source of a bar.  tests/test_raster_cases.py re-measures the checker against the bars on every run.
RC_MEASURED = {
    # name: ((pos x, pos y, pos z), shadow-map depth)                                left out: frame / shadow map
    "cornell": ((9.73e-06, 7.1e-05, 0.000125), 6.37e-05),                          # 0.62 % / 0.02 %
    "near_plane_fan_below16": ((2e-06, 2.37e-06, 1.29e-05), 0.000216),             # 0.60 % / 0.27 %
    "slivers": ((4.68e-08, 4.68e-08, 3.65e-10), 5.96e-08),                         # 0.43 % / 1.09 %
    "slivers_200x120": ((7.19e-08, 7.57e-08, 6.36e-10), 5.96e-08),                 # 0.40 % / 0.71 %
    "full_frame_and_small_opaque": ((3.12e-06, 3.18e-06, 6.78e-08), 5.11e-05),     # 0.10 % / 0.14 %
    "alpha_cards_opaque": ((1.01e-07, 3.97e-08, 1.24e-09), 1.19e-07),              # 0.00 % / 1.04 %
    "single_triangle_17x9": ((3.91e-05, 3.43e-08, 4.83e-07), 3.38e-05),            # 0.65 % / 0.35 %
    "single_triangle_1x1": ((0.000307, 0.0, 1.67e-05), 2.93e-05),                  # 0.00 % / 0.00 %
}
RC_FLOOR = 2.0 ** -23          # one fp32 spacing of a value of the extent's size: no bar is asked to be finer than 4 of them
LEFT_OUT_MAX = 0.02
RC_BAR_FACTOR = 4.0


def rc_bars(name):
    (px, py, pz), d = RC_MEASURED[name]
    f = RC_BAR_FACTOR
    return tuple(max(v, RC_FLOOR) * f for v in (px, py, pz)), max(d, RC_FLOOR) * f


def check_against_ray_caster(name, planes, depth_map, who):
    """Asserts a G-buffer and a shadow map of rc_case(name) against the ray caster and the bars; prints every figure first."""
    r = rc_errors(name, planes, depth_map)
    pos_bar, depth_bar = rc_bars(name)
    print(who, name, "left out %.4f / %.4f" % (r["left_out"], r["shadow_left_out"]), "pos", r["pos_rel"], "bars", pos_bar,
          "depth", r["depth_err"], "bar", depth_bar)
    assert r["left_out"] <= LEFT_OUT_MAX and r["shadow_left_out"] <= LEFT_OUT_MAX
    assert r["cover_mismatch"] == 0 and r["owner_mismatch"] == 0, r["first_bad"]
    assert r["shadow_cover_mismatch"] == 0
    for k in range(3):
        assert r["pos_rel"][k] <= pos_bar[k], (k, r["pos_rel"][k], pos_bar[k])
    assert r["depth_err"] <= depth_bar, (r["depth_err"], depth_bar)
