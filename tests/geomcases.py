"""Meshes built to hit the decision points of the raster input stages (csrc/vct_raster.hip), each with a raw
column-major float32[16] view-projection, and a NumPy float64 classifier that says which decision points a case
really reaches.  Test infrastructure: only tests/ may import this.  No GPU, no library: NumPy alone.

A Case carries everything both sides take: ctx.upload_triangles / upload_mesh_attributes / upload_mesh_uvs /
upload_textures and pyoracle.make_mesh.  Every triangle has its own material whose albedo red channel is
(index + 1) / 4096 (exact in fp32), so the triangle a pixel shows is readable from G-buffer plane 15
(owner_of()); textured (alpha-tested) triangles take the texture's colour there instead.

"Aligned" cases use an orthographic matrix on a power-of-two frame, vertices on the 1/256-pixel grid and
model_scale = 1/16: every fp32 operation between the vertex and its snapped window coordinate is then exact, so a
vertex sits EXACTLY on a pixel centre, a clip plane or depth 0 / 1, and the float64 classifier sees the very numbers
the rasteriser decides on.  classify() checks that claim (counts["inexact_vertices"] == 0) instead of trusting it.
"""
import numpy as np

ALIGNED_SCALE = 0.0625          # exact in fp32, and not the library's default 0.05
ID_STEP = 1.0 / 4096.0


class Case:
    def __init__(self, name, pos, vp, w, h, model_scale, minimum, aligned=False, alpha=None, shadow_size=None,
                 light_vp=None):
        self.name, self.w, self.h, self.model_scale, self.aligned = name, int(w), int(h), float(model_scale), aligned
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
        n = self.ntri = self.pos.shape[0]
        assert n < 4095
        self.vp = np.ascontiguousarray(vp, np.float32).reshape(16)
        self.light_vp = self.vp if light_vp is None else np.ascontiguousarray(light_vp, np.float32).reshape(16)
        self.shadow_size = int(shadow_size or max(w, h))
        self.minimum = dict(minimum)              # classifier counts the case must reach (asserted by every test)
        self.material = np.arange(n, dtype=np.int32)
        self.albedo = np.zeros((n, 4), np.float32)
        self.albedo[:, 0] = (np.arange(n) + 1) * ID_STEP
        self.albedo[:, 1] = 0.5
        self.albedo[:, 2] = 0.25
        self.albedo[:, 3] = 1.0
        self.specular = np.tile(np.array([0.25, 0.5, 0.125], np.float32), (n, 1))
        self.specular[::3, 1:] = 0.0               # both branches of trace.fs:210
        self.uv = np.zeros((n, 6), np.float32)
        self.mat_tex = np.full((n, 3), -1, np.int32)
        self.textures = []
        self.alpha = np.zeros(n, bool) if alpha is None else np.asarray(alpha, bool)
        if self.alpha.any():
            self.textures = [alpha_texture()]
            self.mat_tex[self.alpha, 0] = 0
            rng = np.random.default_rng(7)
            for t in np.nonzero(self.alpha)[0]:   # uv scale from magnified to strongly minified: every mip level
                s = float(2.0 ** rng.integers(-2, 4))
                self.uv[t] = (np.array([0, 0, 1, 0, 0, 1], np.float32) * s + rng.random(1).astype(np.float32))
        self.opaque = ~self.alpha

    def frames(self):
        """(normal, tangent, bitangent) [n, 9]: the geometric frame, or the z frame for a zero-area triangle."""
        p = self.pos.reshape(-1, 3, 3).astype(np.float64)
        nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        ln = np.linalg.norm(nrm, axis=1)
        ok = np.isfinite(ln) & (ln > 0)
        nrm[~ok] = (0.0, 0.0, 1.0)
        nrm[ok] /= ln[ok, None]
        ref = np.where(np.abs(nrm[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
        tan = np.cross(ref, nrm)
        tan /= np.linalg.norm(tan, axis=1)[:, None]
        bit = np.cross(nrm, tan)
        rep = lambda a: np.ascontiguousarray(np.repeat(a[:, None, :], 3, 1).reshape(-1, 9), np.float32)
        return rep(nrm), rep(tan), rep(bit)

    def mesh_args(self):
        """(pos, material, albedo, specular, frames, uv) -- what upload_* and pyoracle.make_mesh take."""
        return self.pos, self.material, self.albedo, self.specular, self.frames(), self.uv

    def subset(self, keep, name=None):
        """The case restricted to the triangles of a boolean mask (ids renumbered), same camera and frame."""
        c = Case(name or self.name + "_opaque", self.pos[keep], self.vp, self.w, self.h, self.model_scale, {},
                 self.aligned, None, self.shadow_size, self.light_vp)
        return c

    def __repr__(self):
        return f"Case({self.name}, {self.ntri} tris, {self.w}x{self.h})"


def alpha_texture(n=16):
    """RGBA8 [n, n, 4]: 2x2-texel checker of alpha 255 / 0 with a colour ramp (mip levels average to alpha ~ 0.5)."""
    t = np.zeros((n, n, 4), np.uint8)
    j, i = np.mgrid[0:n, 0:n]
    t[..., 0] = (i * 255) // (n - 1)
    t[..., 1] = (j * 255) // (n - 1)
    t[..., 2] = 128
    t[..., 3] = np.where(((i // 2) + (j // 2)) % 2 == 0, 255, 0)
    t[: n // 4, : n // 4, 3] = 255            # an opaque corner, so that coarse levels are not all exactly 0.5
    return t


def owner_of(planes, w, h):
    """Triangle index shown by every pixel (-1: not covered), from plane 15 (albedo red).  Opaque cases only."""
    p = np.asarray(planes).reshape(23, -1)
    own = np.rint(p[15].astype(np.float64) / ID_STEP).astype(np.int64) - 1
    own[p[18] < 0.5] = -1
    return own.reshape(h, w)


# ---------------------------------------------------------------------------------------------------------------
# matrices (column-major float32[16]: element [4 * col + row])
def ortho_pixels(w, h, zscale=1.0):
    """World (x, y) in pixels -> the same window coordinates; world z in [-zscale, 0] -> depth [1, 0].
    Exact in fp32 for power-of-two w, h and coordinates on the 1/256 grid."""
    m = np.zeros((4, 4), np.float64)
    m[0, 0], m[0, 3] = 2.0 / w, -1.0
    m[1, 1], m[1, 3] = 2.0 / h, -1.0
    m[2, 2], m[2, 3] = -2.0 / zscale, -1.0
    m[3, 3] = 1.0
    return np.ascontiguousarray(m.T, np.float32).reshape(16)


def perspective_origin(w, h, cot=2.0, near=1.0, far=3.0):
    """Camera at the origin looking down -z, no view rotation: w_clip = -z exactly, and with near = 1, far = 3 the
    depth row is (-2, -3), so z = -1 is exactly on the near plane and z = 0 exactly on w = 0."""
    m = np.zeros((4, 4), np.float64)
    m[0, 0] = cot * h / w
    m[1, 1] = cot
    m[2, 2] = -(far + near) / (far - near)
    m[2, 3] = -2.0 * far * near / (far - near)
    m[3, 2] = -1.0
    return np.ascontiguousarray(m.T, np.float32).reshape(16)


# ---------------------------------------------------------------------------------------------------------------
# the classifier
def _snap(u):
    return np.floor(u * 256.0 + 0.5) / 256.0


def clip_polygons(pos, model_scale, vp):
    """Per triangle: clip coordinates [n,3,4] (float64 from the fp32-scaled vertices) and the list of near-clipped
    polygons (each [k,4], k in 0,3,4), by the rule both rasterisers state: keep z >= -w, cut where the sign changes."""
    p32 = (np.asarray(pos, np.float32).reshape(-1, 3) * np.float32(model_scale)).astype(np.float64)
    M = np.asarray(vp, np.float32).reshape(4, 4).T.astype(np.float64)
    clip = (p32 @ M[:, :3].T + M[:, 3]).reshape(-1, 3, 4)
    polys = []
    for c in clip:
        d = c[:, 2] + c[:, 3]
        out = []
        for i in range(3):
            a, b = c[i], c[(i + 1) % 3]
            da, db = d[i], d[(i + 1) % 3]
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                out.append(a + (b - a) * (da / (da - db)))
        polys.append(np.array(out).reshape(-1, 4))
    return clip, polys


def window_subtris(poly, w, h):
    """Fan sub-triangles (0, t, t+1) of a clipped polygon in window space: list of (unsnapped [3,2], depth [3]);
    a sub-triangle with a vertex at w <= 1e-20 is dropped, as both rasterisers drop it."""
    out = []
    for t in range(1, len(poly) - 1):
        v = poly[[0, t, t + 1]]
        if not (v[:, 3] > 1e-20).all():
            out.append(None)
            continue
        ndc = v[:, :3] / v[:, 3:4]
        win = (ndc[:, :2] * 0.5 + 0.5) * np.array([w, h], np.float64)
        out.append((win, ndc[:, 2] * 0.5 + 0.5))
    return out


def _area(s):
    return (s[1, 0] - s[0, 0]) * (s[2, 1] - s[0, 1]) - (s[2, 0] - s[0, 0]) * (s[1, 1] - s[0, 1])


def classify(pos, model_scale, vp, w, h):
    """Which decision points of the rasteriser a mesh reaches, in float64.  Returns a dict of per-triangle arrays
    ("behind", "on_near", "w_zero", "w_neg", "beyond16", "beyond23", "zero_area", "zero_after_snap", "front",
    "dropped"), per-pixel maps ("on_edge", "on_vertex", "cover_count" [h,w]) and "counts", the totals tests assert."""
    clip, polys = clip_polygons(pos, model_scale, vp)
    n = clip.shape[0]
    d = clip[:, :, 2] + clip[:, :, 3]
    r = dict(behind=(d < 0).sum(1), on_near=(d == 0).sum(1), w_zero=(clip[:, :, 3] == 0).sum(1),
             w_neg=(clip[:, :, 3] < 0).sum(1))
    for k in ("beyond16", "beyond23", "zero_area", "zero_after_snap", "front", "dropped"):
        r[k] = np.zeros(n, bool)
    on_edge, on_vertex = np.zeros((h, w), bool), np.zeros((h, w), bool)
    cover = np.zeros((h, w), np.int32)
    pix_tris = {}
    edge_kind = dict(left=0, top=0, right=0, bottom=0, diagonal=0)
    depth0 = depth1 = inexact = sub_beyond16 = sub_below16_clipped = thin = 0
    cy, cx = np.mgrid[0:h, 0:w] + 0.5
    for t in range(n):
        subs = window_subtris(polys[t], w, h)
        for sub in subs:
            if sub is None:
                r["dropped"][t] = True
                continue
            win, z = sub
            s = _snap(win)
            inexact += int((s != win).any())
            depth0 += int((z == 0.0).sum())
            depth1 += int((z == 1.0).sum())
            big = np.abs(s).max()
            r["beyond16"][t] |= big >= 65536.0
            r["beyond23"][t] |= big >= 8388607.0
            a, a_un = _area(s), _area(win)
            if a == 0.0:
                r["zero_area"][t] = True
                r["zero_after_snap"][t] |= a_un != 0.0
                continue
            if a < 0.0:
                continue
            r["front"][t] = True
            if len(polys[t]) > 3 or r["behind"][t]:
                sub_beyond16 += int(big >= 65536.0)
                sub_below16_clipped += int(big < 65536.0)
            x0, x1 = max(0, int(np.floor(max(s[:, 0].min(), -1.0)))), min(w - 1, int(np.floor(min(s[:, 0].max(), w))))
            y0, y1 = max(0, int(np.floor(max(s[:, 1].min(), -1.0)))), min(h - 1, int(np.floor(min(s[:, 1].max(), h))))
            if x1 < x0 or y1 < y0:
                continue
            X, Y = cx[y0:y1 + 1, x0:x1 + 1], cy[y0:y1 + 1, x0:x1 + 1]
            e, own = [], []
            for k in range(3):
                i, j = (k + 1) % 3, (k + 2) % 3
                dx, dy = s[j, 0] - s[i, 0], s[j, 1] - s[i, 1]
                e.append(dx * (Y - s[i, 1]) - dy * (X - s[i, 0]))
                own.append((dy > 0.0) or (dy == 0.0 and dx < 0.0))
            e = np.array(e)
            inside_closed = (e >= 0.0).all(0)
            zero = (e == 0.0) & inside_closed
            nz = zero.sum(0)
            on_edge[y0:y1 + 1, x0:x1 + 1] |= nz >= 1
            on_vertex[y0:y1 + 1, x0:x1 + 1] |= nz >= 2
            covered = inside_closed.copy()
            for k in range(3):
                i, j = (k + 1) % 3, (k + 2) % 3
                dx, dy = s[j, 0] - s[i, 0], s[j, 1] - s[i, 1]
                cnt = int(zero[k].sum())
                if cnt:
                    edge_kind["left" if dy > 0 else "right" if dy < 0 else "top" if dx < 0 else "bottom"] += cnt
                    if dx != 0.0 and dy != 0.0:
                        edge_kind["diagonal"] += cnt
                if not own[k]:
                    covered &= ~zero[k]
            cover[y0:y1 + 1, x0:x1 + 1] += covered
            # thinner than a pixel: twice the area over the longest edge is the smallest height
            longest = max(np.hypot(*(s[(k + 1) % 3] - s[k])) for k in range(3))
            thin += int(a / longest < 1.0)
            for yy, xx in zip(*np.nonzero(inside_closed)):
                pix_tris.setdefault((y0 + int(yy), x0 + int(xx)), []).append(t)
    r.update(on_edge=on_edge, on_vertex=on_vertex, cover_count=cover, pix_tris=pix_tris)
    r["counts"] = dict(
        triangles=n, behind1=int((r["behind"] == 1).sum()), behind2=int((r["behind"] == 2).sum()),
        behind3=int((r["behind"] == 3).sum()), on_near=int(r["on_near"].sum()), w_zero=int(r["w_zero"].sum()),
        w_neg=int(r["w_neg"].sum()), beyond16=int(r["beyond16"].sum()), beyond23=int(r["beyond23"].sum()),
        clipped_sub_beyond16=sub_beyond16, clipped_sub_below16=sub_below16_clipped,
        zero_area=int(r["zero_area"].sum()), zero_after_snap=int(r["zero_after_snap"].sum()),
        front=int(r["front"].sum()), back=int((~r["front"] & ~r["zero_area"] & (r["behind"] < 3)).sum()),
        dropped=int(r["dropped"].sum()), pixels_on_edge=int(on_edge.sum()), pixels_on_vertex=int(on_vertex.sum()),
        edge_left=edge_kind["left"], edge_top=edge_kind["top"], edge_right=edge_kind["right"],
        edge_bottom=edge_kind["bottom"], edge_diagonal=edge_kind["diagonal"], depth0_vertices=depth0,
        depth1_vertices=depth1, inexact_vertices=inexact, thin=thin, covered_pixels=int((cover > 0).sum()),
        multi_covered_pixels=int((cover > 1).sum()), max_overdraw=int(cover.max()) if cover.size else 0)
    return r


def classify_case(case):
    return classify(case.pos, case.model_scale, case.vp, case.w, case.h)


def check_minimum(case, cls=None):
    """Asserts that the case still reaches what it is named for; returns the classification."""
    cls = cls or classify_case(case)
    c = cls["counts"]
    for k, v in case.minimum.items():
        if k.endswith("_max"):
            assert c[k[:-4]] <= v, (case.name, k, c[k[:-4]], v)
        else:
            assert c[k] >= v, (case.name, k, c[k], v)
    return cls


def verdict(cls, y, x):
    """What the classifier knows about pixel (y, x): for a failure message."""
    tris = cls["pix_tris"].get((int(y), int(x)), [])
    keys = ("behind", "on_near", "w_zero", "w_neg", "beyond16", "beyond23", "zero_area", "front")
    return dict(pixel=(int(y), int(x)), on_edge=bool(cls["on_edge"][y, x]), on_vertex=bool(cls["on_vertex"][y, x]),
                triangles={int(t): {k: int(cls[k][t]) for k in keys} for t in tris[:6]})


# ---------------------------------------------------------------------------------------------------------------
# builders.  Coordinates are written in the unit the matrix sees (pixels / eye space) and divided by the case's
# model_scale at the end, so the kernel's v * model_scale gives them back.
def _finish(name, tris, vp, w, h, scale, minimum, **kw):
    pos = np.asarray(tris, np.float64).reshape(-1, 9) / scale
    return Case(name, pos, vp, w, h, scale, minimum, **kw)


def _front_facing(tri, vp, w, h, want_front=True):
    """tri [3,3] with its winding turned so that the classifier calls it front (or back) facing, where it can tell."""
    c = classify(np.asarray(tri, np.float64).reshape(1, 9), 1.0, vp, w, h)
    is_front = bool(c["front"][0])
    has_area = is_front or c["counts"]["back"] > 0
    if has_area and is_front != want_front:
        return [tri[0], tri[2], tri[1]]
    return tri


def near_plane_fan(w=67, h=45):
    """Perspective camera at the origin; a fan of triangles around the view axis whose outer vertices go behind the
    near plane in every combination.  Eye-space units; near = 1, far = 3."""
    vp = perspective_origin(w, h)
    rng = np.random.default_rng(11)
    tris = []
    N = 72
    for i in range(N):
        ang = 2.0 * np.pi * i / N
        ca, sa = np.cos(ang), np.sin(ang)
        kind = i % 9
        zin = -1.5 - 1.25 * rng.random()                       # inside the depth range
        A = [0.3 * ca * rng.random(), 0.3 * sa * rng.random(), zin]
        front = lambda r, z: [r * ca - 0.2 * sa, r * sa + 0.2 * ca, z]
        side = lambda r, z: [r * ca + 0.2 * sa, r * sa - 0.2 * ca, z]
        if kind == 0:      # nothing behind
            B, C = front(0.6, -2.0), side(0.6, -2.5)
        elif kind == 1:    # one behind, close by: stays below 2^16
            B, C = front(0.6, -2.0), side(0.5, 0.5)
        elif kind == 2:    # two behind
            B, C = front(0.8, -0.25), side(0.7, 1.5)
        elif kind == 3:    # three behind: nothing left
            A, B, C = [0.1 * ca, 0.1 * sa, -0.5], front(0.5, 0.25), side(0.4, -0.75)
        elif kind == 4:    # one vertex exactly on the near plane (z = -1 -> z_clip = -w), the others in front
            B, C = front(0.25, -1.0), side(0.5, -2.0)
        elif kind == 5:    # one vertex exactly at w = 0
            B, C = front(0.5, 0.0), side(0.5, -2.0)
        elif kind == 6:    # one behind and far to the side: the clipped polygon projects beyond 2^16 pixels
            B, C = front(0.6, -2.0), side(3.0e4, 0.5)
        elif kind == 7:    # two behind, one of them very far: beyond 2^23 (the set-up record cannot hold it)
            B, C = front(2.0e6, 0.75), side(5.0e3, 0.25)
        else:              # a vertex on the plane AND one behind it
            B, C = front(0.25, -1.0), side(40.0, 2.0)
        tris.append(_front_facing([A, B, C], vp, w, h, want_front=(i % 18) != 17))
    minimum = dict(behind1=20, behind2=14, behind3=6, on_near=14, w_zero=6, w_neg=30, clipped_sub_beyond16=20,
                   clipped_sub_below16=20, beyond23=6, front=50, covered_pixels=w * h // 4)
    return _finish("near_plane_fan", tris, vp, w, h, ALIGNED_SCALE, minimum)


def pixel_grid(w=64, h=32):
    """Vertices on pixel centres; horizontal, vertical and diagonal edges through pixel centres; both windings."""
    vp = ortho_pixels(w, h)
    tris = []
    cw_, ch_ = 4, 2                                   # cell: 4 x 2 pixels, its diagonals pass through centres
    nx, ny = (w - 8) // cw_, (h - 4) // ch_
    for j in range(ny):
        for i in range(nx):
            x0, y0 = 2.5 + i * cw_, 1.5 + j * ch_
            x1, y1 = x0 + cw_, y0 + ch_
            z = -0.5
            a, b, c, d = [x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]
            if (i + j) % 2 == 0:
                tris += [[a, b, c], [a, c, d]]        # diagonal a-c
            else:
                tris += [[a, b, d], [b, c, d]]        # diagonal b-d
            if (i * 7 + j * 3) % 5 == 0:              # a back-facing copy in FRONT of the sheet: must be culled
                tris.append([[x0, y0, -0.25], [x0, y1, -0.25], [x1, y1, -0.25]])
    # 45-degree edges and vertices on centres, drawn nearer than the sheet, with shared edges in both directions
    for k in range(4):
        x, y = 8.5 + 12 * k, 8.5
        tris += [[[x, y, -0.3], [x + 8, y, -0.3], [x + 8, y + 8, -0.3]],
                 [[x, y, -0.3], [x + 8, y + 8, -0.3], [x, y + 8, -0.3]]]
    minimum = dict(pixels_on_edge=300, pixels_on_vertex=100, edge_left=40, edge_top=40, edge_right=40, edge_bottom=40,
                   edge_diagonal=60, back=10, inexact_vertices_max=0, covered_pixels=1000)
    return _finish("pixel_grid", tris, vp, w, h, ALIGNED_SCALE, minimum, aligned=True)


def depth_ties(w=32, h=32):
    """Coplanar duplicates (same depth at every pixel: the lower index must win, in either submission order) and
    interpenetrating triangles whose depths cross exactly on a column of pixel centres."""
    vp = ortho_pixels(w, h)
    tris = []
    quad = lambda x0, y0, x1, y1, za, zb: [[[x0, y0, za], [x1, y0, zb], [x1, y1, zb]],
                                           [[x0, y0, za], [x1, y1, zb], [x0, y1, za]]]
    for rep in range(3):                                       # the same two triangles three times
        tris += quad(2, 2, 14, 14, -0.5, -0.5)
    tris += quad(3.5, 3.5, 9.5, 9.5, -0.5, -0.5)                # a smaller coplanar patch, later in the order
    # two sheets crossing at x = 24.5 (a column of centres): depth(x) = 0.5 +- (x - 24.5) / 32
    tris += quad(16.5, 2, 30.5, 14, -0.25, -0.6875)
    tris += quad(16.5, 2, 30.5, 14, -0.6875, -0.25)
    # the same pair submitted in the other order, lower half
    tris += quad(16.5, 18, 30.5, 30, -0.6875, -0.25)
    tris += quad(16.5, 18, 30.5, 30, -0.25, -0.6875)
    # duplicates with reversed vertex order inside the triangle (same plane, rotated vertex list)
    t = quad(2, 18, 14, 30, -0.75, -0.75)
    tris += t + [[t[0][1], t[0][2], t[0][0]], [t[1][2], t[1][0], t[1][1]]]
    minimum = dict(multi_covered_pixels=500, max_overdraw=3, inexact_vertices_max=0, front=20)
    return _finish("depth_ties", tris, vp, w, h, ALIGNED_SCALE, minimum, aligned=True)


def depth_planes(w=32, h=16):
    """Triangles at depth exactly 0 (on the near plane), exactly 1 (never visible under LESS against a cleared
    buffer), crossing the far plane (per-pixel far clip) and just inside it."""
    vp = ortho_pixels(w, h)
    t = lambda x0, z0, z1, z2: [[x0, 2, z0], [x0 + 6, 2, z1], [x0, 14, z2]]
    tris = [t(1, 0.0, 0.0, 0.0),                        # depth 0 everywhere: all three vertices on z = -w
            t(9, -1.0, -1.0, -1.0),                     # depth 1 everywhere: covers pixels nothing else covers
            t(17, -0.5, -1.5, -0.5),                    # crosses the far plane
            t(25, -1.0 + 2.0 ** -20, -1.0 + 2.0 ** -20, -1.0 + 2.0 ** -20),     # the last depths below 1
            [[1, 2, 0.25], [7, 2, -0.25], [1, 14, -0.25]]]                  # crosses the near plane in an ortho view
    minimum = dict(depth0_vertices=3, depth1_vertices=3, on_near=3, inexact_vertices_max=0, behind1=1)
    return _finish("depth_planes", tris, vp, w, h, ALIGNED_SCALE, minimum, aligned=True)


def slivers(w=128, h=64, seed=5, aligned=True):
    """Triangles thinner than a pixel, and zero-area ones: a point, collinear, and collinear only after the
    1/256-pixel snap."""
    vp = ortho_pixels(w, h)
    rng = np.random.default_rng(seed)
    g = lambda v: np.round(np.asarray(v) * 256.0) / 256.0       # onto the snap grid
    tris = []
    for i in range(120):
        a = g(rng.random(2) * [w, h])
        ang = rng.random() * 2 * np.pi
        ln = 5.0 + rng.random() * 0.6 * w
        b = g(a + ln * np.array([np.cos(ang), np.sin(ang)]))
        wid = 2.0 ** -rng.integers(1, 8)                         # 1/2 ... 1/128 pixel wide
        c = g(0.5 * (a + b) + wid * np.array([-np.sin(ang), np.cos(ang)]))
        z = -0.1 - 0.8 * rng.random()
        tris.append([[*a, z], [*b, z], [*c, z]])     # flat in depth: the snap cannot tilt it
    for i in range(8):                                          # points
        p = g(rng.random(2) * [w, h])
        tris.append([[*p, -0.05]] * 3)
    for i in range(8):                                          # exactly collinear
        p = g(rng.random(2) * [w / 2, h / 2])
        d = g(rng.random(2) * 8 + 1)
        tris.append([[*p, -0.05], [*(p + d), -0.05], [*(p + 3 * d), -0.05]])
    for i in range(8):                                          # collinear only after the snap: off the grid by 2^-11
        x, y = 4.0 + 12 * i, 10.0 + 5 * i
        tris.append([[x, y, -0.05], [x + 10, y, -0.05], [x + 5, y + 2.0 ** -11, -0.05]])
    tris.append([[0, 0, -0.95], [w, 0, -0.95], [0, h, -0.95]])  # something behind them
    minimum = dict(thin=60, zero_area=24, zero_after_snap=8, covered_pixels=w * h // 3)
    if aligned:
        minimum["inexact_vertices_max"] = 8                     # only the eight off-grid apexes
    tris = [_front_facing(t, vp, w, h) for t in tris]
    return _finish("slivers" if aligned else f"slivers_{w}x{h}", tris, vp, w, h, ALIGNED_SCALE, minimum, aligned=aligned)


def full_frame_and_small(w=200, h=120, seed=3):
    """One triangle that covers every bin of the frame plus many small ones in front of and behind it, a quarter
    of them alpha-tested cards."""
    vp = ortho_pixels(w, h)
    rng = np.random.default_rng(seed)
    tris = [[[-w, -h, -0.5], [3 * w, -h, -0.5], [-w, 3 * h, -0.5]]]
    alpha = [False]
    for i in range(320):
        c = rng.random(2) * [w, h]
        r = 1.0 + rng.random() * 9.0
        ang = rng.random(3) * 2 * np.pi / 3 + np.array([0, 2, 4]) * np.pi / 3
        z = -0.5 + (0.05 + rng.random() * 0.4) * (1 if i % 3 else -1)
        tri = [[c[0] + r * np.cos(a), c[1] + r * np.sin(a), z + 0.02 * k] for k, a in enumerate(ang)]
        tris.append(_front_facing(tri, vp, w, h, want_front=(i % 11) != 10))
        alpha.append(i % 4 == 0)
    minimum = dict(covered_pixels=w * h, multi_covered_pixels=w * h // 5, front=280, back=15)
    return _finish("full_frame_and_small", tris, vp, w, h, ALIGNED_SCALE, minimum, alpha=alpha)


def alpha_cards(w=96, h=64, seed=9):
    """Overlapping alpha-tested quads at different depths and texture scales over an opaque backdrop."""
    vp = ortho_pixels(w, h)
    rng = np.random.default_rng(seed)
    tris = [[[0, 0, -0.9], [w, 0, -0.9], [w, h, -0.9]], [[0, 0, -0.9], [w, h, -0.9], [0, h, -0.9]]]
    alpha = [False, False]
    for i in range(40):
        x0, y0 = rng.random(2) * [w - 20, h - 20]
        sx, sy = 6 + rng.random(2) * 30
        z = -0.1 - 0.7 * rng.random()
        tris += [[[x0, y0, z], [x0 + sx, y0, z], [x0 + sx, y0 + sy, z - 0.05]],
                 [[x0, y0, z], [x0 + sx, y0 + sy, z - 0.05], [x0, y0 + sy, z - 0.05]]]
        alpha += [True, True]
    minimum = dict(covered_pixels=w * h, max_overdraw=4, front=80)
    return _finish("alpha_cards", tris, vp, w, h, ALIGNED_SCALE, minimum, alpha=alpha)


def single_triangle(w=17, h=9):
    vp = ortho_pixels(w, h)
    tri = [[[-0.25, -0.5, -0.25], [w + 0.5, 0.25, -0.5], [w * 0.4, h + 0.75, -0.75]]]
    return _finish(f"single_triangle_{w}x{h}", tri, vp, w, h, ALIGNED_SCALE, dict(triangles=1, front=1,
                                                                               covered_pixels=max(1, w * h // 4)))


def single_pixel():
    """A 1 x 1 frame: one triangle over the only pixel centre, one that misses it, one with an edge through it."""
    vp = ortho_pixels(1, 1)
    tris = [[[0.0, 0.0, -0.5], [1.0, 0.0, -0.5], [0.0, 1.0, -0.5]],           # hypotenuse through (0.5, 0.5): not owned
            [[0.75, 0.75, -0.25], [1.0, 0.75, -0.25], [0.75, 1.0, -0.25]],    # misses the centre
            [[1.0, 1.0, -0.75], [0.0, 1.0, -0.75], [1.0, 0.0, -0.75]]]        # the other half: owns the shared edge
    return _finish("single_pixel", tris, vp, 1, 1, ALIGNED_SCALE,
                   dict(pixels_on_edge=1, covered_pixels=1, inexact_vertices_max=0), aligned=True)


def all_cases():
    return [near_plane_fan(), pixel_grid(), depth_ties(), depth_planes(), slivers(), slivers(200, 120, 6, False),
            full_frame_and_small(), alpha_cards(), single_triangle(), single_triangle(1, 1), single_pixel()]


CASE_NAMES = ["near_plane_fan", "pixel_grid", "depth_ties", "depth_planes", "slivers", "slivers_200x120",
              "full_frame_and_small", "alpha_cards", "single_triangle_17x9", "single_triangle_1x1", "single_pixel"]
_BUILT = {}


def get_case(name):
    if not _BUILT:
        for c in all_cases():
            _BUILT[c.name] = c
        assert list(_BUILT) == CASE_NAMES
    return _BUILT[name]


# ---------------------------------------------------------------------------------------------------------------
# watertightness: one planar rectangle as 2 triangles and as a few hundred
def rectangle_meshes(w=96, h=64, nx=14, ny=10, seed=21):
    """(coarse Case, fine Case): the rectangle [5.25, w - 7.5] x [3.75, h - 4.25] at one depth, as 2 triangles and as
    2 * nx * ny with shared vertices on the 1/256 grid (boundary vertices slide along the boundary, interior ones are
    jittered by up to a quarter cell, so every cell stays convex)."""
    vp = ortho_pixels(w, h)
    rng = np.random.default_rng(seed)
    g = lambda v: np.round(np.asarray(v) * 256.0) / 256.0
    x0, x1, y0, y1, z = 5.25, w - 7.5, 3.75, h - 4.25, -0.5
    coarse = [[[x0, y0, z], [x1, y0, z], [x1, y1, z]], [[x0, y0, z], [x1, y1, z], [x0, y1, z]]]
    dx, dy = (x1 - x0) / nx, (y1 - y0) / ny
    P = np.zeros((ny + 1, nx + 1, 2))
    for j in range(ny + 1):
        for i in range(nx + 1):
            jx = (rng.random() - 0.5) * 0.5 * dx if 0 < i < nx else 0.0
            jy = (rng.random() - 0.5) * 0.5 * dy if 0 < j < ny else 0.0
            P[j, i] = g([x0 + i * dx + jx, y0 + j * dy + jy])
    P[:, 0, 0], P[:, nx, 0], P[0, :, 1], P[ny, :, 1] = x0, x1, y0, y1
    fine = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = P[j, i], P[j, i + 1], P[j + 1, i + 1], P[j + 1, i]
            q = [[*a, z], [*b, z], [*c, z], [*d, z]]
            fine += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]] if rng.random() < 0.5 else [[q[0], q[1], q[3]], [q[1], q[2], q[3]]]
    mk = lambda name, t, m: _finish(name, t, vp, w, h, ALIGNED_SCALE, m)
    return mk("rectangle_2", coarse, dict(front=2)), mk("rectangle_fine", fine, dict(front=2 * nx * ny))


def reversed_case(case):
    """The same triangles submitted in the opposite order (ids follow the new order)."""
    return case.subset(np.arange(case.ntri)[::-1], case.name + "_reversed")


def check_watertight(render):
    """render(case) -> planes [23, w*h].  The fine mesh covers exactly the pixels the 2-triangle mesh covers, and every
    covered pixel has exactly one owner: with all triangles at one depth the first submitted wins a pixel two of them
    claim, so a doubled pixel shows a different triangle when the order is reversed."""
    coarse, fine = rectangle_meshes()
    check_minimum(coarse), check_minimum(fine)
    w, h = fine.w, fine.h
    a = owner_of(render(coarse), w, h)
    b = owner_of(render(fine), w, h)
    c = owner_of(render(reversed_case(fine)), w, h)
    assert (a >= 0).sum() > w * h // 2
    assert np.array_equal(a >= 0, b >= 0), np.argwhere((a >= 0) != (b >= 0))[:8]
    back = np.where(c >= 0, fine.ntri - 1 - c, -1)
    assert np.array_equal(b, back), np.argwhere(b != back)[:8]
    assert np.unique(b[b >= 0]).size > fine.ntri * 0.9        # nearly every small triangle owns some pixel
