"""The scenes of the dynamic-draw tests (include/vct.h "dynamic mesh", drawing), NumPy only: a small static room, a moving
object built to hit the decision points of the dynamic pass, the ONE static mesh the definition names -- the static
triangles followed by the dynamic ones with their defined frames and material -- and the library's bounding-box rule for
the work classes of the direct form.  tests/test_dynamic_draw_cases.py holds the premises on the CPU checker's output.

Units are eye space: the camera sits at the origin and looks down -z (geomcases.perspective_origin, near 1, far 40),
model_scale is 1/16.  The light is orthographic, above and in front of the room.

Static room (9 triangles, one material each, reds 0.05 .. 0.45):
    floor  y = -3        back wall  z = -25        occluder  z = -8, x in [-6, -1], in front of the object's left part
    TIE    a triangle at z = -12 that the object duplicates vertex for vertex
    LOW    a floor patch at y = -2.9 under the object
Object at A (OBJECT_TRIS triangles, palette of 3 colours with reds >= 0.6 and fourth values 0.3, 1.0, 0.0):
    BIG    a quad at z = -10: > 4096 pixels per triangle at 203 x 117, partly behind the occluder, hides the back wall
    WAVE, GROUP, SMALL   one triangle each of <= 4096, <= 256, <= 16 pixels
    DUP    the duplicate of TIE (exact depth ties on every pixel of it; the static triangle must own them)
    SAIL   a large triangle at y = 8 facing the light: > 4096 texels of the 128^2 shadow map (the camera sees its back)
    NEAR   one vertex behind the near plane: a quad, two fan sub-triangles
    BODY   a cloud of small triangles of either winding
B is A moved by MOVE.

The textured room (tests/test_gpu_dynamic_features.py): the same triangles with texture coordinates (room_uv), four small maps
(room_textures: wall, an alpha-tested lace, a height map, floor) and their assignment (room_mat_tex) -- the lace on the
occluder and on TIE opens holes through which the object shows, and hands the tied pixels TIE discards to DUP.  object_lights:
eight local lights around the object (tests/test_gpu_dynamic_readers.py)."""
import numpy as np

import gbuffer_import_ref as gi
import geomcases as gc

f32 = np.float32
MS = 0.0625
FRAMES = ((203, 117), (17, 9))
W, H = FRAMES[0]
SHADOW = 128
NEAR, FAR = 1.0, 40.0
SPECULAR = (0.3, 0.6, 0.2)
MOVE = (2.5, 0.75, -1.0)
PALETTE = np.array([[0.9, 0.15, 0.1, 0.3], [0.6, 0.9, 0.1, 1.0], [0.75, 0.1, 0.9, 0.0]], f32)
SMALL, GROUP, WAVE = 16, 256, 4096          # VCT_RASTER_SMALL / _GROUP / _WAVE (csrc/vct_raster.hip)
VERTEX_LIMIT_GRIDS = 1048576.0              # VCT_VERTEX_LIMIT_GRIDS (include/vct.h)
G = 150.0


def camera(w, h):
    return gc.perspective_origin(w, h, cot=2.0, near=NEAR, far=FAR)


def light_vp():
    """Column-major float32[16]: orthographic, eye (0, 30, 8) looking at (0, -3, -12), 32 x 32 units, depth 5 .. 70."""
    eye, at = np.array([0.0, 30.0, 8.0]), np.array([0.0, -3.0, -12.0])
    fwd = (at - eye) / np.linalg.norm(at - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0]); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = right, up, -fwd
    view[:3, 3] = -view[:3, :3] @ eye
    half, n, f = 16.0, 5.0, 70.0
    proj = np.diag([1.0 / half, 1.0 / half, -2.0 / (f - n), 1.0])
    proj[2, 3] = -(f + n) / (f - n)
    return np.ascontiguousarray((proj @ view).T, f32).reshape(16)


def _quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


TIE_TRI = [[2.0, -1.0, -12.0], [5.0, -1.0, -12.0], [3.5, 2.0, -12.0]]


def static_mesh():
    """(pos [n, 9] f32 model space, material, albedo [n, 4], specular [n, 3], frames)"""
    tris = []
    tris += _quad([-12, -3, -2], [12, -3, -2], [12, -3, -30], [-12, -3, -30])          # floor, normal +y
    tris += _quad([-12, -3, -25], [12, -3, -25], [12, 9, -25], [-12, 9, -25])          # back wall, normal +z
    tris += _quad([-6, -3, -8], [-1, -3, -8], [-1, 1, -8], [-6, 1, -8])                # occluder
    tris += [TIE_TRI]
    tris += _quad([-4, -2.9, -9], [3, -2.9, -9], [3, -2.9, -11], [-4, -2.9, -11])      # low patch
    pos = (np.asarray(tris, np.float64).reshape(-1, 9) / MS).astype(f32)
    n = pos.shape[0]
    alb = np.zeros((n, 4), f32)
    alb[:, 0] = 0.05 * (np.arange(n) + 1)
    alb[:, 1], alb[:, 2], alb[:, 3] = 0.5, 0.25, 1.0
    spec = np.tile(np.array([0.25, 0.5, 0.125], f32), (n, 1))
    spec[::3, 1:] = 0.0
    return pos, np.arange(n, dtype=np.int32), alb, spec, static_frames(pos)


def static_frames(pos):
    """Per-vertex (normal, tangent, bitangent) [n, 9] of a static mesh: geomcases.Case.frames' geometric frame."""
    c = gc.Case("frames", pos, np.eye(4, dtype=f32).reshape(16), 8, 8, MS, {})
    return c.frames()


# the object: names -> triangle indices, filled by object_mesh
PARTS = {}


def object_tris():
    """[n, 3, 3] float64 eye-space triangles of the object at A."""
    rng = np.random.default_rng(41)
    vp = camera(W, H)
    tris, parts = [], {}

    def add(name, ts):
        parts[name] = list(range(len(tris), len(tris) + len(ts)))
        tris.extend(ts)
    add("BIG", _quad([-4, -2, -10], [3, -2, -10], [3, 3.2, -10], [-4, 3.2, -10]))
    add("WAVE", [[[3.5, 2.5, -10], [6.5, 2.5, -10], [5.0, 5.0, -10]]])
    add("GROUP", [[[4.0, -2.5, -9], [4.9, -2.5, -9], [4.4, -1.7, -9]]])
    add("SMALL", [[[6.02, 0.02, -9], [6.16, 0.02, -9], [6.08, 0.14, -9]]])
    add("DUP", [TIE_TRI])
    add("SAIL", [[[-11.0, 8.0, -2.0], [11.0, 8.0, -2.0], [0.0, 8.0, -24.0]]])
    near = [[-4.5, -2.5, -6.0], [-2.5, -2.5, -6.0], [-3.5, -2.0, -0.5]]
    add("NEAR", [gc._front_facing(near, vp, W, H)])
    c = rng.uniform([-3.5, -1.5, -9.8], [6.0, 4.0, -9.0], (40, 1, 3))
    add("BODY", list(c + rng.normal(scale=0.35, size=(40, 3, 3))))
    PARTS.clear(); PARTS.update(parts)
    return np.asarray(tris, np.float64)


def object_mesh(where="A"):
    """(pos [n, 9] f32 model space, material, table [3, 4]) of the object at A or B."""
    t = object_tris()
    if where == "B":
        keep = PARTS["DUP"] + PARTS["NEAR"]          # the tie and the near-clipped triangle stay where they are
        moved = t + np.asarray(MOVE)[None, None, :]
        moved[keep] = t[keep]
        t = moved
    pos = (t.reshape(-1, 9) / MS).astype(f32)
    pos[PARTS["DUP"][0]] = static_mesh()[0][6]       # the very fp32 values of the static TIE triangle
    mat = (np.arange(pos.shape[0]) % 3).astype(np.int32)
    return pos, mat, PALETTE.copy()


def dynamic_frames(pos):
    """The defined frame of dynamic triangles, [n, 9] each: n = cross(p1 - p0, p2 - p0) on the model-space fp32 positions,
    every component a * b - c * d rounded per operation, then the G-buffer import's construction (u, t, b)."""
    p = np.ascontiguousarray(pos, f32).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(f32)
        u, t, bt = gi.frame(n)
    rep = lambda v: np.ascontiguousarray(np.repeat(v[:, None, :], 3, 1).reshape(-1, 9), f32)
    return rep(u), rep(t), rep(bt)


def in_contract(pos, ms=MS, grid=G):
    """The vertex contract per triangle: every coordinate v with fabsf(v * model_scale) <= limit, product in fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.abs(np.ascontiguousarray(pos, f32).reshape(-1, 9) * f32(ms))
        return (v <= f32(VERTEX_LIMIT_GRIDS) * f32(grid)).all(1)


def first_beyond(ms=MS, grid=G):
    """The smallest positive fp32 v whose product v * model_scale (fp32) exceeds the contract's bound."""
    lim = f32(VERTEX_LIMIT_GRIDS) * f32(grid)
    v = f32(lim / f32(ms))
    while f32(v * f32(ms)) <= lim:
        v = np.nextafter(v, f32(np.inf))
    while f32(np.nextafter(v, f32(0)) * f32(ms)) > lim:
        v = np.nextafter(v, f32(0))
    return v


def concatenated(static, dyn, specular=SPECULAR, ms=MS, grid=G):
    """The one static mesh of the definition: (pos, material, albedo, specular, frames).  Dynamic materials follow the
    static table with alpha 1 and the specular constant; a dynamic triangle outside the vertex contract is left out as
    the point (0, 0, 0) -- zero area, drawn by no rasteriser."""
    spos, smat, salb, sspec, sfr = static
    dpos, dmat, dalb = dyn
    dpos = np.ascontiguousarray(dpos, f32).reshape(-1, 9).copy()
    dpos[~in_contract(dpos, ms, grid)] = 0.0
    dfr = dynamic_frames(dpos)
    alb = np.concatenate([salb, np.concatenate([dalb[:, :3], np.ones((dalb.shape[0], 1), f32)], 1)]).astype(f32)
    sp = np.zeros(3, f32) if specular is None else np.asarray(specular, f32)
    spec = np.concatenate([sspec, np.tile(sp, (dalb.shape[0], 1))]).astype(f32)
    pos = np.concatenate([spos, dpos])
    mat = np.concatenate([smat, dmat + salb.shape[0]]).astype(np.int32)
    frames = tuple(np.concatenate([a, b]) for a, b in zip(sfr, dfr))
    return pos, mat, alb, spec, frames


def mesh_of(oracle, m, ms=MS, tex=None, mipmaps=False):
    """tex: (uv [ntri, 6], mat_tex [nmat, 3], textures) of the whole mesh m (textured_cat), or None."""
    pos, mat, alb, spec, frames = m
    if tex is None:
        return oracle.make_mesh(pos, mat, alb, spec, frames, model_scale=ms)
    uv, mat_tex, textures = tex
    assert uv.shape[0] == pos.shape[0] and mat_tex.shape[0] == alb.shape[0]
    return oracle.make_mesh(pos, mat, alb, spec, frames, uv=uv, mat_tex=mat_tex, textures=textures, model_scale=ms,
                            mipmaps=mipmaps)


def reference(oracle, m, w, h, vp=None, lvp=None, S=SHADOW, ms=MS, with_shadow=True, tex=None, mipmaps=False):
    """(depth [S, S], planes [23, h * w]) of mesh tuple m on the CPU checker, the planes under that depth."""
    mesh = mesh_of(oracle, m, ms, tex, mipmaps)
    vp = camera(w, h) if vp is None else vp
    lvp = light_vp() if lvp is None else lvp
    depth = oracle.render_shadow_map(mesh, lvp, S)
    return depth, oracle.render_gbuffer(mesh, vp, w, h, depth if with_shadow else None, lvp)


# ---- the textured room --------------------------------------------------------------------------------------------------------
WALL_TEX, LACE_TEX, BUMP_TEX, FLOOR_TEX = 0, 1, 2, 3
FLOOR_UV, WALL_UV, OCCLUDER_UV, TIE_UV = 12.0, 5.0, 1.5, 1.0


def room_textures():
    """Four power-of-two maps, uint8 [h, w, 4]: 16 x 8 (wall diffuse, TIE specular), the 8 x 8 lace (alpha 0 where
    (i + j) % 3 == 0, else 255), a 4 x 4 height map, 16 x 16 (floor diffuse, wall specular).  Every red value is below 128,
    so that owner_is_dynamic still tells the owner of a textured pixel."""
    rng = np.random.default_rng(3)

    def tex(h, w):
        t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        t[..., 0] >>= 1
        t[..., 3] = 255
        return t
    wall, lace, bump, floor = tex(8, 16), tex(8, 8), tex(4, 4), tex(16, 16)
    lace[..., 3] = np.where((np.add.outer(np.arange(8), np.arange(8)) % 3) == 0, 0, 255)
    return [wall, lace, bump, floor]


def room_uv():
    """uv [9, 6] f32 of static_mesh's triangles: each quad (a, b, c, d) maps to (0, 0), (s, 0), (s, s), (0, s) with its UV
    scale s, TIE to (0, 0), (1, 0), (0.5, 1); the LOW patch has none."""
    def quad(s):
        return [[0, 0, s, 0, s, s], [0, 0, s, s, 0, s]]
    uv = quad(FLOOR_UV) + quad(WALL_UV) + quad(OCCLUDER_UV) + [[0, 0, TIE_UV, 0, 0.5 * TIE_UV, TIE_UV]] + quad(0.0)
    return np.asarray(uv, f32)


def room_mat_tex():
    """mat_tex [9, 3] int32 (diffuse, specular, height) of static_mesh's materials, one per triangle."""
    floor, wall = [FLOOR_TEX, -1, BUMP_TEX], [WALL_TEX, FLOOR_TEX, -1]
    occ, tie, low = [LACE_TEX, -1, -1], [LACE_TEX, WALL_TEX, -1], [-1, -1, -1]
    return np.asarray([floor, floor, wall, wall, occ, occ, tie, low, low], np.int32)


def textured_cat(ndyn_tris=0, ndyn_mats=0):
    """The `tex` argument of mesh_of / reference for the room followed by ndyn_tris dynamic triangles of ndyn_mats
    materials: dynamic triangles get UV 0 and mat_tex -1 (the definition gives the dynamic mesh no textures)."""
    uv = np.concatenate([room_uv(), np.zeros((ndyn_tris, 6), f32)])
    mt = np.concatenate([room_mat_tex(), np.full((ndyn_mats, 3), -1, np.int32)])
    return uv, mt, room_textures()


def object_lights(n=8):
    """lights_ref.many_lights(n) brought around the object: positions scaled to within +- 8 units of (1, 1, -6), between the
    camera and the object; radii and colours as they are."""
    import lights_ref
    out = []
    for light in lights_ref.many_lights(n):
        moved = dict(light)
        moved["position"] = tuple(float(c + 0.12 * p) for c, p in zip((1.0, 1.0, -6.0), light["position"]))
        out.append(moved)
    return out


def boxes(pos, vp, w, h, ms=MS, rows=None):
    """The library's box rule (csrc/vct_raster.hip setup_subtri, k_raster_vis): per triangle the list of bounding-box
    pixel counts (x1 - x0 + 1) * (y1 - y0 + 1) of its front-facing fan sub-triangles, the box clipped to the frame (and
    the scissor rows); in float64 from the fp32-scaled vertices, so sizes are chosen away from the class bounds."""
    y_lo, y_hi = (0, h) if rows is None else rows
    _, polys = gc.clip_polygons(pos, ms, vp)
    out = []
    for poly in polys:
        sizes = []
        for sub in gc.window_subtris(poly, w, h):
            if sub is None:
                continue
            s = gc._snap(sub[0])
            if not gc._area(s) > 0.0:
                continue
            x0, x1 = max(0, int(np.floor(s[:, 0].min()))), min(w - 1, int(np.floor(s[:, 0].max())))
            y0, y1 = max(y_lo, int(np.floor(s[:, 1].min()))), min(y_hi - 1, int(np.floor(s[:, 1].max())))
            if x1 >= x0 and y1 >= y0:
                sizes.append((x1 - x0 + 1) * (y1 - y0 + 1))
        out.append(sizes)
    return out


def work_class(box):
    return 0 if box <= SMALL else 1 if box <= GROUP else 2 if box <= WAVE else 3


def owner_is_dynamic(planes):
    """Per pixel: covered and showing a palette colour (the palette's reds are >= 0.6, the static table's < 0.5)."""
    p = np.asarray(planes).reshape(23, -1)
    return (p[18] >= 0.5) & (p[15] >= 0.55)


def offenders(n=4):
    """n single triangles outside the vertex contract: a NaN, +inf, -inf and the first fp32 beyond the bound, each in one
    coordinate of an otherwise ordinary triangle in front of the camera."""
    base = np.array([[-2.0, 0.0, -6.0], [2.0, 0.0, -6.0], [0.0, 3.0, -6.0]], np.float64) / MS
    bad = [f32(np.nan), f32(np.inf), f32(-np.inf), first_beyond()]
    out = []
    for k, v in enumerate(bad[:n]):
        t = base.astype(f32).copy()
        t[k % 3, (k + 1) % 3] = v
        out.append(t.reshape(9))
    return np.asarray(out, f32)
