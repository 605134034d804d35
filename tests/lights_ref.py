"""numpy restatement of the local lights of include/vct.h ("local lights"): the folding, the term of one light at a point,
the level-0 update behind vct_inject_light and the lit planes of a frame.  Test infrastructure, NumPy only.

fp32 throughout, every operation a single rounded numpy op on float32 operands in the header's order; np.fmax / np.fmin
are C's fmaxf / fminf (a NaN operand gives the other one).  The voxel side starts from what the CPU oracle gives
(oracle.voxelize_conservative_attr: level 0 and the voxel attributes, [z, y, x, 4] uint8) and its result goes through
oracle.build_mips.  The one operation that is not correctly rounded on both sides is powf: callers that want bits keep
the specular planes 0."""
import numpy as np

f32 = np.float32
LIGHTS_MAX = 64
SPOT = 1
SHOW_DIFFUSE, SHOW_SPECULAR = 1, 4


def point(position, color, radius, source_radius):
    return dict(position=tuple(position), color=tuple(color), radius=radius, source_radius=source_radius)


def spot(position, color, radius, source_radius, direction, cos_inner, cos_outer):
    return dict(position=tuple(position), color=tuple(color), radius=radius, source_radius=source_radius,
                direction=tuple(direction), cos_inner=cos_inner, cos_outer=cos_outer, flags=SPOT)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def unorm8_to_float(b):
    """the library's unorm8 decode: (float)c / 255.0f exactly"""
    return np.asarray(b).astype(f32) / f32(255.0)


def float_to_unorm8(x):
    """vct_float_to_unorm8: s = f * 255 + 0.5; not (s > 0) -> 0; s >= 255 -> 255; else truncation"""
    with np.errstate(all="ignore"):
        s = np.asarray(x, f32) * f32(255.0) + f32(0.5)
        out = np.where(s >= f32(255.0), f32(255.0), np.where(s > f32(0.0), s, f32(0.0)))
        return out.astype(np.int32).astype(np.uint8)


def fold(light):
    """One light (a dict of vct_light's fields) as the device sees it."""
    pos = [f32(v) for v in light["position"]]
    col = [f32(v) for v in light["color"]]
    radius, src = f32(light["radius"]), f32(light["source_radius"])
    out = dict(pos=pos, color=col, R2=radius * radius, S2=src * src, spot=bool(int(light.get("flags", 0)) & SPOT))
    if out["spot"]:
        v = [f32(c) for c in light["direction"]]
        ln = np.sqrt(_dot(v, v))                       # the import's unit(v)
        r = f32(1.0) / ln
        out["axis"] = [c * r for c in v] if ln > 0 else [f32(0.0)] * 3
        out["cos_outer"] = f32(light["cos_outer"])
        out["inv_cone"] = f32(1.0) / (f32(light["cos_inner"]) - f32(light["cos_outer"]))
    return out


def term(L, P):
    """`in`, l, att * spot and the spot's t (1 for a point light) of folded light L at the points P = [x, y, z] arrays."""
    with np.errstate(all="ignore"):
        d = [L["pos"][c] - P[c] for c in range(3)]
        r2 = _dot(d, d)
        inside = r2 < L["R2"]
        ln = np.sqrt(r2)
        l = [d[c] / ln for c in range(3)]
        q = r2 / L["R2"]
        w = np.fmax(f32(1.0) - q * q, f32(0.0))
        att = (w * w) / np.fmax(r2, L["S2"])
        t = np.ones_like(r2)
        if L["spot"]:
            c = _dot(L["axis"], l) * f32(-1.0)
            t = np.fmin(np.fmax((c - L["cos_outer"]) * L["inv_cone"], f32(0.0)), f32(1.0))
        return inside, l, att * (t * t), t, r2


def diffuse_sum(lights, P, n):
    """Dsum [3] of arrays, and per light (in, nl, t) for the non-degeneracy counts."""
    zero = np.zeros_like(np.asarray(P[0], f32))
    D = [zero.copy(), zero.copy(), zero.copy()]
    info = []
    with np.errstate(all="ignore"):
        for light in lights:
            L = fold(light)
            inside, l, a_s, t, r2 = term(L, P)
            nl = np.fmax(_dot(n, l), f32(0.0))
            k = np.where(inside, a_s * nl, f32(0.0)).astype(f32)
            for c in range(3):
                D[c] = D[c] + L["color"][c] * k
            info.append(dict(inside=inside, nl=nl, t=t, r2=r2))
    return D, info


def voxel_centres(V, G):
    """centre of voxel i along an axis: (((float)i + 0.5f) / V - 0.5f) * G"""
    return ((np.arange(V).astype(f32) + f32(0.5)) / f32(V) - f32(0.5)) * f32(G)


def voxel_inputs(attr_albedo, attr_normal, G):
    """P, n (lists of [V, V, V] arrays indexed [z, y, x]) and the occupied mask."""
    V = attr_albedo.shape[0]
    c = voxel_centres(V, G)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    with np.errstate(all="ignore"):
        a = [attr_normal[..., k].astype(np.int32).astype(f32) - f32(128.0) for k in range(3)]
        ln = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        n = [a[k] / ln for k in range(3)]
    return [x, y, z], n, attr_albedo[..., 3] == 255


def level0(l0, attr_albedo, attr_normal, lights, G, want_info=False):
    """Level 0 after the lights: l0 (the resolve's output, emission add included), uint8 [V, V, V, 4]."""
    P, n, occ = voxel_inputs(attr_albedo, attr_normal, G)
    D, info = diffuse_sum(lights, P, n)
    out = l0.copy()
    with np.errstate(all="ignore"):
        for c in range(3):
            v = float_to_unorm8(unorm8_to_float(l0[..., c]) + unorm8_to_float(attr_albedo[..., c]) * D[c])
            out[..., c] = np.where(occ, v, l0[..., c])
    return (out, dict(occ=occ, D=D, lights=info)) if want_info else out


def brick_cull(lights, V, G):
    """The voxel kernel's cull restated: [V/8, V/8, V/8, nlights] (indexed [bz, by, bx]) True where light j survives for
    the brick -- r2_min over the box of the brick's voxel centres, in the kernel's operation order."""
    c = voxel_centres(V, G)
    lo, hi = c[0::8], c[7::8]
    out = np.zeros((V // 8, V // 8, V // 8, len(lights)), bool)

    def gap(p, lo, hi):
        a, b = p - hi, p - lo
        return np.where(a > 0, a, np.where(b < 0, b * f32(-1.0), f32(0.0))).astype(f32)
    for j, light in enumerate(lights):
        L = fold(light)
        gx, gy, gz = gap(L["pos"][0], lo, hi), gap(L["pos"][1], lo, hi), gap(L["pos"][2], lo, hi)
        r2 = (gx[None, None, :] * gx[None, None, :] + gy[None, :, None] * gy[None, :, None]) + gz[:, None, None] * gz[:, None, None]
        out[..., j] = r2 < L["R2"]
    return out


def per_brick(mask):
    """[V, V, V] bool -> [V/8, V/8, V/8] any() over each 8^3 brick"""
    V = mask.shape[0]
    return mask.reshape(V // 8, 8, V // 8, 8, V // 8, 8).any(axis=(1, 3, 5))


def class_shininess(gloss_plane, classes):
    """per-pixel Phong exponent under the gloss plane's clamp rule; classes: [(tan_specular, shininess), ...]"""
    b = np.asarray(gloss_plane).astype(np.int64)
    cls = np.where(b < len(classes), b, 0)
    return np.asarray([c[1] for c in classes], f32)[cls]


def lit_planes(planes, lights, cam, shininess, mask=31, E=None):
    """The lit planes [3, npix] of a launch over the whole frame: E + Lit for live pixels, +0 for discarded ones.
    shininess: a scalar or a per-pixel float32 array (class_shininess)."""
    g = np.asarray(planes, f32)
    npix = g.shape[1]
    P, N = [g[0], g[1], g[2]], [g[12], g[13], g[14]]
    live = ~(g[18] < f32(0.5))
    shin = np.broadcast_to(np.asarray(shininess, f32), (npix,))
    with np.errstate(all="ignore"):
        e = [f32(cam[c]) - P[c] for c in range(3)]
        ln = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        Ev = [e[c] / ln for c in range(3)]
        D = [np.zeros(npix, f32) for _ in range(3)]
        S = [np.zeros(npix, f32) for _ in range(3)]
        for light in lights:
            L = fold(light)
            inside, l, a_s, _, _ = term(L, P)
            ndl = _dot(N, l)
            kd = np.where(inside, a_s * np.fmax(ndl, f32(0.0)), f32(0.0)).astype(f32)
            two = f32(2.0) * ndl
            R = [two * N[c] - l[c] for c in range(3)]
            sp = np.power(np.fmax(_dot(Ev, R), f32(0.0)), shin).astype(f32)
            ks = np.where(inside, a_s * sp, f32(0.0)).astype(f32)
            for c in range(3):
                D[c] = D[c] + L["color"][c] * kd
                S[c] = S[c] + L["color"][c] * ks
        out = np.zeros((3, npix), f32)
        for c in range(3):
            dd = D[c] * g[15 + c] if mask & SHOW_DIFFUSE else np.zeros(npix, f32)
            ss = S[c] * g[19 + c] if mask & SHOW_SPECULAR else np.zeros(npix, f32)
            lit = dd + ss
            if E is not None:
                lit = np.asarray(E, f32).reshape(3, -1)[c] + lit
            out[c] = np.where(live, lit, f32(0.0))
    return out


# ---- the inputs of the tests ------------------------------------------------------------------------------------------
# Four lights inside the default grid (150 world units), two of them spots, for voxcases.random_scene(300, 7) at V = 32:
# tests/test_lights_restatement.py holds the counts that make the GPU comparisons non-degenerate.
LIGHTS = [
    point((-30.0, 20.0, 10.0), (900.0, 500.0, 300.0), 55.0, 2.0),
    spot((25.0, 40.0, -20.0), (1500.0, 1500.0, 900.0), 70.0, 1.5, (-0.2, -1.0, 0.3), 0.92, 0.6),
    point((5.0, 10.0, -5.0), (200.0, 400.0, 600.0), 72.0, 1.0),
    spot((-10.0, -50.0, -40.0), (300.0, 700.0, 1200.0), 60.0, 2.5, (0.3, 0.6, 0.7), 0.8, 0.3),
]


def many_lights(n=64, seed=3, G=150.0):
    """n small lights scattered over the grid behind one large light 0 (alternating point / spot)."""
    r = np.random.default_rng(seed)
    out = [point((5.0, -10.0, 15.0), (700.0, 600.0, 500.0), 55.0, 2.0)]
    for i in range(1, n):
        pos = r.uniform(-0.45 * G, 0.45 * G, 3)
        col = r.uniform(20.0, 300.0, 3)
        rad = float(r.uniform(8.0, 22.0))
        if i % 2:
            out.append(point(pos, col, rad, 1.0))
        else:
            out.append(spot(pos, col, rad, 1.0, r.normal(size=3), 0.9, 0.2))
    return out
