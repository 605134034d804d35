"""The G-buffer import of include/vct.h "G-buffer import" restated in numpy: every operation is an fp32 numpy operation
in the order the header writes it (numpy neither fuses nor reassociates), IEEE / and sqrt.  restate() turns a set of
inputs and descriptor fields into the 23 planes (and the pixel-emission and pixel-gloss planes with material ids);
the packers turn a set of 23 planes into each input format.  Test infrastructure: only tests/ and tools/ import this."""
import numpy as np

f32 = np.float32

POSITION_F32X3, POSITION_F32X4, DEPTH_F32 = 0, 1, 2
NORMAL_F32X3, NORMAL_F16X4, NORMAL_OCT = 0, 1, 2
COLOR_UNORM8X4, COLOR_F16X4, COLOR_F32X4 = 0, 1, 2
FLIP_Y, DEPTH_ZERO_TO_ONE, OPAQUE = 1, 2, 4
POSITION_BYTES, NORMAL_BYTES, COLOR_BYTES = (12, 16, 4), (12, 8, 4), (4, 8, 16)
NO_MAP_SHADOW = f32(25.0) * f32(0.111)


def canonical_bits(a):
    """uint32 view of fp32 values with every NaN mapped to one pattern.  Which NaN an invalid operation returns (sign,
    payload) and which operand's payload survives are not defined by IEEE 754: x86 SSE returns 0xffc00000 for inf - inf,
    gfx950 0x7fc00000.  Everything else -- the sign of zeros and infinities included -- is compared as it is."""
    a = np.ascontiguousarray(a, f32)
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7fc00000
    return bits


# ---- decode ----
def half(u16):
    return np.ascontiguousarray(u16).view(np.float16).astype(f32)      # exact


def unorm8(c):
    return c.astype(f32) / f32(255.0)


def snorm16(s):
    return np.maximum(s.astype(np.int32), -32767).astype(f32) / f32(32767.0)


def octahedral(ex, ey):
    one = f32(1.0)
    z = (one - np.abs(ex)) - np.abs(ey)
    fold = z < 0
    x = np.where(fold, (one - np.abs(ey)) * np.where(ex >= 0, one, -one), ex)
    y = np.where(fold, (one - np.abs(ex)) * np.where(ey >= 0, one, -one), ey)
    return np.stack([x, y, z], 1).astype(f32)


def read_normal(buf, fmt, npix):
    if fmt == NORMAL_F32X3:
        return np.ascontiguousarray(buf, f32).reshape(npix, 3)
    if fmt == NORMAL_F16X4:
        return half(np.ascontiguousarray(buf).view(np.uint16).reshape(npix, 4))[:, :3]
    e = snorm16(np.ascontiguousarray(buf).view(np.int16).reshape(npix, 2))
    return octahedral(e[:, 0], e[:, 1])


def read_color(buf, fmt, npix):
    if fmt == COLOR_UNORM8X4:
        return unorm8(np.ascontiguousarray(buf).view(np.uint8).reshape(npix, 4))
    if fmt == COLOR_F16X4:
        return half(np.ascontiguousarray(buf).view(np.uint16).reshape(npix, 4))
    return np.ascontiguousarray(buf, f32).reshape(npix, 4)


# ---- frame ----
def unit(v):
    v = np.ascontiguousarray(v, f32)
    l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    il = f32(1.0) / l
    return np.where((l > 0)[:, None], v * il[:, None], f32(0.0)).astype(f32)


def frame(n):
    """(u, t, b) of the geometric normals n [k, 3]"""
    u = unit(n)
    ax, ay, az = np.abs(u[:, 0]), np.abs(u[:, 1]), np.abs(u[:, 2])
    ymajor = (ay >= ax) & (ay >= az)
    zero = np.zeros_like(ax)
    k = np.where(ymajor[:, None], np.stack([zero, -u[:, 2], u[:, 1]], 1), np.stack([u[:, 2], zero, -u[:, 0]], 1)).astype(f32)
    t = unit(k)
    b = np.stack([u[:, 1] * t[:, 2] - u[:, 2] * t[:, 1], u[:, 2] * t[:, 0] - u[:, 0] * t[:, 2],
                  u[:, 0] * t[:, 1] - u[:, 1] * t[:, 0]], 1).astype(f32)
    return u, t, b


# ---- shadow ----
def light_space(P, light_vp):
    """d [k, 4] of the positions P [k, 3]: the shade kernel's transform, m column-major [16]"""
    m = np.asarray(light_vp, f32).reshape(16)
    with np.errstate(all="ignore"):
        return np.stack([((m[r] * P[:, 0] + m[4 + r] * P[:, 1]) + m[8 + r] * P[:, 2]) + m[12 + r] for r in range(4)], 1).astype(f32)


def pcf(d, depth):
    with np.errstate(all="ignore"):
        return _pcf(np.ascontiguousarray(d, f32), depth)


def _pcf(d, depth):
    """PCF count * 0.111f of trace.fs:132-163 for the light-space coordinates d [k, 4] over the fp32 depth map [S, S] (as a
    GL depth texture: clamped to [0, 1], bilinear, clamp to edge), tap by tap in the shade kernel's operation order."""
    S = depth.shape[0]
    tex = np.clip(np.nan_to_num(np.asarray(depth, f32), nan=0.0), 0.0, 1.0).astype(f32)
    half_, fS, top = f32(0.5), f32(S), f32(S - 1)
    cx, cy, cz = d[:, 0] * half_ + half_, d[:, 1] * half_ + half_, d[:, 2] * half_ + half_
    cur = cz / d[:, 3] - f32(0.002)
    step = f32(1.0) / fS

    def clamp(f):
        return np.where(f < 0, 0, np.where(f > top, S - 1, np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)))

    cnt = np.zeros(d.shape[0], f32)
    for kx in range(-2, 3):
        for ky in range(-2, 3):
            x = (cx + step * f32(kx)) * fS - half_
            y = (cy + step * f32(ky)) * fS - half_
            fx, fy = np.floor(x), np.floor(y)
            a, b = x - fx, y - fy
            i0, i1, j0, j1 = clamp(fx), clamp(fx + f32(1.0)), clamp(fy), clamp(fy + f32(1.0))
            one = f32(1.0)
            tap = (((one - a) * (one - b) * tex[j0, i0] + a * (one - b) * tex[j0, i1]) + (one - a) * b * tex[j1, i0]) + a * b * tex[j1, i1]
            cnt = cnt + np.where(cur <= tap, one, f32(0.0))
    return (cnt * f32(0.111)).astype(f32)


# ---- the import ----
def restate(w, h, position, normal, albedo, shading_normal=None, specular=None, shadow=None, material=None,
            position_format=POSITION_F32X3, normal_format=NORMAL_F32X3, albedo_format=COLOR_UNORM8X4,
            specular_format=COLOR_UNORM8X4, flags=0, inv_view_proj=None, depth_clear=1.0, normal_scale=1.0,
            specular_constant=(0.0, 0.0, 0.0), shadow_map=None, light_vp=None, emission=None, mat_class=None):
    """planes [23, h*w] fp32 (and, with `material`, (planes, emission planes [3, h*w] or None, gloss plane [h*w] uint8 or
    None)).  shadow_map [S, S] + light_vp (column-major [16]): the context's map, used where `shadow` is None.  emission
    [nmat, 3] / mat_class [nmat]: the attached tables."""
    npix = w * h
    with np.errstate(all="ignore"):
        ys, xs = np.divmod(np.arange(npix), w)
        src = (np.where(flags & FLIP_Y, h - 1 - ys, ys) * w + xs).astype(np.int64)       # element of every input per frame pixel
        surface = np.ones(npix, bool)
        if position_format == DEPTH_F32:
            depth = np.ascontiguousarray(position, f32).reshape(npix)[src]
            surface = ~((depth == f32(depth_clear)) | np.isnan(depth))
            nx = (f32(2.0) * (xs.astype(f32) + f32(0.5))) / f32(w) - f32(1.0)
            ny = (f32(2.0) * (ys.astype(f32) + f32(0.5))) / f32(h) - f32(1.0)
            nz = depth if flags & DEPTH_ZERO_TO_ONE else f32(2.0) * depth - f32(1.0)
            m = np.asarray(inv_view_proj, f32).reshape(16)
            r = [((m[i] * nx + m[4 + i] * ny) + m[8 + i] * nz) + m[12 + i] for i in range(4)]
            P = np.stack([r[0] / r[3], r[1] / r[3], r[2] / r[3]], 1).astype(f32)
        elif position_format == POSITION_F32X4:
            p4 = np.ascontiguousarray(position, f32).reshape(npix, 4)[src]
            surface = ~(p4[:, 3] == 0)
            P = p4[:, :3]
        else:
            P = np.ascontiguousarray(position, f32).reshape(npix, 3)[src]
        ns = f32(normal_scale)
        u, t, b = frame(read_normal(normal, normal_format, npix)[src])
        su = u if shading_normal is None else unit(read_normal(shading_normal, normal_format, npix)[src])
        alb = read_color(albedo, albedo_format, npix)[src]
        if specular is None:
            spec = np.broadcast_to(np.asarray(specular_constant, f32), (npix, 3))
        else:
            spec = read_color(specular, specular_format, npix)[src][:, :3]
        g = np.zeros((23, npix), f32)
        g[0:3] = P.T
        g[3:6] = (u * ns).T
        g[6:9] = (t * ns).T
        g[9:12] = (b * ns).T
        g[12:15] = su.T
        g[15:18] = alb[:, :3].T
        g[18] = f32(1.0) if flags & OPAQUE else alb[:, 3]
        g[19:22] = spec.T
        if shadow is not None:
            g[22] = np.ascontiguousarray(shadow, f32).reshape(npix)[src]
        elif shadow_map is not None:
            d = light_space(P, light_vp)
            finite = np.isfinite(d).all(1)
            g[22] = np.where(finite, pcf(np.where(finite[:, None], d, f32(0.0)), shadow_map), f32(0.0))
        else:
            g[22] = NO_MAP_SHADOW
        g[:, ~surface] = 0.0
    if material is None:
        return g
    ids = np.ascontiguousarray(material, np.uint16).reshape(npix)[src].astype(np.int64)
    em = gl = None
    if emission is not None:
        table = np.asarray(emission, f32).reshape(-1, 3)
        known = surface & (ids < table.shape[0])
        em = np.where(known[None, :], table[np.where(known, ids, 0)].T, f32(0.0)).astype(f32)
    if mat_class is not None:
        cls = np.asarray(mat_class, np.uint8).reshape(-1)
        known = surface & (ids < cls.shape[0])
        gl = np.where(known, cls[np.where(known, ids, 0)], 0).astype(np.uint8)
    return g, em, gl


# ---- seeded inputs: every format of every input for one frame, with the adversarial values of the issue ----
ADVERSARIAL_NORMALS = np.array(
    [[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0], [-np.inf, 1, 2], [np.nan, np.nan, np.nan],                # zero, NaN, inf
     [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 3, 0], [-0.0, 0.0, -2.0],   # axis-aligned
     [1, 1, 0], [1, -1, 0], [0, 1, 1], [0, -1, -1], [1, 0, 1], [-1, 0, 1], [1, 1, 1], [-1, -1, -1],       # equal largest
     [0.5, 1, 1], [1, 1, 0.5], [1e-30, 0, 0], [1e30, 1e30, 0], [1e-23, 1e-23, 1e-23]], f32)               # ... and the range
ADVERSARIAL_OCT = np.array(
    [[32767, 32767], [-32767, 32767], [32767, -32767], [-32767, -32767], [-32768, -32768], [-32768, 0], [0, -32768],
     [-32768, 32767], [0, 0], [32767, 0], [0, 32767], [-32767, 0], [16384, 16383], [16384, 16384], [-16384, -16384],
     [1, -1], [-1, 0]], np.int16)
ADVERSARIAL_COLORS = np.array([[np.nan, 0.5, 0.5, 1.0], [np.inf, 0.0, -1.0, 0.5], [2.0, 6e-8, 1e-7, 0.49], [0.1, 0.2, 0.3, -0.0],
                               [0.1, 0.2, 0.3, np.nan], [65504.0, -65504.0, 6.1e-5, 0.5]], f32)


def seeded_inputs(w, h, seed, no_surface=0.05, nmat=5):
    """Everything an import of a w x h frame can be handed, in every format: dicts position / normal / shading_normal /
    albedo / specular keyed by format, plus shadow, material, inv_view_proj (column-major [16]) and depth_clear.  About
    `no_surface` of the pixels have no surface in the formats that can say so; the adversarial values sit at seeded places."""
    r = np.random.default_rng(seed)
    n = w * h

    def place(values, special):
        k = min(len(special), n)
        values[r.permutation(n)[:k]] = special[r.permutation(len(special))[:k]]
        return values

    hole = r.random(n) < no_surface
    P = (r.random((n, 3)) * 120.0 - 60.0).astype(f32)
    pw = np.where(hole, 0.0, np.where(r.random(n) < 0.5, 1.0, r.normal(size=n))).astype(f32)
    pw[~hole & (pw == 0)] = 1.0
    if n > 8:
        pw[r.integers(n)] = -0.0                            # w = -0 is no surface too: -0 == 0
    depth = (0.05 + 0.9 * r.random(n)).astype(f32)
    depth_clear = f32(1.0)
    depth[hole] = depth_clear
    depth = place(depth, np.array([np.nan, 0.0, 0.5], f32))
    # a perspective camera looking down -z from (3, 4, 60), inverted in float64
    fov, aspect, near, far = np.radians(60.0), w / h, 0.5, 400.0
    t = 1.0 / np.tan(fov / 2)
    proj = np.array([[t / aspect, 0, 0, 0], [0, t, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]])
    view = np.eye(4); view[:3, 3] = (-3.0, -4.0, -60.0)
    inv = np.linalg.inv(proj @ view)
    nrm = place(r.normal(size=(n, 3)).astype(f32), ADVERSARIAL_NORMALS)
    snrm = place(r.normal(size=(n, 3)).astype(f32), ADVERSARIAL_NORMALS)

    def halves(v):
        out = np.zeros((n, 4), np.float16)
        with np.errstate(all="ignore"):
            out[:, :3] = v.astype(np.float16)
        out[:, 3] = r.random(n).astype(np.float16)
        out[r.integers(n), :3] = np.array([6e-8, -6e-8, 3e-5], np.float16)       # subnormal halves
        return out

    def colors():
        c = r.random((n, 4)).astype(f32)
        c[:, 3] = np.where(r.random(n) < 0.2, c[:, 3], 1.0)
        c8 = r.integers(0, 256, (n, 4)).astype(np.uint8)
        c8[:, 3] = np.where(r.random(n) < 0.2, c8[:, 3], 255)
        c32 = place(c.copy(), ADVERSARIAL_COLORS)
        with np.errstate(all="ignore"):
            c16 = place(c.copy(), ADVERSARIAL_COLORS).astype(np.float16)
        return {COLOR_UNORM8X4: c8, COLOR_F16X4: c16, COLOR_F32X4: c32}

    return dict(
        position={POSITION_F32X3: P, POSITION_F32X4: np.concatenate([P, pw[:, None]], 1), DEPTH_F32: depth},
        normal={NORMAL_F32X3: nrm, NORMAL_F16X4: halves(nrm), NORMAL_OCT: place(r.integers(-32768, 32768, (n, 2)).astype(np.int16), ADVERSARIAL_OCT)},
        shading_normal={NORMAL_F32X3: snrm, NORMAL_F16X4: halves(snrm),
                        NORMAL_OCT: place(r.integers(-32768, 32768, (n, 2)).astype(np.int16), ADVERSARIAL_OCT)},
        albedo=colors(), specular=colors(),
        shadow=(r.random(n) * 2.775).astype(f32),
        material=place(r.integers(0, nmat + 2, n).astype(np.uint16), np.array([65535, nmat, nmat - 1, 0], np.uint16)),
        inv_view_proj=np.ascontiguousarray(inv.T.reshape(16), f32), depth_clear=depth_clear)


# ---- packers: a set of 23 planes [23, h*w] into each input format (frame order; flip=True: row 0 on top) ----
def _rows(a, w, h, flip):
    a = a.reshape(h, w, *a.shape[1:])
    return np.ascontiguousarray(a[::-1] if flip else a).reshape(h * w, *a.shape[2:])


def pack_position(planes, fmt, w, h, flip=False, surface=None):
    P = np.ascontiguousarray(planes[0:3].T, f32)
    if fmt == POSITION_F32X4:
        wcol = np.ones(P.shape[0], f32) if surface is None else surface.astype(f32)
        P = np.concatenate([P, wcol[:, None]], 1)
    return _rows(P, w, h, flip)


def pack_vectors(v, fmt, w, h, flip=False):
    """vectors [h*w, 3] as a normal target"""
    v = np.ascontiguousarray(v, f32)
    if fmt == NORMAL_F16X4:
        out = np.zeros((v.shape[0], 4), np.float16)
        with np.errstate(all="ignore"):
            out[:, :3] = v.astype(np.float16)
        return _rows(out, w, h, flip)
    if fmt == NORMAL_OCT:
        return _rows(oct_encode(v), w, h, flip)
    return _rows(v, w, h, flip)


def oct_encode(v):
    """unit-ish vectors [k, 3] -> octahedral SNORM16 x 2 (zero and non-finite vectors encode as (0, 0))"""
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        s = np.abs(v).sum(1)
        p = v[:, :2] / s[:, None]
        fold = v[:, 2] < 0
        q = (1.0 - np.abs(p[:, ::-1])) * np.where(p >= 0, 1.0, -1.0)
        p = np.where(fold[:, None], q, p)
        p = np.where(np.isfinite(p), p, 0.0)
    return np.clip(np.rint(p * 32767.0), -32767, 32767).astype(np.int16)


def pack_color(c, fmt, w, h, flip=False):
    """colours [h*w, 4] in [0, 1] as a colour target"""
    c = np.ascontiguousarray(c, f32)
    if fmt == COLOR_UNORM8X4:
        return _rows(np.clip(np.rint(np.nan_to_num(c) * 255.0), 0, 255).astype(np.uint8), w, h, flip)
    if fmt == COLOR_F16X4:
        with np.errstate(all="ignore"):
            return _rows(c.astype(np.float16), w, h, flip)
    return _rows(c, w, h, flip)


def project_depth(P, view_proj, zero_to_one=False):
    """(x, y, depth) in float64 of world points P [k, 3] under the column-major matrix view_proj [16]: window x, y in
    pixels / frame size units [-1, 1] and the depth value a depth buffer of that convention would hold."""
    m = np.asarray(view_proj, np.float64).reshape(4, 4).T
    c = np.concatenate([np.asarray(P, np.float64), np.ones((len(P), 1))], 1) @ m.T
    ndc = c[:, :3] / c[:, 3:4]
    return ndc[:, 0], ndc[:, 1], ndc[:, 2] if zero_to_one else (ndc[:, 2] + 1.0) / 2.0
