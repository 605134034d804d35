"""Adversarial G-buffers for the cone trace's tile front end and composite (csrc/vct_trace.hip cone_frame_from_gbuffer,
cone_dir, specular_dir, the alive test, composite), beside synth.random_gbuffer / coherent_gbuffer.  Test
infrastructure, NumPy only: no oracle, no GPU.

get_case(name, w, h) takes the coherent floor of synth.coherent_gbuffer and overwrites chosen pixels -- the CASE PIXELS --
with the values of one family; it returns a Case with planes [23, h*w], a per-pixel class and the touched mask.  The
class says what the G-buffer contract of include/vct.h promises for the pixel:
    finite           every plane's effect is finite: the oracle's fp32 rgb is finite
    nonfinite_rgb    a degenerate frame / view vector / NaN term: some rgb channel is NaN or inf, in this pixel only
    discarded        albedo.a < 0.5: the clear colour
    beyond_contract  a finite cone sample position would leave the position bound (only with beyond=True; never sent
                     to a GPU: the float -> int conversion of its texel coordinate is not defined)
Classes are declared from the arithmetic (each spec says why); tests/test_gbuffer_cases.py holds the oracle to them.

Placement (every frame is 3 x 2 tiles of 8 x 8; 21 x 13 is ragged in both directions), see _place:
    (3, 3)    lane 27 of tile (0, 0), whose other lanes are the coherent floor: the cooperative sampler's anchor
    (8, 0)    the first live lane of tile (1, 0), whose lane 27 -- pixel (11, 3) -- is discarded: the fallback anchor
    tile (2, 0)   every in-frame pixel is a case pixel
    tile (0, 1)   every spec of the family once, in order
"""
import numpy as np

import synth

f32 = np.float32
FINITE, NONFINITE_RGB, DISCARDED, BEYOND = "finite", "nonfinite_rgb", "discarded", "beyond_contract"
CAM, LIGHT = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)
FRAMES = ((24, 16), (21, 13))
V = 16
MODEL_SCALE = f32(0.05)
LIMIT_GRIDS = 1048576.0                      # VCT_GBUFFER_LIMIT_GRIDS of include/vct.h
# grid size -> max_distance: the default, and the grid size outside the shipped divisor table that the device verifies
# at run time (test_gpu_march_params.VERIFIED_G, traced with max_distance = G / 2 there too)
GRIDS = {150.0: 75.0, 100.0: 50.0}
INF, NAN = f32(np.inf), f32(np.nan)


class Env:
    def __init__(self, G):
        self.G = f32(G)
        self.max_distance = f32(GRIDS[float(G)])
        self.vs = f32(G) / f32(V)
        self.cam = np.array(CAM, f32)
        self.light = np.array(LIGHT, f32)


class Case:
    def __init__(self, name, w, h, env, planes, cls, touched, base):
        self.name, self.w, self.h = name, w, h
        self.G, self.max_distance = float(env.G), float(env.max_distance)
        self.planes, self.cls, self.touched, self.base = planes, cls, touched, base

    def config(self):
        """vct_config fields of the case (the oracle's parameters carry the same values)."""
        return dict(voxel_dim=V, width=self.w, height=self.h, grid_world_size=self.G, max_distance=self.max_distance)


def base_gbuffer(w, h, G=150.0):
    """The coherent floor, scaled with the grid (G = 150: synth.coherent_gbuffer's defaults)."""
    return synth.coherent_gbuffer(w, h, plane_y=-20.0 * G / 150.0, extent=60.0 * G / 150.0)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(a):
    """fp32 normalize in the oracle's operation order (IEEE sqrt and divisions)."""
    a = np.asarray(a, f32)
    ln = np.sqrt(_dot(a, a))
    return np.array([a[0] / ln, a[1] / ln, a[2] / ln], f32)


def _below(x):
    """The largest fp32 <= the float64 x."""
    v = f32(x)
    return v if float(v) <= x else np.nextafter(v, f32(0.0) if x > 0 else -INF)


def exceeds_position_bound(planes, G, max_distance):
    """Per pixel: live, planes 0-5 finite, and |P| + |N_world| * vs + max_distance > LIMIT_GRIDS * G on some axis (the
    position contract of include/vct.h, evaluated in float64).  A non-finite position or normal is inside the contract:
    its samples are NaN whatever the texel index."""
    g = np.asarray(planes, np.float64)
    reach = np.abs(g[0:3]) + np.abs(g[3:6]) * (G / V) + max_distance
    with np.errstate(invalid="ignore"):
        return ~(planes[18] < f32(0.5)) & np.isfinite(g[0:6]).all(0) & (reach > LIMIT_GRIDS * G).any(0)


# ---- families: lists of specs; a spec edits one pixel's 23 values in place and returns its class ----------------------------
def _tangent_frames(env, beyond):
    def t_zero(px):            # c1 = c2 = 0 and det = 0: inv_det = inf, 0 * inf = NaN in every cone direction
        px[6:9] = 0
        return NONFINITE_RGB

    def n_zero(px):            # det = T . (B x 0) = 0
        px[3:6] = 0
        return NONFINITE_RGB

    def b_parallel_t(px):      # T x B = 0 exactly: cone 0 runs along normalize(0 * inv_det) = NaN, whatever det rounds to
        px[9:12] = px[6:9]
        return NONFINITE_RGB

    def mirrored(px):          # frame x -1: det < 0, the cross products keep their sign, every direction flips
        px[3:12] *= f32(-1)
        return FINITE

    def sheared(px):           # non-unit, non-orthogonal, det finite and far from 0
        n, t, b = px[3:6].copy(), px[6:9].copy(), px[9:12].copy()
        px[3:6] = f32(0.7) * n
        px[6:9] = f32(2.0) * t + f32(0.5) * n
        px[9:12] = f32(1.5) * b + f32(0.3) * t - f32(0.2) * n
        return FINITE

    def bump_zero(px):         # cos_theta = 0, R = normalize(-L), the specular cone runs along -E: all finite
        px[12:15] = 0
        return FINITE

    def bump_long(px):
        px[12:15] *= f32(3.0)
        return FINITE

    def bump_opposite(px):
        px[12:15] *= f32(-1)
        return FINITE

    return [t_zero, mirrored, n_zero, sheared, b_parallel_t, bump_zero, bump_long, bump_opposite]


def _frame_scales(env, beyond):
    """Planes 3-11 = unit frame * s.  det ~ s^3: 1e-36 at 1e-12, subnormal with a finite reciprocal at 1.5e-13 (3.4e-39 >
    1 / FLT_MAX), subnormal with an infinite reciprocal at 1e-13, 0 at 1e-16 and below.  Upwards the frame itself stays
    finite until det overflows (s > 7e12), but N_world * vs carries the cone start out of the position bound first
    (s * vs > 2^20 G: s > 1.7e7 at V = 16).  So the overflowing determinant inside the contract scales T and B only and
    leaves N_world at model scale: at 1e25 every product of T x B (1e50) and of T . (B x N) (5e48; its largest term is at
    least a third of that) overflows, det = +-inf, inv_det = +-0, the columns B x N and N x T (5e23) become +-0 and
    T x B (inf, or inf - inf) * 0 is NaN; every diffuse cone has a share of that column, so all six run along NaN.  At
    1e18 the same frame stays finite: T x B ~ 1e36, det ~ 5e34, inv_det ~ 2e-35 is a normal number."""
    def scaled(s, cls):
        def spec(px):
            px[3:12] = (px[3:12] / MODEL_SCALE) * f32(s)
            return cls
        return spec

    def tb_scaled(s, cls):
        def spec(px):
            px[6:12] = (px[6:12] / MODEL_SCALE) * f32(s)
            return cls
        return spec

    specs = [scaled(1e-12, FINITE), scaled(1e-13, NONFINITE_RGB), scaled(1e-6, FINITE), scaled(1e-16, NONFINITE_RGB),
             scaled(1.0, FINITE), scaled(1.5e-13, FINITE), scaled(1e3, FINITE), scaled(1e-20, NONFINITE_RGB),
             scaled(1e6, FINITE), scaled(1e7, FINITE), tb_scaled(1e18, FINITE), tb_scaled(1e25, NONFINITE_RGB)]
    if beyond:
        specs += [scaled(1e8, BEYOND), scaled(1e12, BEYOND), scaled(1e13, BEYOND)]
    return specs


def _view_vector(env, beyond):
    L = _normalize(env.light)

    def on_camera(px):         # E = normalize(0) = NaN: fmaxf drops it from the Phong term, the specular cone's direction keeps it
        px[0:3] = env.cam
        return NONFINITE_RGB

    def ulp_from_camera(px):   # |cam - P|^2 = ulp^2 ~ 6e-14: normal, E = (-1, 0, 0)
        px[0:3] = env.cam
        px[0] = np.nextafter(env.cam[0], INF)
        return FINITE

    def n_perp_l(px):          # L.y * L.x - L.x * L.y + 0 * L.z == 0 exactly: cos_theta = 0, R = -L
        px[12:15] = [L[1], -L[0], 0.0]
        return FINITE

    def n_anti_l(px):          # cos_theta clamps to 0, R = L
        px[12:15] = -L
        return FINITE

    def n_along_e(px):         # reflect(-E, E) = E: the specular cone runs at the camera
        px[12:15] = _normalize(env.cam - px[0:3])
        return FINITE

    def n_perp_e(px):          # reflect(-E, N) = -E: away from the camera, through the surface
        E = _normalize(env.cam - px[0:3])
        px[12:15] = [E[1], -E[0], 0.0]
        return FINITE

    return [on_camera, ulp_from_camera, n_perp_l, n_anti_l, n_along_e, n_perp_e]


def position_limit(env, nw):
    """The largest in-contract |P| on an axis whose N_world component is nw (float64)."""
    return LIMIT_GRIDS * float(env.G) - float(env.max_distance) - abs(float(nw)) * float(env.vs)


def _positions(env, beyond):
    G, vs = env.G, env.vs
    specs = []

    def tiny(v):
        # an axis-aligned frame with N_world along y: cone 0 runs along y with dir.x = dir.z = 0 exactly, so its sample
        # positions carry P.x and P.z unchanged into the divide by G / 2 (the other cones add dir * dist)
        def spec(px):
            s = MODEL_SCALE
            px[3:6], px[6:9], px[9:12], px[12:15] = [0, s, 0], [s, 0, 0], [0, 0, s], [0, 1, 0]
            if np.signbit(v):
                px[3], px[5] = f32(-0.0), f32(-0.0)
            px[0], px[2] = v, v
            return FINITE
        return spec

    t100 = f32(2.0 ** -100)
    for v in (f32(0.0), f32(-0.0), f32(1e-45), f32(-1e-45), t100, np.nextafter(t100, f32(0)), np.nextafter(t100, f32(1)),
              -t100, f32(2.0 ** -126)):
        specs.append(tiny(v))

    def on_axis(axis, v):
        def spec(px):
            px[axis] = v
            return FINITE
        return spec

    for axis in range(3):
        for sgn in (-1.0, 1.0):
            specs.append(on_axis(axis, f32(sgn) * (G * f32(0.5))))               # exactly on a grid face
    for n, i in enumerate((0, 7, 15)):                                          # texel centres of level 0
        specs.append(on_axis(n % 3, (f32(i) + f32(0.5)) * vs - G * f32(0.5)))
    for n, i in enumerate((1, 8)):                                              # texel faces of level 0
        specs.append(on_axis((n + 1) % 3, f32(i) * vs - G * f32(0.5)))
    specs += [on_axis(0, f32(2.5) * G), on_axis(1, f32(-3.25) * G), on_axis(2, f32(7.0) * G)]     # grids outside: wrap repeats

    def far_corner(px):
        px[0:3] = [-10.0 * G, 10.0 * G, -10.0 * G]
        return FINITE
    specs.append(far_corner)

    def at_limit(axis, sgn, step, cls=FINITE):
        def spec(px):
            v = _below(position_limit(env, px[3 + axis]))
            for _ in range(abs(step)):
                v = np.nextafter(v, f32(0) if step < 0 else INF)
            px[axis] = f32(sgn) * v
            return cls
        return spec

    for axis in range(3):
        for sgn in (-1.0, 1.0):
            specs += [at_limit(axis, sgn, 0), at_limit(axis, sgn, -1)]
    if beyond:
        specs += [at_limit(0, 1.0, 1, BEYOND), at_limit(1, -1.0, 1, BEYOND), at_limit(2, 1.0, 1, BEYOND)]

        def past_int_range(px):    # u ~ 2^31.5: where the GPU saturates and C++ is undefined
            px[0] = f32(3.0e9) * G / f32(V)
            return BEYOND
        specs.append(past_int_range)
    return specs


def _alive_test(env, beyond):
    def alpha(v, cls):
        def spec(px):
            px[18] = v
            return cls
        return spec

    # trace.fs:171 discards on alpha < 0.5: NaN compares false, so a NaN alpha is NOT discarded (and is the pixel's alpha)
    return [alpha(f32(0.5), FINITE), alpha(np.nextafter(f32(0.5), f32(0)), DISCARDED), alpha(NAN, FINITE),
            alpha(f32(-0.0), DISCARDED), alpha(INF, FINITE), alpha(f32(2.0), FINITE)]


def _colours(env, beyond):
    """fp16 rounds 65519 down to 65504 and 65520 up to inf.  Alpha passes through the composite untouched, so those exact
    values go there; rgb reaches the neighbourhood through scaled albedo / specular colour.  A pixel that overflows fp16 has
    shadow = 0: its Phong term is exactly 0, so the frame must match the oracle's bits (test_gpu_trace_inputs.py)."""
    def alpha(v):
        def spec(px):
            px[18] = v
            return FINITE
        return spec

    def albedo(k, dark):
        def spec(px):
            px[15:18] *= f32(k)
            if dark:
                px[22] = 0
            return FINITE
        return spec

    def specular(k, dark):
        def spec(px):
            px[19:22] *= f32(k)
            if dark:
                px[22] = 0
            return FINITE
        return spec

    def albedo_values(px):
        px[15:18] = [65504.0, 65519.0, 65520.0]
        px[22] = 0
        return FINITE

    def both_negative(px):
        px[15:18] *= f32(-1)
        px[19:22] *= f32(-1)
        return FINITE

    def shadow(v, cls=FINITE):
        def spec(px):
            px[22] = v
            return cls
        return spec

    return [alpha(f32(65504.0)), albedo(1e3, False), alpha(f32(65519.0)), alpha(f32(65520.0)), alpha(f32(1e5)),
            albedo(1e5, True), albedo(1e6, True), albedo(1e30, True), albedo_values, specular(1e3, False),
            specular(1e6, True), specular(1e30, True), albedo(-1.0, False), specular(-1.0, False), both_negative,
            shadow(f32(0.0)), shadow(f32(1.0)), shadow(f32(-0.25)), shadow(f32(1.5)), shadow(NAN, NONFINITE_RGB)]


FAMILIES = {
    "tangent_frames": (_tangent_frames, 150.0),
    "frame_scales": (_frame_scales, 150.0),
    "view_vector": (_view_vector, 150.0),
    "positions_g150": (_positions, 150.0),
    "positions_g100": (_positions, 100.0),
    "alive_test": (_alive_test, 150.0),
    "colours": (_colours, 150.0),
}
CASE_NAMES = tuple(FAMILIES)


def _place(name, w, h, env, specs):
    assert (w + 7) // 8 == 3 and (h + 7) // 8 == 2 and 0 < len(specs) <= 8 * (h - 8)
    base = base_gbuffer(w, h, float(env.G))
    g = base.reshape(23, h, w).copy()
    cls = np.full((h, w), FINITE, object)
    touched = np.zeros((h, w), bool)
    slots = [(3, 3), (8, 0)]
    slots += [(x, y) for y in range(8) for x in range(16, w)]
    first_of_each = len(slots)
    slots += [(i % 8, 8 + i // 8) for i in range(len(specs))]
    g[18, 3, 11] = 0.0                                           # lane 27 of tile (1, 0)
    cls[3, 11], touched[3, 11] = DISCARDED, True
    def first_live_spec():
        """The fallback anchor must be alive: the family's first spec after specs[0] that does not discard the pixel."""
        for spec in specs[1:] + specs[:1]:
            px = g[:, 0, 8].copy()
            with np.errstate(all="ignore"):
                spec(px)
            if not px[18] < f32(0.5):
                return spec
        raise AssertionError(name)

    for k, (x, y) in enumerate(slots):
        px = g[:, y, x].copy()
        spec = specs[(k - first_of_each) % len(specs)] if k >= first_of_each else specs[k % len(specs)]
        if k == 1:
            spec = first_live_spec()
        with np.errstate(all="ignore"):
            cls[y, x] = spec(px)
        g[:, y, x] = px
        touched[y, x] = True
    return Case(name, w, h, env, np.ascontiguousarray(g.reshape(23, h * w), f32), cls.ravel(), touched.ravel(), base)


def get_case(name, w, h, beyond=False):
    family, G = FAMILIES[name]
    env = Env(G)
    return _place(name, w, h, env, family(env, beyond))


# ---- the tiled device layout (include/vct.h VCT_GB_TILED) ---------------------------------------------------------------------
def to_tiled(planes, w, h):
    """(tiled [ty, tx, 23, 64] with zero padding, in_frame [ty, tx, 64])."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    img = np.zeros((23, ty * 8, tx * 8), f32)
    img[:, :h, :w] = np.asarray(planes, f32).reshape(23, h, w)
    inside = np.zeros((ty * 8, tx * 8), bool)
    inside[:h, :w] = True
    tiled = img.reshape(23, ty, 8, tx, 8).transpose(1, 3, 0, 2, 4).reshape(ty, tx, 23, 64)
    return np.ascontiguousarray(tiled), inside.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty, tx, 64)


def poison_padding(tiled, in_frame):
    """Out-of-frame lanes of every plane (alpha >= 0.5 included) filled with NaN, +inf, -inf and 3e38 in turn."""
    out = tiled.copy()
    junk = np.array([NAN, INF, -INF, f32(3e38)], f32)
    fill = junk[(np.arange(23)[:, None] + np.arange(64)[None, :]) % 4]          # [23, 64]
    pad = ~in_frame[:, :, None, :] & np.ones((1, 1, 23, 1), bool)
    out[pad] = np.broadcast_to(fill, tiled.shape)[pad]
    assert (out[:, :, 18, :][~in_frame] != 0).all()
    return out
