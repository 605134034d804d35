"""Float64 restatement of the three stages that have no code in the project this one was modelled on -- the voxel
attributes, the second bounce and the directional (anisotropic) mip chains with their sampling route -- NumPy only.
Test infrastructure.

Written from PROSE: the text of oracle/vct_oracle.h ("second bounce", "anisotropic (directional) mip volumes"),
include/vct.h and SURVEY.md Appendix A (A.1 - A.5) and section 8 row a3.  Not from oracle/vct_oracle.cpp and not from the
kernels: no operation order, fused operation or fp32 intermediate is taken over.  Every input (uint8 texels, float32
parameters and positions) is widened exactly and everything after that is plain float64.  The cone table is stated here
by itself, from row a3 ("weights .25, .15 x 5", six unit directions): one cone along the normal, five tilted 60 degrees
from it and 72 degrees apart starting at +y, i.e. (sin 60 sin 72k, sin 60 cos 72k, 1/2), to the six decimals a shader
literal holds.

The comparison rule (agree): a byte b agrees with an exact value x (LSB units, clamped to [0, 255]) when
|b - x| <= 0.5 + eps.  eps bounds the fp32 roundings of the route that produced b; U = 2^-24 is fp32's unit roundoff.

  eps_mip = 16 * 255 * U = 2.4e-4 LSB, one directional level from its eight children:
      decode of F and B (byte / 255): U each on values <= 1; 1 - F.a: its decode's U plus its own U; the fused
      F + (1 - F.a) * B: 3 U carried by the product, 2 U for its one rounding on a value <= 2 -- 6 U per pair; four pairs
      24 U, their three sums (values <= 4, 6, 8) 18 U; the quarter is exact: 10.5 U on a parent <= 2.  The scale by 255
      and the + 0.5 in front of the floor round once each on a value that matters only below 256: 2 * 256 U / 255 each.
      10.5 + 2 + 2 < 16.  A level >= 2 is built from the previous level's BYTES as downloaded, so this never compounds.

  eps_bounce(V, G, constants) = 255 * 2 * sum over the steps k of an unstopped cone of E_k, + 4 * 255 * U:
      E_k = (3 * C_POS(k) * N_k + 30) * U bounds one sample's fp32 error.  N_k = V >> floor(lod_k) is the finer of the two
      levels the step blends; a texel coordinate is position / G * N_k, so an error of the position in units of G is
      multiplied by N_k, and a trilinear weight moves the sample by at most the largest texel difference, 1, per axis
      (3 axes).  C_POS(k) = 12 + k / 2 counts the roundings of the position in units of G: P = ((i + .5) / V - .5) * G
      three on |P| / G <= 1/2 (1.5 U); the direction (cross, two normalisations, the 3-term combination: 10 roundings)
      times dist / G <= 1/2 (5.5 U with the product's own); dist's k additions (k / 2 U); start = P + n * vs and
      start + dist * dir (1.5 U); the division by G / 2, the + 0.5 and the - 0.5 after the scale by N (3.5 U).  30 U is
      the rest of a sample: eight decodes, seven weighted sums twice, the level blend and the fp32 log2 behind its
      weight (lod <= log2 V, one ulp of it and of the quotient in front).  The march feeds a sample's error into colour,
      occlusion and alpha alike and alpha's error into every later step, hence the factor 2; the six weights sum to 1 and
      albedo, occlusion <= 1, so the gather adds nothing.  4 U: the two decodes, the product with albedo and the final
      scale.  At 16^3 / G = 150 / default constants this is 0.038 LSB, at 32^3 0.075 LSB: a worst case over ALL
      volumes (every neighbouring texel pair differing by 255), which is why the measured figures below are far inside.

Left out of the 0.5 + eps comparison, and instead held to |b - x| <= 1 + eps against the float64 run of either outcome of
the decision (the nearer one; no byte can be within 1 of two outcomes that differ by more): voxels with a cone that comes within MARGIN of a discrete decision,
      |alpha - max_alpha| <= sum_k E_k  (alpha's own accumulated bound),
      |dist - max_distance| / max_distance <= (steps + 2) * U  (dist is a sum of `steps` terms),
  or with ||n.y| - 0.9| <= 8 U (three products, two sums, a root and a quotient behind n.y, and the threshold 0.9 itself
  is the float32 0.9, 1 U away).  The share left out is capped at CAP = 2 % per case.

  A cone whose dist is formed without any rounding (the voxel size is a float32, wins the max() by more than a rounding
  and every partial sum is a float32: the 0.07 cone at 16^3 / G = 150 reaches dist = 8 * 9.375 = 75.0 = max_distance
  exactly) takes the distance test as fp32 does and is not left out for it.
  "Either outcome": the float64 bounce run again with max_alpha and max_distance moved by twice the margin each way, and
  with the other helper; the step total must lie between the smallest and the largest of these runs' totals, and equal
  the float64 total when nothing is left out.

The raw fp32 cones of the directional trace have no byte to bracket: check_cones() measures, per channel, the largest
|fp32 - float64| / max(|float64|, 1e-3) outside the left-out cones and requires equal step counts there.

Measured (tests/test_highprec_restatement.py, the oracle against this module; tests/test_gpu_highprec.py, the kernels
against it, printed the same figures to the last digit, the GPU being bit-equal to the oracle):
  bounce, 16 cases (16^3 and 32^3, both wrap modes, G = 150 / 100 / 317.3, three constant sets) and the merged chain:
      left out 0 - 0.35 % (at most 2 voxels of 578; cap 2 %), largest |b - x| - 0.5 from -7.6e-4 to -9.0e-6 -- no byte
      needed eps at all -- against eps = 0.029 - 0.104 LSB; step totals equal in every case.
      The dense 16^3 scene: 0.10 %, -3.2e-5 (eps 0.034); mover A at 64^3: 0.42 %, -2.3e-5 (eps 0.145); with the mover's
      emission table: -8.3e-5 at 16^3, -2.9e-5 at 64^3.
  directional mips, V = 8 / 16 / 32 / 64 on four volumes: nothing left out; largest |b - x| - 0.5 = 5.7e-14 (exact ties,
      up to 23,061 of 112,344 bytes, which fp32 and float64 may round either way) against eps_mip = 2.4e-4.
  albedo: 0.9f * 255 = 229.4999939 exactly; fp32 rounds the product to 229.5 and the byte is 230, 6.1e-6 beyond the half,
      inside EPS_UNORM = 3.1e-5.
  directional trace, 12 cases (two 24 x 16 frames, both wrap modes, three constant sets): left out 0 - 0.71 %, step counts
      equal everywhere, largest deviation 8.23e-5 (a cone of about 1e-3, i.e. 8e-8 absolute); CONE_DEV_MEASURED = 8.3e-5
      holds the oracle, the GPU gets CONE_BOUND = 4 x that = 3.32e-4 and measured the oracle's own figures.
"""
import numpy as np

U = 2.0 ** -24
CAP = 0.02
EPS_MIP = 16 * 255 * U
HELPER_MARGIN = 8 * U

# weights .25, .15 x 5; one cone along the normal, five at 60 degrees from it, 72 degrees apart
CONE_WEIGHTS = np.array([0.25, 0.15, 0.15, 0.15, 0.15, 0.15], np.float32).astype(np.float64)
CONE_DIRS = np.array([[0.0, 0.0, 1.0],
                      [0.0, 0.866025, 0.5],
                      [0.823639, 0.267617, 0.5],
                      [0.509037, -0.700629, 0.5],
                      [-0.509037, -0.700629, 0.5],
                      [-0.823639, 0.267617, 0.5]], np.float32).astype(np.float64)

# The oracle's raw fp32 cones of the directional trace against frame_cones(), the largest relative deviation (relative to
# max(|value|, 1e-3)) over the cases of tests/test_highprec_restatement.py test_directional_trace; the GPU, bit-equal to the
# oracle under the older tests, gets four times it for the cases that list does not hold.
CONE_DEV_MEASURED = 8.3e-5
CONE_BOUND = 4 * CONE_DEV_MEASURED


def f64(x):
    """Exact widening of a float32 (or uint8) value or array."""
    return np.asarray(x).astype(np.float64)


def params(p):
    """The float32 fields of an oracle parameter block, widened exactly."""
    return dict(V=int(p.V), G=float(np.float32(p.G)), max_distance=float(np.float32(p.max_distance)),
                max_alpha=float(np.float32(p.max_alpha)), tan_diffuse=float(np.float32(p.tan_diffuse)),
                tan_specular=float(np.float32(p.tan_specular)), wrap_repeat=int(p.wrap_repeat))


def levels_of(chain, V):
    """The isotropic chain as a list of float64 [N, N, N, 4] (z, y, x), texel = byte / 255 (A.1)."""
    out, off, n = [], 0, V
    chain = np.asarray(chain, np.uint8).reshape(-1, 4)
    while n >= 1:
        out.append(f64(chain[off:off + n ** 3].reshape(n, n, n, 4)) / 255.0)
        off += n ** 3
        n //= 2
    return out


def aniso_levels_of(aniso, V):
    """[6] lists of float64 levels 1 .. log2 V of the directional chains (entry 0 of each list is None)."""
    aniso = np.asarray(aniso, np.uint8).reshape(6, -1, 4)
    out = []
    for d in range(6):
        lv, off, n = [None], 0, V // 2
        while n >= 1:
            lv.append(f64(aniso[d, off:off + n ** 3].reshape(n, n, n, 4)) / 255.0)
            off += n ** 3
            n //= 2
        out.append(lv)
    return out


# ---- sampler (A.2, A.3) -------------------------------------------------------------------------------------------------
def tri(level, uv, wrap_repeat=1):
    """Trilinear sample of one level at texture coordinates uv [M, 3]: texel centres at (i + 0.5) / N."""
    N = level.shape[0]
    c = uv * N - 0.5
    i0 = np.floor(c)
    a = c - i0
    i0 = i0.astype(np.int64)
    i1 = i0 + 1
    if wrap_repeat:
        i0, i1 = i0 % N, i1 % N
    else:
        i0, i1 = np.clip(i0, 0, N - 1), np.clip(i1, 0, N - 1)
    out = 0.0
    for dz, wz in ((i0[:, 2], 1 - a[:, 2]), (i1[:, 2], a[:, 2])):
        for dy, wy in ((i0[:, 1], 1 - a[:, 1]), (i1[:, 1], a[:, 1])):
            for dx, wx in ((i0[:, 0], 1 - a[:, 0]), (i1[:, 0], a[:, 0])):
                out = out + level[dz, dy, dx] * (wz * wy * wx)[:, None]
    return out


def tri_aniso(alevels, l, uv, dirs, wrap_repeat=1):
    """Level l >= 1 of the directional chains for unit directions dirs [M, 3]: dir^2 . tri(chain[axis, sign])."""
    out = 0.0
    for axis in range(3):
        t = np.where((dirs[:, axis] >= 0)[:, None], tri(alevels[2 * axis][l], uv, wrap_repeat),
                     tri(alevels[2 * axis + 1][l], uv, wrap_repeat))
        out = out + (dirs[:, axis] ** 2)[:, None] * t
    return out


def texture_lod(levels, uv, lod, wrap_repeat=1, alevels=None, dirs=None):
    """textureLod: lod clamped to the chain, (1 - f) * level floor(lod) + f * the next (clamped).  With alevels the levels
    >= 1 come from the directional chains."""
    top = len(levels) - 1
    lod = np.clip(lod, 0.0, float(top))
    d1 = np.floor(lod).astype(np.int64)
    f = lod - d1
    out = np.zeros((uv.shape[0], 4))

    def level(l, m):
        if alevels is None or l == 0:
            return tri(levels[l], uv[m], wrap_repeat)
        return tri_aniso(alevels, l, uv[m], dirs[m], wrap_repeat)
    for l in np.unique(d1):
        m = d1 == l
        out[m] = level(l, m) * (1 - f[m])[:, None] + level(min(l + 1, top), m) * f[m][:, None]
    return out


def sample(levels, G, pos, lod, wrap_repeat=1, alevels=None, dirs=None):
    return texture_lod(levels, pos / G + 0.5, lod, wrap_repeat, alevels, dirs)


# ---- cone march (A.4) ---------------------------------------------------------------------------------------------------
def march(levels, pr, start_from, normal_world, dirs, tan_half, alevels=None, d_alpha=0.0, d_dist=0.0):
    """All cones of one aperture at once.  start_from, normal_world, dirs: [M, 3].  Returns (rgb-occlusion [M, 4], steps
    [M], alpha_margin [M], dist_margin [M]): the margins are each cone's smallest |alpha - max_alpha| and
    |dist - max_distance| / max_distance after any step.  d_alpha, d_dist shift the two thresholds (the alternatives of a
    near decision)."""
    V, G = pr["V"], pr["G"]
    max_a, max_d = pr["max_alpha"] + d_alpha, pr["max_distance"] * (1.0 + d_dist)
    vs = G / V
    M = dirs.shape[0]
    start = start_from + normal_world * vs
    dist = np.full(M, vs)
    acc = np.zeros((M, 4))
    alpha = np.zeros(M)
    steps = np.zeros(M, np.int64)
    am = np.full(M, np.inf)
    dm = np.full(M, np.inf)
    exact = np.full(M, float(np.float32(vs)) == vs)
    while True:
        live = (dist < max_d) & (alpha < max_a)
        if not live.any():
            break
        i = np.nonzero(live)[0]
        diam = np.maximum(vs, 2.0 * tan_half * dist[i])
        lod = np.log2(diam / vs)
        v = sample(levels, G, start[i] + dist[i, None] * dirs[i], lod, pr["wrap_repeat"], alevels, dirs[i])
        w = 1.0 - alpha[i]
        acc[i, :3] += w[:, None] * v[:, :3]
        acc[i, 3] += w * v[:, 3] / (1.0 + 0.03 * diam)
        alpha[i] += w * v[:, 3]
        dist[i] += diam
        steps[i] += 1
        am[i] = np.minimum(am[i], np.abs(alpha[i] - pr["max_alpha"]))
        # while the voxel size wins the max() by more than a rounding and every partial sum is a float32, fp32 forms
        # the same dist without any rounding: its comparison with max_distance is this one, however close
        exact[i] &= (2.0 * tan_half * (dist[i] - diam) <= vs * (1.0 - 4 * U)) & (dist[i].astype(np.float32) == dist[i])
        dm[i] = np.minimum(dm[i], np.where(exact[i], np.inf, np.abs(dist[i] - pr["max_distance"]) / pr["max_distance"]))
    return acc, steps, am, dm


def unstopped(pr, tan_half):
    """[(k, lod_k)] of a cone that nothing stops before max_distance."""
    vs = pr["G"] / pr["V"]
    dist, out = vs, []
    while dist < pr["max_distance"]:
        diam = max(vs, 2.0 * tan_half * dist)
        out.append((len(out), float(np.log2(diam / vs))))
        dist += diam
    return out


def march_error(pr, tan_half):
    """sum_k E_k of the module docstring: the fp32 route's accumulated error of one cone's alpha (and of each channel)."""
    top = int(np.log2(pr["V"]))
    return sum((3 * (12 + k / 2) * (pr["V"] >> min(int(lod), top)) + 30) * U for k, lod in unstopped(pr, tan_half))


def eps_bounce(pr):
    return 255.0 * (2.0 * march_error(pr, pr["tan_diffuse"]) + 4 * U)


def margins(pr, tan_half):
    """(alpha margin, relative distance margin) inside which a cone's termination counts as undecided."""
    return march_error(pr, tan_half), (len(unstopped(pr, tan_half)) + 2) * U


# ---- the comparison rule ------------------------------------------------------------------------------------------------
def lsb(x):
    """An exact value in [0, 1] units -> LSB units, clamped to [0, 255]."""
    return np.clip(np.asarray(x, np.float64) * 255.0, 0.0, 255.0)


def excess(b, x):
    """|b - x| - 0.5 per byte, x in LSB units (already clamped)."""
    return np.abs(f64(b) - x) - 0.5


def agree(b, x, eps, what=""):
    """Assert |b - x| <= 0.5 + eps everywhere; returns the largest |b - x| - 0.5."""
    e = excess(b, x)
    worst = float(e.max()) if e.size else -0.5
    bad = np.argwhere(e > eps)
    assert bad.shape[0] == 0, (what, "bytes outside 0.5 + eps", bad.shape[0], "worst", worst, "eps", eps, bad[:4].tolist())
    return worst


# ---- directional chains -------------------------------------------------------------------------------------------------
def aniso_level(children, d):
    """One level of direction d = 2 * axis + sign from its children, float64 [N, N, N, 4] (z, y, x) in [0, 1] units ->
    the exact parent [N/2, N/2, N/2, 4] in [0, 1] units, unclamped.  The 2x2x2 block is four pairs along the axis; per pair
    F + (1 - F.a) * B with F the child met first when travelling in direction d: towards +axis (sign 0) one comes from the
    low side, so F is the child with the lower coordinate."""
    axis, sign = d // 2, d % 2
    ax = 2 - axis                                   # the array is (z, y, x)
    lo = np.take(children, np.arange(0, children.shape[ax], 2), axis=ax)
    hi = np.take(children, np.arange(1, children.shape[ax], 2), axis=ax)
    F, B = (lo, hi) if sign == 0 else (hi, lo)
    comp = F + (1.0 - F[..., 3:4]) * B
    for other in range(3):
        if other != ax:
            n = comp.shape[other]
            comp = np.take(comp, np.arange(0, n, 2), axis=other) + np.take(comp, np.arange(1, n, 2), axis=other)
    return comp * 0.25


def aniso_chain_from_bytes(level0, aniso):
    """Exact values, in LSB units, of every texel of every directional level, each level computed from the BYTES of the
    level before it (level 0 for level 1): float64 [6, chain_texels - V^3, 4] in the layout of `aniso`."""
    V = level0.shape[0]
    aniso = np.asarray(aniso, np.uint8).reshape(6, -1, 4)
    out = np.zeros(aniso.shape)
    for d in range(6):
        prev, off, n = f64(level0) / 255.0, 0, V // 2
        while n >= 1:
            out[d, off:off + n ** 3] = lsb(aniso_level(prev, d)).reshape(-1, 4)
            prev = f64(aniso[d, off:off + n ** 3].reshape(n, n, n, 4)) / 255.0
            off += n ** 3
            n //= 2
    return out


# ---- bounce -------------------------------------------------------------------------------------------------------------
def unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def bounce_frame(n, helper_y):
    """(t, b) of the bounce's tangent frame: t = normalize(cross(helper, n)), b = cross(n, t); helper (0,1,0) where
    helper_y else (1,0,0)."""
    h = np.where(helper_y[:, None], [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    t = unit(np.cross(h, n))
    return t, np.cross(n, t)


def bounce(pr, chain0, albedo, normal, flip_helper=False, d_alpha=0.0, d_dist=0.0):
    """The second bounce.  chain0: bounce-0 chain; albedo, normal: uint8 [V, V, V, 4].  Returns a dict:
    idx [K, 3] (z, y, x) of the voxels that march, x [K, 3] the exact unclamped out.rgb in LSB units, steps [K],
    alpha_margin / dist_margin [K] (smallest over the voxel's six cones), helper_margin [K] = ||n.y| - 0.9|, and marched
    (bool [V, V, V]).  Every other voxel is copied.  flip_helper takes the other helper for every voxel."""
    V, G = pr["V"], pr["G"]
    levels = levels_of(chain0, V)
    l0 = np.asarray(chain0, np.uint8).reshape(-1, 4)[:V ** 3].reshape(V, V, V, 4)
    nb = np.asarray(normal, np.uint8)[..., :3].astype(np.int64) - 128
    marched = (l0[..., 3] != 0) & (nb != 0).any(-1)
    idx = np.argwhere(marched)
    K = idx.shape[0]
    P = ((idx[:, ::-1] + 0.5) / V - 0.5) * G                    # (x, y, z) of the voxel centre
    n = unit(f64(nb[marched][:, :3]))
    thr = float(np.float32(0.9))
    helper_y = np.abs(n[:, 1]) < thr
    t, b = bounce_frame(n, helper_y ^ flip_helper)
    dirs = unit(t[:, None, :] * CONE_DIRS[None, :, 0:1] + b[:, None, :] * CONE_DIRS[None, :, 1:2] +
                n[:, None, :] * CONE_DIRS[None, :, 2:3]).reshape(-1, 3)
    rep = lambda a: np.repeat(a, 6, axis=0)
    acc, steps, am, dm = march(levels, pr, rep(P), rep(n), dirs, pr["tan_diffuse"], d_alpha=d_alpha, d_dist=d_dist)
    ind = (acc.reshape(K, 6, 4) * CONE_WEIGHTS[None, :, None]).sum(1)
    occlusion = 1.0 - ind[:, 3]
    alb = f64(np.asarray(albedo, np.uint8)[marched][:, :3]) / 255.0
    x = (f64(l0[marched][:, :3]) / 255.0 + alb * (occlusion[:, None] * ind[:, :3])) * 255.0
    return dict(idx=idx, x=x, steps=steps.reshape(K, 6).sum(1), alpha_margin=am.reshape(K, 6).min(1),
                dist_margin=dm.reshape(K, 6).min(1), helper_margin=np.abs(np.abs(n[:, 1]) - thr), marched=marched)


def check_bounce(pr, chain0, albedo, normal, out_l0, out_steps, what=""):
    """Hold a bounce's output (level 0 uint8 [V, V, V, 4], total steps) to the float64 bounce by the module's rule.
    Returns dict(left_out share, worst |b - x| - 0.5 among the compared bytes, eps, voxels)."""
    V = pr["V"]
    r = bounce(pr, chain0, albedo, normal)
    eps = eps_bounce(pr)
    a_m, d_m = margins(pr, pr["tan_diffuse"])
    l0 = np.asarray(chain0, np.uint8).reshape(-1, 4)[:V ** 3].reshape(V, V, V, 4)
    out_l0 = np.asarray(out_l0, np.uint8).reshape(V, V, V, 4)
    assert np.array_equal(out_l0[~r["marched"]], l0[~r["marched"]]), (what, "a voxel that marches nothing was changed")
    assert np.array_equal(out_l0[..., 3], l0[..., 3]), (what, "alpha changed")
    got = out_l0[r["marched"]][:, :3]
    near_cone = (r["alpha_margin"] <= a_m) | (r["dist_margin"] <= d_m)
    near_helper = r["helper_margin"] <= HELPER_MARGIN
    out = near_cone | near_helper
    K = max(out.size, 1)
    share = float(out.sum()) / K
    assert share <= CAP, (what, "left out", share)
    worst = agree(got[~out], np.clip(r["x"][~out], 0, 255), eps, what)
    lo_steps = hi_steps = int(r["steps"].sum())
    if out.any():
        alts = [r]
        if near_cone.any():
            alts += [bounce(pr, chain0, albedo, normal, d_alpha=s * 2 * a_m, d_dist=s * 2 * d_m) for s in (-1, 1)]
        if near_helper.any():
            alts.append(bounce(pr, chain0, albedo, normal, flip_helper=True))
        e = np.min([np.abs(f64(got[out]) - np.clip(a["x"][out], 0, 255)).max(-1) for a in alts], axis=0)
        assert (e <= 1.0 + eps).all(), (what, "a left-out voxel is off either alternative", float(e.max()))
        inside = [int(a["steps"][~out].sum()) for a in alts[:1]][0]
        lo_steps = inside + min(int(a["steps"][out].sum()) for a in alts)
        hi_steps = inside + max(int(a["steps"][out].sum()) for a in alts)
    assert lo_steps <= int(out_steps) <= hi_steps, (what, "steps", int(out_steps), lo_steps, hi_steps)
    return dict(left_out=share, worst=worst, eps=eps, voxels=int(out.size), steps=int(r["steps"].sum()))


# ---- attributes ---------------------------------------------------------------------------------------------------------
def face_normal(tri_pos):
    """Front-face unit normal of a triangle (CCW = front): normalize(cross(v1 - v0, v2 - v0)), from float32 vertices."""
    v = f64(np.asarray(tri_pos, np.float32).reshape(3, 3))
    return unit(np.cross(v[1] - v[0], v[2] - v[0]))


def quantise_normal(n):
    """floor(n * 127 + 0.5) + 128 per component: in [1, 255]."""
    return (np.floor(np.asarray(n, np.float64) * 127.0 + 0.5) + 128.0).astype(np.int64)


EPS_UNORM = 2 * 256 * U     # a * 255 and the + 0.5 in front of the floor: one fp32 rounding each on a value below 256


def albedo_lsb(a):
    """A float32 material colour -> its exact value in LSB units: a * 255 with a widened exactly.  The byte is held to it by
    agree(.., EPS_UNORM): 0.9f * 255 = 229.4999939 exactly, fp32 rounds the product to 229.5 and the byte is 230."""
    return np.clip(f64(np.asarray(a, np.float32)), 0.0, 1.0) * 255.0


# ---- directional trace --------------------------------------------------------------------------------------------------
def frame_cones(pr, chain, aniso, planes, camera_pos):
    """The seven cones of every pixel of a G-buffer (planes [23, npix] float32) over the directional chains: six diffuse
    along normalize(TBN . d_i) with TBN = inverse(transpose(mat3(T, B, N))) of the raw varyings (A.5), one specular along
    reflect(-E, bump N), E = normalize(camera - P), all from P with Normal_world = the raw normal (A.4).  Returns
    (cones [npix, 7, 4], steps [npix, 7], alpha_margin [npix, 7], dist_margin [npix, 7])."""
    V = pr["V"]
    g = f64(planes)
    P, Nw, T, B, bump = g[0:3].T, g[3:6].T, g[6:9].T, g[9:12].T, g[12:15].T
    npix = P.shape[0]
    M = np.stack([T, B, Nw], axis=2)                              # columns T, B, N
    TBN = np.linalg.inv(np.transpose(M, (0, 2, 1)))
    dd = unit(np.einsum("pij,cj->pci", TBN, CONE_DIRS))           # [npix, 6, 3]
    E = unit(f64(np.asarray(camera_pos, np.float32))[None, :] - P)
    I = -E
    R = unit(I - 2.0 * (bump * I).sum(-1, keepdims=True) * bump)
    levels, alevels = levels_of(chain, V), aniso_levels_of(aniso, V)
    rep = lambda a: np.repeat(a, 6, axis=0)
    c6, s6, a6, d6 = march(levels, pr, rep(P), rep(Nw), dd.reshape(-1, 3), pr["tan_diffuse"], alevels)
    c1, s1, a1, d1 = march(levels, pr, P, Nw, R, pr["tan_specular"], alevels)
    cat = lambda six, one, tail: np.concatenate([six.reshape((npix, 6) + tail), one.reshape((npix, 1) + tail)], 1)
    return cat(c6, c1, (4,)), cat(s6, s1, ()), cat(a6, a1, ()), cat(d6, d1, ())


def check_cones(pr, chain, aniso, planes, camera_pos, got_cones, got_steps, bound=None, what=""):
    """Hold the raw fp32 cones and step counts of a directional trace to the float64 cones.  Left out (capped at CAP):
    cones within margins() of a termination decision.  Steps must be equal outside them.  Returns dict(left_out,
    dev = the largest relative deviation per channel, relative to max(|value|, 1e-3)); with `bound` it is asserted."""
    cones, steps, am, dm = frame_cones(pr, chain, aniso, planes, camera_pos)
    out = np.zeros(steps.shape, bool)
    for sl, tan in ((slice(0, 6), pr["tan_diffuse"]), (slice(6, 7), pr["tan_specular"])):
        a_m, d_m = margins(pr, tan)
        out[:, sl] = (am[:, sl] <= a_m) | (dm[:, sl] <= d_m)
    share = float(out.mean())
    assert share <= CAP, (what, "left out", share)
    got_steps = np.asarray(got_steps).reshape(steps.shape)
    bad = np.argwhere((got_steps != steps) & ~out)
    assert bad.shape[0] == 0, (what, "step counts differ", bad.shape[0], bad[:4].tolist())
    assert (np.abs(got_steps.astype(np.int64) - steps) <= 1).all(), (what, "a left-out cone is off by more than a step")
    dev = np.abs(f64(np.asarray(got_cones, np.float32)).reshape(cones.shape) - cones) / np.maximum(np.abs(cones), 1e-3)
    dev = dev[~out].max(0)
    if bound is not None:
        assert (dev <= bound).all(), (what, "cone deviation", dev.tolist(), "bound", bound)
    return dict(left_out=share, dev=dev, marched=int((cones[..., 3] > 0).sum()), steps=int(steps.sum()))
