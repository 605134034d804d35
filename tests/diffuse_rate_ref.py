"""numpy restatement of the half-rate diffuse gather of include/vct.h (vct_set_diffuse_rate(ctx, 2)): anchors, the
acceptance test, W, the interpolation and the fill set, from G-buffer planes and per-pixel raw cones
(oracle.trace(..., want_cones=True): the full-rate trace supplies every pixel's cones, this picks from them), then the
composite of components_ref with the resulting gather in place of the pixel's own.

fp32 throughout: plain multiplies, adds and compares in the header's order, one division at the end -- numpy's fp32
operations are those operations, so nothing here is inexact that the kernel is not."""
import numpy as np

import components_ref as cr
import synth

f32 = np.float32
NORMAL_COS2 = f32(0.8125)      # VCT_DIFFUSE_RATE_NORMAL_COS2
PLANE_TOL = f32(0.25)          # VCT_DIFFUSE_RATE_PLANE_TOL
WEIGHTS = (9, 3, 3, 1)
NO_ANCHOR = 255


def header_constants(path):
    """VCT_DIFFUSE_RATE_* values of include/vct.h."""
    import re
    txt = open(path).read()
    return {m.group(1): float(m.group(2)) for m in re.finditer(r"#define\s+(VCT_DIFFUSE_RATE_[A-Z0-9_]+)\s+([0-9.]+)f", txt)}


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def classify(planes, w, h, vs):
    """The geometry of a rate-2 pass: dict(alive, code [ch, cw] (anchor's place j * 2 + i or NO_ANCHOR), apix [ch, cw]
    (the anchor's pixel index), anchor, fill, marched [npix] bool, W [npix] int, accepted [4, npix] bool, cand [4, npix]
    (coarse index of candidate k; meaningless where not accepted))."""
    g = np.asarray(planes, np.float32)
    assert g.shape == (23, w * h)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    alive = ~(g[18] < f32(0.5))
    alive2 = alive.reshape(h, w)
    code = np.full((ch, cw), NO_ANCHOR, np.int64)
    apix = np.zeros((ch, cw), np.int64)
    cy, cx = np.meshgrid(np.arange(ch), np.arange(cw), indexing="ij")
    for k in (3, 2, 1, 0):                                   # the first in the order (0,0), (1,0), (0,1), (1,1) wins
        px, py = 2 * cx + (k & 1), 2 * cy + (k >> 1)
        ok = (px < w) & (py < h)
        ok[ok] = alive2[py[ok], px[ok]]
        code[ok] = k
        apix[ok] = (py * w + px)[ok]
    y, x = np.divmod(np.arange(w * h), w)
    qx, qy = x >> 1, y >> 1
    anchor = alive & (code[qy, qx] == ((y & 1) * 2 + (x & 1)))
    vs = f32(vs)
    n_p = [g[3], g[4], g[5]]
    P_p = [g[0], g[1], g[2]]
    accepted = np.zeros((4, w * h), bool)
    cand = np.zeros((4, w * h), np.int64)
    W = np.zeros(w * h, np.int64)
    with np.errstate(all="ignore"):
        l_p = _dot(n_p, n_p)
        tol = (PLANE_TOL * (vs * vs)) * l_p
        for k in range(4):
            ccx = qx + np.where(x & 1, 1, -1) * (k & 1)
            ccy = qy + np.where(y & 1, 1, -1) * (k >> 1)
            ok = (ccx >= 0) & (ccx < cw) & (ccy >= 0) & (ccy < ch)
            ccx, ccy = np.clip(ccx, 0, cw - 1), np.clip(ccy, 0, ch - 1)
            ok &= code[ccy, ccx] != NO_ANCHOR
            a = apix[ccy, ccx]
            n_k = [g[3][a], g[4][a], g[5][a]]
            P_k = [g[0][a], g[1][a], g[2][a]]
            dn = _dot(n_p, n_k)
            d = _dot([P_k[0] - P_p[0], P_k[1] - P_p[1], P_k[2] - P_p[2]], n_p)
            l_k = _dot(n_k, n_k)
            ok &= (dn > f32(0.0)) & (dn * dn >= NORMAL_COS2 * (l_p * l_k)) & (d * d <= tol)
            accepted[k] = ok & alive & ~anchor
            cand[k] = ccy * cw + ccx
            W += WEIGHTS[k] * accepted[k]
    fill = alive & ~anchor & (W == 0)
    return dict(alive=alive, code=code, apix=apix, anchor=anchor, fill=fill, marched=anchor | fill, W=W, accepted=accepted,
                cand=cand, cw=cw, ch=ch)


def gather_rate2(cones, cls):
    """ind_p [npix, 4] fp32: a marched pixel's own gather, an interpolated pixel's S / W; 0 where discarded."""
    own = cr.gather(np.asarray(cones, np.float32))
    coarse = own[cls["apix"].ravel()]                         # the sample of every quad (garbage where it has none)
    S = None
    with np.errstate(all="ignore"):
        for k in range(4):
            t = np.where(cls["accepted"][k][:, None], f32(WEIGHTS[k]) * coarse[cls["cand"][k]], f32(0.0)).astype(np.float32)
            S = t if S is None else S + t
        interp = (S / cls["W"].astype(np.float32)[:, None]).astype(np.float32)
    ind = np.where(cls["marched"][:, None], own, interp).astype(np.float32)
    ind[~cls["alive"]] = 0
    return ind


def composite_with_ind(planes, ind, spec_cone, cam, light, ambient=0.1, shininess=20.0, mask=cr.SHOW_ALL):
    """components_ref.composite with the 6-cone gather given instead of formed from the pixel's cones: the same
    operations in the same order."""
    cones = np.zeros((ind.shape[0], 7, 4), np.float32)
    cones[:, 6] = spec_cone
    keep = cr.gather
    try:
        cr.gather = lambda _cones: np.asarray(ind, np.float32)
        return cr.composite(planes, cones, cam, light, ambient, shininess, mask)
    finally:
        cr.gather = keep


def restate(planes, w, h, vs, ref, cam, light, ambient=0.1, shininess=20.0, mask=cr.SHOW_ALL, aov=0):
    """A rate-2 trace from the oracle's full-rate trace `ref` (cones, steps).  dict(rgba32f, ind, marched [npix] bool,
    cones [npix, 7, 4] and steps [npix, 7] as the debug outputs show them, total_steps, cls)."""
    cls = classify(planes, w, h, vs)
    dif, spc = cr.marched_groups(mask, aov)
    cones = cr.masked_cones(ref["cones"], mask, aov)
    steps = np.array(ref["steps"], np.uint8, copy=True)
    marched = cls["marched"] if dif else np.zeros_like(cls["marched"])
    ind = gather_rate2(cones, cls) if dif else np.zeros((w * h, 4), np.float32)
    cones[~marched, :6] = 0
    steps[~marched, :6] = 0
    if not spc:
        steps[:, 6] = 0
    out = composite_with_ind(planes, ind, cones[:, 6], cam, light, ambient, shininess, mask)
    return dict(rgba32f=out["rgba32f"], ind=out["ind"], marched=marched, cones=cones, steps=steps,
                total_steps=int(steps.astype(np.int64).sum()), cls=cls, direct=out["direct"], spec_cone=out["spec_cone"])


def _rotate_x(v, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.stack([v[0], c * v[1] - s * v[2], s * v[1] + c * v[2]]).astype(np.float32)


def mixed_gbuffer(w, h, seed=5):
    """The coherent floor of synth.coherent_gbuffer with what a half-rate gather must not blur across: a block lifted by
    10 world units, a block whose frame is tilted by 45 degrees, one-pixel-wide lifted lines at an odd x and at an odd y,
    5 % discarded pixels and four quads with 0, 1, 2 and 3 leading pixels discarded plus one quad without any."""
    g = synth.coherent_gbuffer(w, h, seed=seed).reshape(23, h, w).copy()
    g[1, h // 8:h // 8 + h // 4, w // 8:w // 8 + w // 4] += 10.0                    # lifted block
    ys, xs = slice(h // 2, h // 2 + h // 4), slice(w // 2, w // 2 + w // 4)          # tilted block
    for k in (3, 6, 9, 12):
        g[k:k + 3, ys, xs] = _rotate_x(g[k:k + 3, ys, xs], 45.0)
    lx, ly = (w // 3) | 1, (2 * h // 3) | 1
    g[1, :, lx] += 10.0
    g[1, ly, :] += 10.0
    r = np.random.default_rng(seed)
    g[18][r.uniform(size=(h, w)) < 0.05] = 0.0
    for n, q in enumerate((2, 4, 6, 8, 10)):                                         # quads along row pair 2, 3
        g[18, 2:4, 2 * q:2 * q + 2] = 1.0
        order = ((0, 0), (1, 0), (0, 1), (1, 1))
        for i, j in order[:n if n < 4 else 4]:
            g[18, 2 + j, 2 * q + i] = 0.0
    return np.ascontiguousarray(g.reshape(23, h * w), np.float32)
