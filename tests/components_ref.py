"""numpy restatement of the masked composite of include/vct.h (lighting components, S/VoxelConeTracing.fs:188-227)
and of the per-component outputs, from G-buffer planes and per-pixel raw cones (oracle.trace(..., want_cones=True)).

fp32 throughout, in the kernel's operation order; the 6-cone gather is an fma chain (fs:194-199), emulated in fp64
(the product of two fp32 values is exact there).  With SHOW_ALL it is the oracle's composite (tests pin that).
max(x, 0) is C's fmaxf as in the oracle and the kernel: a NaN dot product (P == camera, a NaN normal) gives 0."""
import numpy as np

SHOW_DIFFUSE, SHOW_INDIRECT_DIFFUSE, SHOW_SPECULAR, SHOW_INDIRECT_SPECULAR, SHOW_AMBIENT_OCCLUSION = 1, 2, 4, 8, 16
SHOW_ALL = 31
AOV_INDIRECT_DIFFUSE, AOV_INDIRECT_SPECULAR, AOV_DIRECT = 1, 2, 4
CONE_WEIGHTS = np.array([0.25, 0.15, 0.15, 0.15, 0.15, 0.15], np.float32)      # trace.fs:48

f32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(a):
    ln = np.sqrt(_dot(a, a))
    return [a[0] / ln, a[1] / ln, a[2] / ln]


def _reflect(i, n):
    d = f32(2.0) * _dot(n, i)
    return [i[0] - d * n[0], i[1] - d * n[1], i[2] - d * n[2]]


def marched_groups(mask, aov=0):
    """(diffuse cones marched, specular cone marched) -- the skip rule of include/vct.h."""
    diffuse = bool(mask & (SHOW_INDIRECT_DIFFUSE | SHOW_AMBIENT_OCCLUSION)) or bool(aov & AOV_INDIRECT_DIFFUSE)
    specular = (bool(mask & SHOW_INDIRECT_SPECULAR) or (bool(mask & SHOW_AMBIENT_OCCLUSION) and bool(mask & SHOW_SPECULAR))
                or bool(aov & AOV_INDIRECT_SPECULAR))
    return diffuse, specular


def gather(cones):
    """inDirectDiffuse (fs:194-199): fma chain over cones 0..5, [npix, 4] fp32."""
    ind = np.zeros((cones.shape[0], 4), np.float32)
    for i in range(6):
        ind = _fma(np.full_like(ind, CONE_WEIGHTS[i]), cones[:, i, :], ind)
    return ind


def composite(planes, cones, cam, light, ambient=0.1, shininess=20.0, mask=SHOW_ALL):
    """Returns dict(rgba32f [npix, 4], ind, spec_cone, direct [npix, 4] raw per-component values, alive [npix])."""
    g = np.asarray(planes, np.float32)
    cones = np.asarray(cones, np.float32)
    with np.errstate(all="ignore"):
        P = [g[0], g[1], g[2]]
        N = [g[12], g[13], g[14]]
        alb = g[15:19]
        shadow = g[22]
        alive = ~(g[18] < f32(0.5))
        ind = gather(cones)
        sc = cones[:, 6, :]
        L = _normalize([f32(light[0]), f32(light[1]), f32(light[2])])                       # :179
        E = _normalize([f32(cam[0]) - P[0], f32(cam[1]) - P[1], f32(cam[2]) - P[2]])        # :181
        cos_theta = np.fmax(_dot(N, L), f32(0.0))                                            # :188
        raw_dd = shadow * cos_theta
        dd = raw_dd if mask & SHOW_DIFFUSE else np.zeros_like(raw_dd)                        # :190
        occ = f32(1.0) - ind[:, 3] if mask & SHOW_AMBIENT_OCCLUSION else np.ones_like(raw_dd)   # :201
        ird = ind[:, :3] if mask & SHOW_INDIRECT_DIFFUSE else np.zeros_like(ind[:, :3])      # :203
        D = [(dd + occ * ird[:, c]) * alb[c] for c in range(3)]                              # :205
        R = _normalize(_reflect([-L[0], -L[1], -L[2]], N))                                   # :212
        spec = np.power(np.fmax(_dot(E, R), f32(0.0)), f32(shininess)).astype(np.float32)   # :213
        raw_ds = spec * shadow
        ds = raw_ds if mask & SHOW_SPECULAR else np.zeros_like(raw_ds)                       # :215
        socc = f32(1.0) - sc[:, 3] if mask & SHOW_AMBIENT_OCCLUSION else np.ones_like(raw_dd)   # :221
        irs = sc[:, :3] if mask & SHOW_INDIRECT_SPECULAR else np.zeros_like(sc[:, :3])
        S = [(irs[:, c] + socc * ds) * g[19 + c] for c in range(3)]                          # :223
        A = [f32(ambient) * alb[c] * occ for c in range(3)]                                  # :225
        out = np.stack([(A[c] + D[c]) + S[c] for c in range(3)] + [alb[3]], axis=1).astype(np.float32)   # :227
    cc = f32(0.5) if ambient < 0.5 else f32(1.0)                                             # VCT.h:156-159
    out[~alive] = np.array([cc, cc, cc, 1.0], np.float32)
    direct = np.stack([raw_dd, raw_ds, shadow, np.ones_like(shadow)], axis=1).astype(np.float32)
    zero = ~alive
    ind = ind.copy(); ind[zero] = 0
    scz = sc.copy(); scz[zero] = 0
    direct[zero] = 0
    return dict(rgba32f=out, ind=ind, spec_cone=scz, direct=direct, alive=alive)


def masked_cones(cones, mask, aov=0):
    """The cones a trace with this mask leaves: groups nothing reads are zero (not marched)."""
    c = np.array(cones, np.float32, copy=True)
    dif, spc = marched_groups(mask, aov)
    if not dif:
        c[:, :6] = 0
    if not spc:
        c[:, 6] = 0
    return c


def marched_steps(steps, mask, aov=0):
    """Executed cone steps of a trace with this mask, from the oracle's per-cone steps [npix, 7]."""
    dif, spc = marched_groups(mask, aov)
    s = np.asarray(steps, np.int64)
    return int((s[:, :6].sum() if dif else 0) + (s[:, 6].sum() if spc else 0))


def to_f16_bits(x):
    """Round-to-nearest-even fp32 -> fp16 bits (numpy's cast: the rounding of the kernel's pack and the oracle)."""
    with np.errstate(over="ignore"):          # a value that rounds to 65520 or more becomes inf, as in the kernel's pack
        return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def header_constants(path):
    """VCT_SHOW_* and VCT_AOV_* values parsed from include/vct.h."""
    import re
    txt = open(path).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(VCT_(?:SHOW|AOV)_[A-Z_]+)\s*=\s*(\d+)", txt)}
