"""numpy float32 restatement of the voxel view (include/vct.h "voxel view"): the ray of every pixel, its entry into the
grid and the plain cell-by-cell walk -- no empty-space skipping, every cell fetched.  Vectorised over pixels.

Every operation is one float32 operation in the written order; comparisons with NaN are false, as on the GPU.
volume: uint8 [N, N, N, 4] indexed [z, y, x] (the linear layout of the C ABI's up/downloads)."""
import numpy as np

F = np.float32
INF = F(np.inf)


def rays(m, w, h, G, N):
    """(g, e, ok): grid-unit origins and directions float32 [h * w, 3], and False where o or d is non-finite or d = 0.
    m: the column-major inverse view-projection, float32[16]."""
    m = np.asarray(m, F).reshape(16)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x, y = xs.reshape(-1).astype(F), ys.reshape(-1).astype(F)
    with np.errstate(all="ignore"):
        nx = (F(2) * (x + F(0.5))) / F(w) - F(1)
        ny = (F(2) * (y + F(0.5))) / F(h) - F(1)
        pts = []
        for nz in (F(-1), F(1)):
            r = [((m[i] * nx + m[4 + i] * ny) + m[8 + i] * nz) + m[12 + i] for i in range(4)]
            pts.append(np.stack([r[a] / r[3] for a in range(3)], axis=1).astype(F))
        o, d = pts[0], (pts[1] - pts[0]).astype(F)
        ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)
        g = ((o / F(G) + F(0.5)) * F(N)).astype(F)
        e = ((d / F(G)) * F(N)).astype(F)
    return g, e, ok


def march(volume, g, e, max_alpha, ok=None):
    """The entry and the walk for rays given in grid units: float32 [n, 4] (C_r, C_g, C_b, A); a miss is zeros."""
    vol = np.asarray(volume, np.uint8)
    N = vol.shape[0]
    assert vol.shape == (N, N, N, 4)
    g, e = np.asarray(g, F).reshape(-1, 3), np.asarray(e, F).reshape(-1, 3)
    n = g.shape[0]
    hit = np.ones(n, bool) if ok is None else np.asarray(ok, bool).copy()
    fN = F(N)
    nz = e != 0
    with np.errstate(all="ignore"):
        inv = np.where(nz, F(1) / np.where(nz, e, F(1)), F(0)).astype(F)
        t_in, t_out = np.zeros(n, F), np.full(n, INF, F)
        for a in range(3):
            t0, t1 = (F(0) - g[:, a]) * inv[:, a], (fN - g[:, a]) * inv[:, a]
            lo, hi = np.where(t1 < t0, t1, t0), np.where(t1 < t0, t0, t1)
            t_in = np.where(nz[:, a] & (lo > t_in), lo, t_in)
            t_out = np.where(nz[:, a] & (hi < t_out), hi, t_out)
            hit &= nz[:, a] | ((g[:, a] >= 0) & (g[:, a] < fN))
        hit &= t_in < t_out
        f = np.floor(g + t_in[:, None] * e)
        f = np.where(f > 0, f, F(0))
        f = np.where(f < fN - F(1), f, fN - F(1))
    c = f.astype(np.int64)
    plane = (e > 0).astype(np.int64)
    step = np.where(e > 0, 1, -1).astype(np.int64)
    C, A = np.zeros((n, 3), F), np.zeros(n, F)
    active = hit.copy()
    one255 = F(255)
    while active.any():
        i = np.nonzero(active)[0]
        ci = c[i]
        T = vol[ci[:, 2], ci[:, 1], ci[:, 0]].astype(F) / one255
        with np.errstate(all="ignore"):
            oma = F(1) - A[i]
            C[i] = C[i] + oma[:, None] * T[:, :3]
            A[i] = A[i] + oma * T[:, 3]
            go = ~(A[i] >= F(max_alpha))
            t = np.where(nz[i], ((ci + plane[i]).astype(F) - g[i]) * inv[i], INF).astype(F)
        axis = np.zeros(len(i), np.int64)
        tm = t[:, 0].copy()
        y = t[:, 1] < tm
        axis[y], tm[y] = 1, t[y, 1]
        axis[t[:, 2] < tm] = 2
        rows = np.arange(len(i))
        ci[rows, axis] += step[i][rows, axis]
        c[i] = ci
        go &= (ci[rows, axis] >= 0) & (ci[rows, axis] < N)
        active[i] = go
    return np.concatenate([C, A[:, None]], axis=1).astype(F)


def view(volume, m, w, h, G, max_alpha):
    """The frame of the view, float32 [h, w, 4] (row 0 = bottom row)."""
    N = np.asarray(volume).shape[0]
    g, e, ok = rays(m, w, h, G, N)
    return march(volume, g, e, max_alpha, ok).reshape(h, w, 4)


def half_bits(img):
    """float32 -> the uint16 bits of its round-to-nearest-even fp16 (the frame's rounding)."""
    with np.errstate(over="ignore"):
        return np.asarray(img, F).astype(np.float16).view(np.uint16)


def level_of(chain, V, level):
    """Level `level` of a linear chain (uint8 [texels, 4]) as [N, N, N, 4]."""
    off = sum((V >> l) ** 3 for l in range(level))
    N = V >> level
    return np.asarray(chain, np.uint8).reshape(-1, 4)[off:off + N ** 3].reshape(N, N, N, 4)
