"""The reference of per-material gloss (include/vct.h "per-material gloss"), formed from the CPU oracle as it is.

Pixels are independent in the oracle, so the frame the oracle gives with class k's tan_specular and shininess, read at the
pixels of class k, is exact: trace() runs pyoracle.trace once per class and takes frame, cones and steps per pixel from the
run of the pixel's clamped class; the total step count is the sum over the pixels.  Test infrastructure: NumPy + the oracle,
no GPU."""

import numpy as np

CLASSES_MAX = 8
# the classes the tests use: the three BASELINE apertures, a long table and a short one
CLASSES = ((0.07, 20.0), (0.105, 8.0), (0.2, 4.0), (0.02, 64.0), (1.0, 1.0))


def clamp_class(plane, nclasses):
    """The class a byte of the pixel-gloss plane means: b < nclasses ? b : 0."""
    b = np.asarray(plane).astype(np.int64)
    return np.where(b < nclasses, b, 0)


def class_params(p, cls):
    """A copy of the oracle parameters `p` with one class's tan_specular and shininess."""
    q = type(p).from_buffer_copy(p)
    q.tan_specular, q.shininess = float(cls[0]), float(cls[1])
    return q


def class_runs(oracle, p, chain, planes, classes, nthreads=4):
    """pyoracle.trace(..., want_cones=True) once per class, in class order."""
    return [oracle.trace(class_params(p, c), chain, planes, nthreads=nthreads, want_cones=True) for c in classes]


def select(runs, plane, classes):
    """Per pixel the outputs of the run of its clamped class; total_steps is the sum of the selected steps."""
    k = clamp_class(plane, len(classes))
    out = {}
    for key in ("rgba32f", "rgba16f", "steps", "cones"):
        stack = np.stack([r[key] for r in runs])              # [nclasses, npix, ...]
        out[key] = stack[k, np.arange(k.shape[0])]
    out["total_steps"] = int(out["steps"].astype(np.int64).sum())
    out["cls"] = k
    return out


def trace(oracle, p, chain, planes, classes, plane, nthreads=4):
    return select(class_runs(oracle, p, chain, planes, classes, nthreads), plane, classes)


def checkerboard(w, h, nclasses, in_frame_extra=None):
    """Class (x + 2 y) % nclasses per pixel: every 8 x 8 tile of the frame holds every class (nclasses <= 8).  A few
    in-frame bytes are replaced by in_frame_extra (a value >= nclasses: read as class 0)."""
    y, x = np.divmod(np.arange(w * h), w)
    plane = ((x + 2 * y) % nclasses).astype(np.uint8)
    if in_frame_extra is not None:
        plane[(x * 7 + y * 3) % 11 == 0] = in_frame_extra
    return plane


def to_tiled(plane, w, h, pad=0):
    """linear [h*w] -> tiled [tiles, 64] with the lanes outside a ragged frame set to `pad`."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    img = np.full((ty * 8, tx * 8), pad, np.uint8)
    img[:h, :w] = np.asarray(plane, np.uint8).reshape(h, w)
    return np.ascontiguousarray(img.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64))


def pixel_class(planes, albedo, mat_class):
    """The pixel-gloss plane a G-buffer pass writes for a flat-material scene whose materials have pairwise different
    albedo: mat_class[material whose albedo equals planes 15-18 exactly] where the raster oracle has a surface, 0 where
    it has none."""
    albedo = np.ascontiguousarray(albedo, np.float32).reshape(-1, 4)
    assert len({tuple(a) for a in albedo.view(np.uint32).tolist()}) == albedo.shape[0], "albedos must differ pairwise"
    out = np.zeros(planes.shape[1], np.uint8)
    covered = (planes[15:19].view(np.uint32) != 0).any(0)
    seen = np.zeros(planes.shape[1], bool)
    for m in range(albedo.shape[0]):
        hit = (planes[15:19].view(np.uint32) == albedo[m].view(np.uint32)[:, None]).all(0) & covered
        out[hit] = mat_class[m]
        seen |= hit
    assert np.array_equal(seen, covered), "a covered pixel shows no material's albedo"
    return out
