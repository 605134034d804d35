"""Expected values of the emissive materials (include/vct.h "emissive materials"), from the CPU oracle as it is.  Test
infrastructure, NumPy only.

Level 0: L is oracle.voxelize_conservative of the scene as it is (shadow map and textures included); Em is
oracle.voxelize_conservative of the same triangles with the emission table as the colour table, no shadow map, no
texture coordinates and no textures; rgb = min(255, L + Em) per byte, alpha is L's.  Frame: the composite of
tests/components_ref.py plus E, one fp32 add per channel, for the pixels that are not discarded."""
import numpy as np

import components_ref

f32 = np.float32

# the inputs of the level-0 tests: two emissive materials of voxcases.random_scene's five, one with a channel above 1
EMISSION = np.array([[0.0, 0.0, 0.0], [0.9, 0.35, 0.1], [0.0, 0.0, 0.0], [0.25, 2.0, 0.6], [0.0, 0.0, 0.0]], f32)


def pad4(em):
    """[nmat, 3] -> the [nmat, 4] colour table make_scene takes (the fourth column is not read by the voxelizer)."""
    em = np.ascontiguousarray(em, f32).reshape(-1, 3)
    return np.concatenate([em, np.ones((em.shape[0], 1), f32)], 1)


def level0(oracle, p, pos, mat, alb, em, ms=0.05, **scene_kw):
    """(expected level 0, L, Em), uint8 [V, V, V, 4] each.  scene_kw: what make_scene takes for the lit scene
    (shadow_depth, light_vp, uv, mat_tex, textures, mipmaps)."""
    L = oracle.voxelize_conservative(p, oracle.make_scene(pos, mat, alb, ms, **scene_kw))
    Em = oracle.voxelize_conservative(p, oracle.make_scene(pos, mat, pad4(em), ms))
    out = L.copy()
    out[..., :3] = np.minimum(255, L[..., :3].astype(np.int32) + Em[..., :3].astype(np.int32)).astype(np.uint8)
    return out, L, Em


def non_degeneracy(L, Em, em):
    """Counts that keep a level-0 comparison from passing vacuously."""
    lit = L[..., 3] > 0
    s = L[..., :3].astype(np.int32) + Em[..., :3].astype(np.int32)
    consts = {tuple(int(v) for v in np.floor(np.minimum(np.asarray(e, np.float64), 1.0) * 255.0 + 0.5)) for e in em}
    values = {tuple(int(v) for v in t) for t in np.unique(Em[lit][:, :3], axis=0)}
    return dict(saturating=int((s > 255).any(-1).sum()),
                both=int(((L[..., :3] > 0).any(-1) & (Em[..., :3] > 0).any(-1)).sum()),
                mixed_values=len(values - consts - {(0, 0, 0)}),
                same_alpha=bool(np.array_equal(L[..., 3], Em[..., 3])))


def pixel_emission(planes, albedo, em):
    """E [3, npix] for a flat-material scene whose materials have pairwise different albedo: the visible material of a
    pixel is the one whose albedo equals planes 15-18 exactly; 0 where the oracle has no surface."""
    albedo = np.ascontiguousarray(albedo, f32).reshape(-1, 4)
    em = np.ascontiguousarray(em, f32).reshape(-1, 3)
    assert len({tuple(a) for a in albedo.view(np.uint32).tolist()}) == albedo.shape[0], "albedos must differ pairwise"
    E = np.zeros((3, planes.shape[1]), f32)
    covered = (planes[15:19].view(np.uint32) != 0).any(0)
    seen = np.zeros(planes.shape[1], bool)
    for m in range(albedo.shape[0]):
        hit = (planes[15:19].view(np.uint32) == albedo[m].view(np.uint32)[:, None]).all(0) & covered
        E[:, hit] = em[m][:, None]
        seen |= hit
    assert np.array_equal(seen, covered), "a covered pixel shows no material's albedo"
    return E


def frame(rgba32f, planes, E):
    """The frame with pixel emission as fp16 bits [npix, 4]: rgb + E in fp32 (one add per channel) for the pixels that are
    not discarded, from the composite without emission (components_ref.composite / diffuse_rate_ref.restate: rgba32f)."""
    rgba = np.array(rgba32f, f32, copy=True)
    live = ~(np.asarray(planes, f32)[18] < f32(0.5))
    E = np.ascontiguousarray(E, f32).reshape(3, -1)
    with np.errstate(all="ignore"):
        rgba[live, :3] = (rgba[live, :3] + E[:, live].T).astype(f32)
    return components_ref.to_f16_bits(rgba)


# ---- a closed room lit by nothing but an emissive panel ---------------------------------------------------------------
def _quad(corners, normal):
    """Two triangles of a quad wound counter-clockwise as seen from the side `normal` points to: ([2, 9] positions, normal)."""
    a, b, c, d = (np.asarray(v, np.float64) for v in corners)
    n = np.asarray(normal, np.float64)
    if np.dot(np.cross(b - a, c - a), n) < 0:
        b, d = d, b
    return np.array([np.concatenate([a, b, c]), np.concatenate([a, c, d])]), n


class Room:
    """Model units (model_scale 0.05, grid 150): a box x, z in [-1000, 1000], y in [-1000, 200] seen from inside; a panel
    under its ceiling (material 2, the only emitter) over both halves of the floor; a plate at y = -600 over the half x < 0
    of the floor (material 3), seen from below.  Flat materials with pairwise different albedo; every face looks inward."""
    albedo = np.array([[0.7, 0.7, 0.7, 1.0], [0.6, 0.5, 0.4, 1.0], [0.9, 0.9, 0.8, 1.0], [0.3, 0.3, 0.5, 1.0]], f32)
    specular = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.0, 0.0, 0.0], [0.3, 0.3, 0.3]], f32)
    emission = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [2.0, 0.9, 0.6], [0.0, 0.0, 0.0]], f32)
    PANEL, FLOOR, PLATE = 2, 1, 3
    camera = dict(position=(0.0, -42.0, 45.0), yaw=-90.0, pitch=10.0)      # world units, below the plate, looking along -z

    def __init__(self):
        lo, hi, top = -1000.0, 1000.0, 200.0
        faces = [
            (([lo, lo, lo], [hi, lo, lo], [hi, lo, hi], [lo, lo, hi]), (0, 1, 0), 1),            # floor
            (([lo, top, lo], [hi, top, lo], [hi, top, hi], [lo, top, hi]), (0, -1, 0), 0),       # ceiling
            (([lo, lo, lo], [lo, top, lo], [lo, top, hi], [lo, lo, hi]), (1, 0, 0), 0),
            (([hi, lo, lo], [hi, top, lo], [hi, top, hi], [hi, lo, hi]), (-1, 0, 0), 0),
            (([lo, lo, lo], [hi, lo, lo], [hi, top, lo], [lo, top, lo]), (0, 0, 1), 0),
            (([lo, lo, hi], [hi, lo, hi], [hi, top, hi], [lo, top, hi]), (0, 0, -1), 0),
            (([-600.0, 80.0, -950.0], [600.0, 80.0, -950.0], [600.0, 80.0, -400.0], [-600.0, 80.0, -400.0]), (0, -1, 0), 2),
            (([lo, -600.0, lo], [0.0, -600.0, lo], [0.0, -600.0, hi], [lo, -600.0, hi]), (0, -1, 0), 3),
        ]
        pos, nrm, tan, bit, mat = [], [], [], [], []
        for corners, n, m in faces:
            p, n = _quad(corners, n)
            t = np.array([n[1], n[2], n[0]], np.float64)          # axis-aligned normals: a cyclic shift is orthogonal
            b = np.cross(n, t)
            for tri in p:
                pos.append(tri); mat.append(m)
                nrm.append(np.tile(n, 3)); tan.append(np.tile(t, 3)); bit.append(np.tile(b, 3))
        self.pos = np.asarray(pos, f32)
        self.material = np.asarray(mat, np.int32)
        self._frames = [np.asarray(a, f32) for a in (nrm, tan, bit)]
        self.uv = np.zeros((self.pos.shape[0], 6), f32)
        self.mat_tex = np.full((4, 3), -1, np.int32)
        self.textures = []
        self.ntri, self.nmat = self.pos.shape[0], 4

    def frames(self):
        return self._frames
