"""The scenes, volumes and constants that tests/test_highprec_restatement.py (CPU, the oracle against
tests/highprec_ref.py) and tests/test_gpu_highprec.py (GPU, the kernels against it) share.  NumPy only."""
import numpy as np

import dyncases as dc
import dynemiscases
import synth

MS = dc.MS
# (tan_diffuse, max_distance, max_alpha): the defaults and two others
CONSTANTS = [(0.577, 75.0, 0.95), (0.4, 40.0, 0.7), (0.577, 111.0, 0.999)]
GRIDS_WORLD = [150.0, 100.0, 317.3]
# bounce cases (V, wrap_repeat, G, constants index): both grids x both wrap modes x the three constant sets at G = 150,
# and every other G once per wrap mode
BOUNCE_CASES = [(V, wrap, 150.0, c) for V in (16, 32) for wrap in (1, 0) for c in range(3)] + \
               [(V, wrap, G, 0) for V, wrap, G in ((16, 1, 100.0), (32, 0, 100.0), (32, 1, 317.3), (16, 0, 317.3))]
GPU_BOUNCE_CASES = [(V, wrap, 150.0, c) for V in (16, 32) for wrap in (1, 0) for c in range(3)] + [(32, 1, 317.3, 0)]


# the directional trace's third set: 1 - max_alpha < 2^-5 sends the march to its IEEE-divide kernels whatever the device's
# divisor check says (tests/test_gpu_march_params.py); 0.999 would do that too, but there 3 - 4 % of the frame's cones
# saturate within the alpha margin of the threshold, over the cap
TRACE_CONSTANTS = CONSTANTS[:2] + [(0.577, 111.0, 0.98)]


def constants_kw(c, table=None):
    td, md, ma = (table or CONSTANTS)[c]
    return dict(tan_diffuse=td, max_distance=md, max_alpha=ma)


def rescaled(mesh, G):
    """The mesh rescaled with the grid's world size so that it still fills the grid (as tools/fuzz_gpu.py does)."""
    pos, mat, alb = mesh
    return (pos.astype(np.float64) * (G / 150.0)).astype(np.float32), mat, alb


def shadow_for(G):
    """The raised shadow map of test_gpu_dynamic.shadow_maps(), its matrix seeing the rescaled world as before."""
    from test_gpu_dynamic import RAISED, shadow_maps
    depth, vp = shadow_maps()[RAISED]
    vp = vp.copy()
    vp[:, :3] /= np.float32(G / 150.0)
    return depth, vp


def static_mesh(G=150.0):
    return rescaled(dc.static_scene(), G)


EMISSION = dynemiscases.EM          # the mover's emission table in the bounce cases


def mover(G=150.0):
    return rescaled(dc.dynamic_mesh(dc.A), G)


# ---- volumes of the directional-mip cases ---------------------------------------------------------------------------
VOLUMES = ["noise", "random", "binary", "alphas"]


def volume(kind, V):
    r = np.random.default_rng(1000 + V)
    if kind == "noise":
        return synth.noise_volume(V, seed=3, occupancy=0.3)
    if kind == "random":
        return r.integers(0, 256, (V, V, V, 4), dtype=np.uint8)
    if kind == "binary":                                         # every level-1 parent is a tie or an integer
        return (r.integers(0, 2, (V, V, V, 4)) * 255).astype(np.uint8)
    vol = r.integers(0, 256, (V, V, V, 4), dtype=np.uint8)
    vol[..., 3] = r.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (V, V, V))
    return vol


# ---- frames of the directional trace --------------------------------------------------------------------------------
W, H = 24, 16
CAMERA = (10.0, 30.0, 60.0)


def frames():
    return {"random": synth.random_gbuffer(W * H, seed=11), "coherent": synth.coherent_gbuffer(W, H)}


# ---- known-answer blocks --------------------------------------------------------------------------------------------
A_COL, B_COL = (200, 40, 90, 255), (10, 250, 132, 255)


def split_block(axis, front, back):
    """A 2x2x2 block (z, y, x) whose lower half along `axis` (0 = x) is `front` and upper half `back`."""
    blk = np.zeros((2, 2, 2, 4), np.uint8)
    sl = [slice(None)] * 3
    sl[2 - axis] = 0
    blk[tuple(sl)] = front
    sl[2 - axis] = 1
    blk[tuple(sl)] = back
    return blk


def tiled(blk, V):
    return np.tile(blk, (V // 2, V // 2, V // 2, 1))


MEAN_AB = (105, 145, 111, 255)           # ((200 + 10) / 2, (40 + 250) / 2, (90 + 132) / 2, 255)
C_COL = (12, 248, 132, 255)


def known_blocks():
    """[(2x2x2 block, {direction: its level-1 texel, written out by hand})], direction = 2 * axis + (0: towards +axis)."""
    out = []
    for axis in range(3):
        # lower half A, upper half B, both opaque: towards +axis the lower half is met first and hides the other; the four
        # other chains see pairs of equal colours side by side: the mean
        out.append((split_block(axis, A_COL, B_COL),
                    {d: (A_COL if d % 2 == 0 else B_COL) if d // 2 == axis else MEAN_AB for d in range(6)}))
        # an empty front half: the back colour at a quarter per covered pair -- C / 4 = (3, 62, 33, 63.75); from the other
        # side C stands in front of nothing: the same
        for pairs, want in ((1, (3, 62, 33, 64)), (3, (9, 186, 99, 191)), (4, C_COL)):
            blk = split_block(axis, (0, 0, 0, 0), (0, 0, 0, 0))
            for i in [i for i in np.ndindex(2, 2, 2) if i[2 - axis] == 1][:pairs]:
                blk[i] = C_COL
            out.append((blk, {2 * axis: want, 2 * axis + 1: want}))
        # a front of alpha 128: F + (127 / 255) * B = (100 + 19.92, 60 + 99.61, 20 + 39.84, 128 + 127); from the other
        # side the opaque one hides it
        out.append((split_block(axis, (100, 60, 20, 128), (40, 200, 80, 255)),
                    {2 * axis: (120, 160, 60, 255), 2 * axis + 1: (40, 200, 80, 255)}))
    return out


# ---- known-answer triangles (model units; model_scale 0.05, G = 150, 16^3: one voxel = 187.5 model units) -----------
def tri_mesh(tris, albedo=((0.9, 0.5, 0.25, 1.0),), material=None):
    pos = np.asarray(tris, np.float32).reshape(-1, 9)
    mat = np.zeros(pos.shape[0], np.int32) if material is None else np.asarray(material, np.int32)
    return pos, mat, np.asarray(albedo, np.float32).reshape(-1, 4)


CCW_Z = [[-300.0, -200.0, 100.0], [400.0, -250.0, 100.0], [50.0, 350.0, 100.0]]      # counter-clockwise seen from +z
TILTED = [[0.0, 0.0, 0.0], [900.0, 0.0, 450.0], [0.0, 900.0, 240.0]]
# (triangle, the normal bytes written out by hand)
KNOWN_TRIANGLES = {
    "ccw_z": (CCW_Z, (128, 128, 255)),
    "cw_z": ([CCW_Z[0], CCW_Z[2], CCW_Z[1]], (128, 128, 1)),
    "plus_x": ([[100.0, -300.0, -200.0], [100.0, 400.0, -250.0], [100.0, 50.0, 350.0]], (255, 128, 128)),
    "minus_x": ([[100.0, -300.0, -200.0], [100.0, 50.0, 350.0], [100.0, 400.0, -250.0]], (1, 128, 128)),
    "plus_y": ([[-200.0, 100.0, -300.0], [-250.0, 100.0, 400.0], [350.0, 100.0, 50.0]], (128, 255, 128)),
    "minus_y": ([[-200.0, 100.0, -300.0], [350.0, 100.0, 50.0], [-250.0, 100.0, 400.0]], (128, 1, 128)),
    # cross((900,0,450), (0,900,240)) = (-405000, -216000, 810000) = 27000 * (-15, -8, 30), |(-15,-8,30)| = sqrt(1189) = 34.482;
    # n = (-.43500, -.23200, .87001); n * 127 = (-55.245, -29.464, 110.49) -> floor(. + .5) = (-55, -29, 110) -> + 128
    "tilted": (TILTED, (73, 99, 238)),
    # a component with n * 127 = k + 0.5 EXACTLY needs n = (2k + 1) / 254 rational with an even denominator in lowest
    # terms; a normal of integer (or any float32, i.e. dyadic) vertices has rational n only when |cross| is rational, and
    # then n = p / q in lowest terms with p^2 + r^2 + s^2 = q^2 -- q even forces p, r, s all even (squares mod 4), a
    # contradiction with lowest terms.  So no such triangle exists; the nearest case kept is 3-4-0: n = (.6, .8, 0),
    # n * 127 = (76.2, 101.6, 0) -> (76, 102, 0) -> (204, 230, 128)
    "three_four": ([[0.0, 0.0, -200.0], [-400.0, 300.0, -200.0], [0.0, 0.0, 200.0]], (204, 230, 128)),
}
