"""Meshes for the voxelizer's decision points (csrc/vct_voxelize.hip), beside test_gpu_parity.random_scene.  Test
infrastructure, NumPy only.  Every builder returns (pos [n,9] f32 model space, material, albedo, model_scale, G, V).

Two unit systems: the default (model_scale 0.05, grid_world_size 150: one voxel of a 32^3 grid is 93.75 model units,
the outer faces are at +-1500) and an exact one (model_scale 1/16, grid_world_size 128, V = 32: one voxel is 64 model
units, the outer faces at +-1024, and every fp32 operation from the vertex to its voxel coordinate is exact, so a
vertex sits exactly ON a voxel face)."""
import numpy as np

DEFAULT = (0.05, 150.0, 32)
EXACT = (0.0625, 128.0, 32)


def random_scene(ntri, seed, big=2):
    """The scene of test_gpu_parity.random_scene (small triangles, a few large, a point, an axis-aligned wall)."""
    r = np.random.default_rng(seed)
    c = r.uniform(-1300, 1300, (ntri, 1, 3))
    pos = c + r.normal(scale=25.0, size=(ntri, 3, 3))
    big = min(big, max(ntri - 2, 0))
    pos[:big] = c[:big] + r.normal(scale=400.0, size=(big, 3, 3))
    if ntri > big + 1:
        pos[big] = pos[big, 0][None, :]
        pos[big + 1] = [[-1000, -1000, 200], [1000, -1000, 200], [1000, 1000, 200]]
    mat = r.integers(0, 5, ntri).astype(np.int32)
    alb = r.uniform(0.1, 1.0, (5, 4)).astype(np.float32)
    return pos.astype(np.float32).reshape(-1, 9), mat, alb


def _mesh(tris, seed=0):
    pos = np.asarray(tris, np.float64).reshape(-1, 9).astype(np.float32)
    r = np.random.default_rng(seed)
    mat = (np.arange(pos.shape[0]) % 5).astype(np.int32)
    alb = r.uniform(0.1, 1.0, (5, 4)).astype(np.float32)
    return pos, mat, alb


def _voxel_coords(pos, ms, G, V):
    w = pos.reshape(-1, 3).astype(np.float32) * np.float32(ms)
    return ((w.astype(np.float64) / G) + 0.5) * V


def outside_each_side():
    """Six triangles entirely beyond one face each (near it, and far away), beside a few inside."""
    ms, G, V = DEFAULT
    H = 0.5 * G / ms
    tris = []
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            for dist in (1.02, 40.0):
                t = np.array([[-200.0, -150.0, 0.0], [250.0, -100.0, 0.0], [0.0, 300.0, 0.0]])
                t = np.roll(t, axis, 1)
                t[:, axis] = sgn * (H * dist + np.array([0.0, 20.0, 45.0]))
                tris.append(t)
    inside = random_scene(20, 5)[0].reshape(-1, 3, 3)
    pos, mat, alb = _mesh(np.concatenate([np.array(tris), inside]))
    g = _voxel_coords(pos, ms, G, V).reshape(-1, 3, 3)
    out = ((g < 0).all(1) | (g > V).all(1)).any(1)
    assert out[:12].all() and out.sum() >= 12
    return pos, mat, alb, ms, G, V


def straddling_each_face():
    """Triangles that cross each of the six outer faces, two of them an edge and a corner of the grid."""
    ms, G, V = DEFAULT
    H = 0.5 * G / ms
    tris = []
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            t = np.array([[-300.0, -250.0, 0.0], [350.0, -200.0, 0.0], [40.0, 400.0, 0.0]])
            t = np.roll(t, axis, 1)
            t[:, axis] = sgn * (H + np.array([-260.0, 30.0, 310.0]))
            tris.append(t)
    tris.append(np.array([[H - 100, H - 120, 0.0], [H + 200, H - 50, 50.0], [H - 60, H + 220, -40.0]]))       # an edge
    tris.append(np.array([[H - 90, H - 90, H - 90], [H + 300, H + 10, H - 20], [H - 10, H + 280, H + 150]]))  # a corner
    pos, mat, alb = _mesh(tris)
    g = _voxel_coords(pos, ms, G, V).reshape(-1, 3, 3)
    crosses = (((g < 0).any(1) & (g >= 0).any(1)) | ((g > V).any(1) & (g <= V).any(1))).any(1)
    assert crosses.all()
    return pos, mat, alb, ms, G, V


def on_voxel_faces():
    """Exact units: vertices exactly on voxel faces, inner and the outer ones at +-G/2; axis-aligned triangles lying IN
    a face plane, diagonal ones through voxel corners."""
    ms, G, V = EXACT
    s = 64.0                                            # one voxel in model units
    H = 16 * s
    tris = [
        [[-H, -H, 0.0], [H, -H, 0.0], [H, H, 0.0]],                      # in the plane between two voxel layers, corner to corner
        [[-H, -H, -H], [H, -H, -H], [H, H, -H]],                         # in the outer face z = -G/2
        [[-H, -H, H], [H, H, H], [-H, H, H]],                            # in the outer face z = +G/2 (the first voxel outside)
        [[H, -4 * s, -4 * s], [H, 4 * s, -4 * s], [H, 4 * s, 4 * s]],    # in x = +G/2
        [[-H, -4 * s, -4 * s], [-H, 4 * s, 4 * s], [-H, 4 * s, -4 * s]], # in x = -G/2
        [[2 * s, 3 * s, 5 * s], [6 * s, 3 * s, 5 * s], [2 * s, 7 * s, 9 * s]],     # every vertex on a voxel corner, tilted
        [[-8 * s, -8 * s, -8 * s], [8 * s, 8 * s, 8 * s], [8 * s, -8 * s, 0.0]],   # through the grid's centre along a diagonal
        [[3 * s, 0.0, 0.0], [3 * s, 5 * s, 0.0], [3 * s, 0.0, 5 * s]],   # in an inner face x = const
        [[0.0, -H, 2 * s], [5 * s, -H, 2 * s], [0.0, -H, 6 * s]],        # in y = -G/2
        [[0.0, H, 2 * s], [0.0, H, 6 * s], [5 * s, H, 2 * s]],           # in y = +G/2
    ]
    pos, mat, alb = _mesh(tris)
    g = _voxel_coords(pos, ms, G, V)
    assert (g == np.round(g)).all() and (g == 0).sum() >= 8 and (g == V).sum() >= 8
    return pos, mat, alb, ms, G, V


def degenerate_triangles():
    """Points and collinear triangles (exact units, so collinear stays collinear after scaling), beside ordinary ones."""
    ms, G, V = EXACT
    s = 64.0
    tris = []
    for i in range(6):
        p = [(-7 + 2.5 * i) * s, (3 - i) * s + 7.0, (i - 2.25) * s]
        tris.append([p, p, p])                                                                # point
        d = np.array([(1 + i) * 16.0, (3 - i) * 8.0, 24.0])
        tris.append([p, list(np.array(p) + d), list(np.array(p) + 4 * d)])                    # collinear
        tris.append([p, list(np.array(p) + d), p])                                            # two vertices equal
    tris.append([[-5 * s, -5 * s, 1.0], [6 * s, -4 * s, 9.0], [0.0, 7 * s, 30.0]])
    pos, mat, alb = _mesh(tris)
    return pos, mat, alb, ms, G, V


def inside_one_voxel():
    ms, G, V = DEFAULT
    tris = [[[10.0, 12.0, 14.0], [40.0, 15.0, 20.0], [20.0, 50.0, 33.0]]]                     # voxel (16,16,16): 0..93.75
    pos, mat, alb = _mesh(tris)
    g = np.floor(_voxel_coords(pos, ms, G, V))
    assert (g == g[0]).all()
    return pos, mat, alb, ms, G, V


def one_triangle():
    ms, G, V = DEFAULT
    pos, mat, alb = _mesh([[[-900.0, -700.0, -300.0], [1000.0, -500.0, 100.0], [-100.0, 1100.0, 600.0]]])
    return pos, mat, alb, ms, G, V


def whole_grid_and_a_crowded_brick(ntri=8000, seed=5):
    """One triangle spanning the whole grid and far beyond, and thousands of small ones crowded into a few bricks (a
    brick slot above 4096 fragments is cut into chunks)."""
    ms, G, V = DEFAULT
    r = np.random.default_rng(seed)
    c = np.array([[[-300.0, 150.0, 420.0]]]) + r.normal(scale=60.0, size=(ntri, 1, 3))
    small = c + r.normal(scale=70.0, size=(ntri, 3, 3))
    huge = np.array([[[-9000.0, -7000.0, -100.0], [9500.0, -6000.0, 200.0], [-500.0, 11000.0, 350.0]]])
    pos = np.concatenate([huge, small]).astype(np.float32).reshape(-1, 9)
    mat = r.integers(0, 5, ntri + 1).astype(np.int32)
    alb = r.uniform(0.1, 1.0, (5, 4)).astype(np.float32)
    return pos, mat, alb, ms, G, V


def counted(n):
    pos, mat, alb = random_scene(n, seed=100 + n)
    return (pos, mat, alb) + DEFAULT


EDGE_CASES = {
    "outside_each_side": outside_each_side, "straddling_each_face": straddling_each_face,
    "on_voxel_faces": on_voxel_faces, "degenerate_triangles": degenerate_triangles,
    "inside_one_voxel": inside_one_voxel, "one_triangle": one_triangle,
    "whole_grid_and_a_crowded_brick": whole_grid_and_a_crowded_brick,
    "count_63": lambda: counted(63), "count_65": lambda: counted(65),
    "count_255": lambda: counted(255), "count_257": lambda: counted(257),
}


def rescale(pos, model_scale, G):
    """A default-units mesh rescaled so that it fills a grid of G at model_scale as it fills 150 at 0.05."""
    return (np.asarray(pos, np.float64) * (0.05 / model_scale) * (G / 150.0)).astype(np.float32)


def at_the_bound(model_scale, G, inside=True):
    """The largest fp32 vertex value whose fp32 product with model_scale is still <= 2^20 * G (inside), or the
    smallest one whose product exceeds it."""
    ms, lim = np.float32(model_scale), np.float32(2.0 ** 20) * np.float32(G)
    v = np.float32(lim / ms)
    while v * ms <= lim:
        v = np.nextafter(v, np.float32(np.inf))
    # v: the first value beyond
    if not inside:
        return v
    while v * ms > lim:
        v = np.nextafter(v, np.float32(0))
    return v
