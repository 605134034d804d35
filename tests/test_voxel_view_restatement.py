"""The numpy restatement of the voxel view (tests/voxel_view_ref.py) against cases worked out by hand (include/vct.h
"voxel view").  CPU only."""
import numpy as np

import voxel_view_ref as vv

F = np.float32


def _vol(N):
    return np.zeros((N, N, N, 4), np.uint8)       # [z, y, x]


def test_axis_aligned_rays_through_4_cubed():
    """An orthographic matrix whose rays run along +z through the cell centres of a 4^3 grid (G = 4, frame 4 x 4):
    pixel (x, y) visits the cells (x, y, 0 .. 3) in that order."""
    N, G = 4, 4.0
    m = np.zeros(16, F)
    m[0], m[5], m[10], m[15] = 2.0, 2.0, 4.0, 1.0        # point = (2 nx, 2 ny, 4 nz), w = 1
    g, e, ok = vv.rays(m, 4, 4, G, N)
    assert ok.all()
    # nx = -.75, -.25, .25, .75 -> o = 2 nx -> g = o + 2 = .5, 1.5, 2.5, 3.5; z: o = -4 -> g = -2, e = (8 / 4) 4 = 8
    assert np.array_equal(g.reshape(4, 4, 3)[2, 1], np.array([1.5, 2.5, -2.0], F))
    assert np.array_equal(e.reshape(4, 4, 3)[2, 1], np.array([0.0, 0.0, 8.0], F))
    vol = _vol(N)
    vol[1, 2, 1] = (255, 0, 0, 128)          # cell (x 1, y 2, z 1): red, half transparent
    vol[3, 2, 1] = (0, 255, 0, 255)          # behind it: green, opaque
    vol[0, 0, 0] = (0, 0, 255, 255)          # pixel (0, 0): an opaque blue cell in front ...
    vol[2, 0, 0] = (255, 255, 255, 255)      # ... hides the white one
    vol[2, 3, 3] = (9, 0, 0, 0)              # alpha 0, colour != 0: still adds its colour
    out = vv.view(vol, m, 4, 4, G, 0.95)
    a = F(128) / F(255)
    oma = F(1) - a
    assert np.array_equal(out[2, 1], np.array([F(1), oma * F(1), F(0), a + oma * F(1)], F))
    assert np.array_equal(out[0, 0], np.array([0, 0, 1, 1], F))
    assert np.array_equal(out[3, 3], np.array([F(9) / F(255), 0, 0, 0], F))
    rest = np.ones((4, 4), bool)
    rest[2, 1] = rest[0, 0] = rest[3, 3] = False
    assert (out[rest] == 0).all()                         # hits of empty columns: (0, 0, 0, 0)


def test_tie_steps_x_before_y_and_start_inside():
    """g = (.5, .5, .5), e = (1, 1, 0): the start is inside the grid (t_in = 0, cell (0, 0, 0)) and every x plane ties
    with a y plane (t = .5, 1.5, ...): x goes first, so (1, 0, 0) is visited and (0, 1, 0) never is."""
    vol = _vol(4)
    vol[0, 0, 1] = (255, 0, 0, 0)            # (x 1, y 0): on the path
    vol[0, 1, 0] = (0, 255, 0, 0)            # (x 0, y 1): not on it
    vol[0, 1, 1] = (0, 0, 51, 0)             # (1, 1): after the y step
    vol[0, 3, 3] = (0, 0, 102, 0)            # (3, 3): the last cell before the walk leaves through x = 4
    out = vv.march(vol, [[0.5, 0.5, 0.5]], [[1.0, 1.0, 0.0]], 0.95)
    assert np.array_equal(out[0], np.array([F(1), F(0), F(51) / F(255) + F(102) / F(255), F(0)], F))
    # a start inside, walking -z from cell (1, 2, 3): cells z = 3, 2, 1, 0
    vol = _vol(4)
    vol[3, 2, 1] = (10, 0, 0, 0)
    vol[0, 2, 1] = (0, 20, 0, 255)
    vol[1, 2, 2] = (0, 0, 99, 255)           # a neighbouring column
    out = vv.march(vol, [[1.5, 2.5, 3.25]], [[0.0, 0.0, -2.0]], 0.95)
    assert np.array_equal(out[0], np.array([F(10) / F(255), F(20) / F(255), 0, 1], F))


def test_misses():
    vol = np.full((4, 4, 4, 4), 255, np.uint8)
    g = [[-1.0, 0.5, 0.5],       # e_x = 0 with g_x outside [0, N)
         [-1.0, -1.0, 0.5],      # x enters at t = 1, y leaves at t = -1: t_in >= t_out
         [0.5, 0.5, 0.5]]        # inside, but flagged as a non-finite ray
    e = [[0.0, 1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 0.0, 0.0]]
    out = vv.march(vol, g, e, 0.95, ok=[True, True, False])
    assert (out == 0).all()
    # through the matrix: every ray of a camera whose far points coincide with its near points has d = 0
    m = np.zeros(16, F)
    m[0], m[5], m[14], m[15] = 1.0, 1.0, 1.0, 1.0          # point = (nx, ny, 1): independent of nz
    g, e, ok = vv.rays(m, 3, 2, 4.0, 4)
    assert not ok.any()
    assert (vv.view(vol, m, 3, 2, 4.0, 0.95) == 0).all()
    # and a non-finite point (r_w = 0)
    m[15] = 0.0
    assert not vv.rays(m, 3, 2, 4.0, 4)[2].any()


def test_half_bits_round_to_nearest_even():
    assert vv.half_bits(np.array([1.0, 0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], F)).tolist() == [0x3c00, 0, 0x3c00, 0x3c02]
