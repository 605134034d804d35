"""CPU: csrc/vct_tilediv.h without a GPU -- the multiply-high division of a tile index by tiles_x and the unit light vector
that vct_launch_trace hands the tile kernels -- in a stand-alone program with and without ASan + UBSan.

The division: vct_create accepts every positive int32 width, so tiles_x goes up to 2^28 and tile indices up to 2^31, which
cannot be enumerated.  The program therefore (tests/tilediv_check_main.cpp) covers every d in 1 .. 2048 over [0, d * 2048)
with all n of the first and last 4 d, 10^6 seeded n per d and both ends of every quotient's run -- the quotient is monotone
in n, so the ends settle the whole range -- and, over [0, 2^31), 2^28, the powers of two with their neighbours and 4000
seeded d above 2048 with the edges, seeded quotient ends and seeded n.  Every quotient is held to q d <= n < q d + d.

The light vector: the chain of trace.fs:179 restated in numpy float32 and compared bit for bit, NaN patterns included."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def build_check(tmp, sanitize):
    exe = os.path.join(str(tmp), "tilediv_check_san" if sanitize else "tilediv_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "tilediv_check_main.cpp")])
    return exe


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tilediv_check")
    return tmp, build_check(tmp, False), build_check(tmp, True)


def test_division_with_and_without_asan_ubsan(checkers):
    _, plain, san = checkers
    for exe in (plain, san):
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        m = re.search(r"tilediv_check ok \((\d+) quotients\)", out.stdout)
        assert m and int(m.group(1)) > 2048 * 10**6
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def light_vectors():
    r = np.random.default_rng(5)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 2.5, 0], [0, 0, -1e-3]], f32)
    named = np.array([[0, 1, 0.25], [3e-20, 4e-20, 0], [1e19, 1e19, 1e19], [1e20, -2e20, 3e19], [1e-20, 1e-20, 1e-20],
                      [0, 0, 0], [-0.0, 0.0, -0.0], [3, 4, 0], [1e-30, 0, 0], [np.inf, 1, 0], [np.nan, 1, 0]], f32)
    unit = r.normal(size=(20000, 3))
    unit = (unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(f32)
    scaled = (r.normal(size=(20000, 3)) * 10.0 ** r.uniform(-20, 20, size=(20000, 1))).astype(f32)
    return np.concatenate([axes, named, unit, scaled])


def light_unit_np(v):
    """normalize(LightDirection): l = sqrt((x*x + y*y) + z*z), then three divisions, every operation in float32."""
    v = v.astype(f32)
    with np.errstate(all="ignore"):
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        length = np.sqrt((x * x + y * y) + z * z)
        assert length.dtype == f32
        return v / length[:, None]


def test_light_unit_equals_the_numpy_chain_bit_for_bit(checkers):
    tmp, plain, san = checkers
    v = light_vectors()
    want = light_unit_np(v)
    assert want.dtype == f32
    paths = [os.path.join(str(tmp), name) for name in ("lights.bin", "unit.bin")]
    v.tofile(paths[0])
    for exe in (plain, san):
        subprocess.check_call([exe] + paths, timeout=120)
        got = np.fromfile(paths[1], f32).reshape(-1, 3)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # what the cases are there for
    named = {tuple(float(c) for c in row): want[i] for i, row in enumerate(v[:19])}
    assert np.isnan(named[(0.0, 0.0, 0.0)]).all()                                   # 0 / 0
    assert np.array_equal(named[(1.0, 0.0, 0.0)], np.array([1, 0, 0], f32))
    tiny = want[8 + 1]                 # (3e-20, 4e-20, 0): the squares are denormal, the length is not
    assert np.allclose(tiny, [0.6, 0.8, 0.0], rtol=1e-3)
    huge = want[8 + 2]                 # (1e19, 1e19, 1e19): the sum of squares is finite (3e38), just
    assert np.isfinite(huge).all() and np.allclose(huge, 3 ** -0.5, rtol=1e-6)
    assert (want[8 + 3] == 0).all()    # 1e20: the squares overflow, x / inf = 0 -- what the shader's normalize gives too


def test_header_is_free_of_hip_calls_and_the_kernels_use_it():
    hdr = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "csrc", "vct_tilediv.h")).read()
    assert "hip/" not in hdr and not re.search(r"\bhip[A-Z]\w*\(", hdr)
    src = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "csrc", "vct_trace.hip")).read()
    assert "vct_tilediv_make(" in src and "vct_light_unit(" in src
    kernels = src[src.index("k_trace_tile(const VctTraceParams p)"):src.index("Half-rate diffuse gather (include/vct.h")]
    assert "/ p.tiles_x" not in kernels and "p.light[" not in kernels
