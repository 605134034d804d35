"""CPU: the local lights of include/vct.h ("local lights") without a GPU -- that the restatement of tests/lights_ref.py is
not degenerate on the inputs the GPU tests use (every count below is asserted, so a change of lights_ref.LIGHTS that
empties one of them fails here), that skipping out-of-range lights keeps the bits and that the order of the lights is
part of the definition, the voxel kernel's brick cull restated and held against the per-voxel range test, the header
against the binding, and the table check and the folding of vct_set_lights in a stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lights_ref as lr
import voxcases
from test_gpu_parity import light_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, G = 32, 150.0


@pytest.fixture(scope="module")
def scene(oracle):
    pos, mat, alb = voxcases.random_scene(300, 7)
    depth, vp = light_setup(64, 3)
    sc = oracle.make_scene(pos, mat, alb, shadow_depth=depth, light_vp=vp)
    l0, aa, an = oracle.voxelize_conservative_attr(oracle.default_params(V), sc)
    out, info = lr.level0(l0, aa, an, lr.LIGHTS, G, want_info=True)
    return dict(l0=l0, aa=aa, an=an, out=out, info=info)


def test_light_set():
    assert len(lr.LIGHTS) == 4 and sum(1 for l in lr.LIGHTS if l.get("flags", 0) & lr.SPOT) == 2
    for l in lr.LIGHTS:
        assert all(abs(c) < G / 2 for c in l["position"])            # inside the grid


def test_random_scene_expectation_is_not_degenerate(scene):
    s, info = scene, scene["info"]
    occ, l0, out = info["occ"], s["l0"], s["out"]
    assert np.array_equal(occ, l0[..., 3] == 255)                    # the attributes cover level 0's voxels
    assert np.array_equal(out[~occ], l0[~occ]) and np.array_equal(out[..., 3], l0[..., 3])
    changed = (out != l0).any(-1)
    assert changed.sum() >= 200, changed.sum()
    saturating = ((out[..., :3] == 255) & (l0[..., :3] != 255)).any(-1)
    assert saturating.sum() >= 20, saturating.sum()
    gated = np.zeros_like(occ)
    for li in info["lights"]:
        gated |= occ & li["inside"] & (li["nl"] == 0)
    assert gated.sum() >= 20, gated.sum()
    # brick slots (bricks with an occupied voxel) against the kernel's cull
    slots = lr.per_brick(occ)
    reached = lr.brick_cull(lr.LIGHTS, V, G).sum(-1)
    assert (slots & (reached == 0)).sum() >= 1 and (slots & (reached >= 2)).sum() >= 1
    # each spot shows all three parts of its cone on occupied voxels in range
    for j, l in enumerate(lr.LIGHTS):
        if not l.get("flags", 0) & lr.SPOT:
            continue
        li = info["lights"][j]
        m = occ & li["inside"]
        assert (m & (li["t"] == 0)).any() and (m & (li["t"] > 0) & (li["t"] < 1)).any() and (m & (li["t"] == 1)).any(), j


def test_brick_cull_never_drops_a_light_in_range(scene):
    """The cull's r2_min is a lower bound of r2 over EVERY voxel of the brick (occupied or not): a culled brick has no
    voxel in range.  Held for the test lights, the 64 of the many-light case and lights on and beyond the grid's faces."""
    P, _, _ = lr.voxel_inputs(scene["aa"], scene["an"], G)
    r = np.random.default_rng(2)
    extra = [lr.point(r.uniform(-90.0, 90.0, 3), (1.0, 1.0, 1.0), float(r.uniform(1.0, 60.0)), 1.0) for _ in range(40)]
    extra += [lr.point((75.0, -75.0, 0.0), (1.0, 1.0, 1.0), 9.5, 1.0), lr.point((-72.65625, 2.34375, 2.34375), (1.0, 1.0, 1.0), 4.6875, 1.0)]
    lights = lr.LIGHTS + lr.many_lights() + extra
    cull = lr.brick_cull(lights, V, G)
    culled_some = 0
    for j, light in enumerate(lights):
        inside = lr.term(lr.fold(light), P)[0]
        assert not (lr.per_brick(inside) & ~cull[..., j]).any(), j
        culled_some += int((~cull[..., j]).any())
    assert culled_some >= len(lights) // 2


def test_a_light_on_a_voxel_centre_leaves_it_finite(scene):
    occ = scene["info"]["occ"]
    z, y, x = (int(v) for v in np.argwhere(occ)[len(np.argwhere(occ)) // 2])
    c = lr.voxel_centres(V, G)
    on = lr.point((float(c[x]), float(c[y]), float(c[z])), (50.0, 50.0, 50.0), 20.0, 1.0)
    out, info = lr.level0(scene["l0"], scene["aa"], scene["an"], [on], G, want_info=True)
    assert info["lights"][0]["r2"][z, y, x] == 0 and info["lights"][0]["inside"][z, y, x]
    assert all(np.isfinite(d[z, y, x]) and d[z, y, x] == 0 for d in info["D"])       # l is NaN, nl = fmaxf(NaN, 0) = 0
    assert np.array_equal(out[z, y, x], scene["l0"][z, y, x])
    assert all(np.isfinite(d[occ]).all() for d in info["D"])
    assert (out != scene["l0"]).any()                                # its neighbours are lit


def test_skipping_out_of_range_lights_keeps_the_bits(scene):
    """Per voxel: the sum over only the lights whose `in` is true there equals the sum over all, bit for bit -- what lets
    the kernels skip a light for a whole brick or tile.  Restated per subset of lights (2^4 subsets)."""
    P, n, occ = lr.voxel_inputs(scene["aa"], scene["an"], G)
    full, info = lr.diffuse_sum(lr.LIGHTS, P, n)
    inside = np.stack([li["inside"] for li in info], -1)
    seen = np.zeros_like(occ)
    for subset in range(16):
        keep = [j for j in range(4) if subset >> j & 1]
        where = (inside == np.array([j in keep for j in range(4)])).all(-1)      # exactly these lights are in range
        part, _ = lr.diffuse_sum([lr.LIGHTS[j] for j in keep], P, n)
        for c in range(3):
            assert np.array_equal(part[c][where].view(np.uint32), full[c][where].view(np.uint32)), (subset, c)
        seen |= where
    assert seen.all()


def test_the_order_of_the_lights_is_part_of_the_definition(scene):
    P, n, occ = lr.voxel_inputs(scene["aa"], scene["an"], G)
    a, _ = lr.diffuse_sum(lr.LIGHTS, P, n)
    b, _ = lr.diffuse_sum(lr.LIGHTS[::-1], P, n)
    differ = sum(int((a[c][occ].view(np.uint32) != b[c][occ].view(np.uint32)).sum()) for c in range(3))
    assert differ >= 1


def test_many_lights_case_is_not_degenerate(scene):
    """64 lights: light 0 is the only one in range of some brick slot, and most slots see only a few of the 64."""
    lights = lr.many_lights()
    assert len(lights) == lr.LIGHTS_MAX
    occ = scene["info"]["occ"]
    cull = lr.brick_cull(lights, V, G)
    slots = lr.per_brick(occ)
    only0 = slots & cull[..., 0] & (cull.sum(-1) == 1)
    assert only0.sum() >= 1
    assert (cull[slots].sum(-1) >= 3).any() and cull[..., 1:].any(axis=(0, 1, 2)).sum() >= 40
    out = lr.level0(scene["l0"], scene["aa"], scene["an"], lights, G)
    assert (out != scene["l0"]).any(-1).sum() >= 100


def test_lit_planes_restatement_properties():
    """Discarded pixels are +0, a masked term is absent, and E is added to Lit (not the other way round in value)."""
    import synth
    planes = synth.random_gbuffer(61 * 43, seed=21, discard_frac=0.05)
    planes[19:22] = 0.0
    cam = (3.0, 4.0, -2.0)
    lights = pixel_lights()
    lit = lr.lit_planes(planes, lights, cam, 20.0)
    live = ~(planes[18] < 0.5)
    assert (lit[:, ~live].view(np.uint32) == 0).all()
    assert (lit[:, live] > 0).any(0).sum() >= 500 and (lit[:, live] == 0).all(0).sum() >= 100
    assert not lr.lit_planes(planes, lights, cam, 20.0, mask=31 & ~lr.SHOW_DIFFUSE).any()       # specular planes are 0
    E = np.full((3, planes.shape[1]), 0.25, np.float32)
    both = lr.lit_planes(planes, lights, cam, 20.0, E=E)
    assert np.array_equal(both[:, live], (E[:, live] + lit[:, live]).astype(np.float32)) and not both[:, ~live].any()


def pixel_lights():
    """Lights for synth.random_gbuffer's positions (uniform in [-70, 70]^3): in range of part of the frame only."""
    return [lr.point((10.0, 0.0, -20.0), (400.0, 300.0, 200.0), 60.0, 2.0),
            lr.spot((-40.0, 30.0, 20.0), (900.0, 900.0, 500.0), 80.0, 1.5, (1.0, -0.5, -0.3), 0.9, 0.3),
            lr.point((50.0, -50.0, 50.0), (50.0, 100.0, 150.0), 35.0, 1.0),
            lr.spot((0.0, -60.0, -50.0), (200.0, 500.0, 800.0), 70.0, 2.5, (0.1, 0.8, 0.6), 0.7, 0.2)]


def test_header_and_binding_agree():
    import vctpkg
    vct = vctpkg.load()
    hdr = open(os.path.join(ROOT, "include", "vct.h")).read()
    for name, args in (("vct_set_lights", 3), ("vct_get_lights", 3), ("vct_download_pixel_lights", 2), ("vct_last_lights_ms", 2)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        params = re.sub(r"/\*.*?\*/", "", m.group(1))
        assert len(params.split(",")) == args, (name, m.group(1))
        assert name in vct.ABI_SYMBOLS and hasattr(vct.lib(), name)
        assert len(getattr(vct.lib(), name).argtypes) == args
    assert int(re.search(r"#define VCT_LIGHTS_MAX (\d+)", hdr).group(1)) == vct.LIGHTS_MAX == lr.LIGHTS_MAX == 64
    assert int(re.search(r"#define VCT_LIGHT_SPOT (\d+)u", hdr).group(1)) == vct.LIGHT_SPOT == lr.SPOT
    body = re.search(r"typedef struct vct_light \{(.*?)\} vct_light;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            names.append(decl.split()[-1].split("[")[0])
    assert names == [f[0] for f in vct.Light._fields_]
    assert C.sizeof(vct.Light) == 56
    assert int(re.search(r"#define VCT_ABI_VERSION (\d+)", hdr).group(1)) == vct.ABI_VERSION      # vct_config did not change
    for method in ("set_lights", "lights", "download_pixel_lights", "last_lights_ms"):
        assert callable(getattr(vct.Context, method))
    a, b = vct.point_light((1, 2, 3), (4, 5, 6), 7, 8), lr.point((1, 2, 3), (4, 5, 6), 7, 8)
    assert a == b
    assert vct.spot_light((1, 2, 3), (4, 5, 6), 7, 8, (0, 1, 0), 0.9, 0.5) == lr.spot((1, 2, 3), (4, 5, 6), 7, 8, (0, 1, 0), 0.9, 0.5)


def test_demo_light_option_is_checked_before_a_gpu_is_touched():
    exe = os.path.join(ROOT, "voxel-cone-tracing_amd", "vct_demo")

    def run(*extra):
        return subprocess.run([exe, "--scene", "procedural:cornell", "--voxels", "32", "--size", "64x48", "--shadow", "128",
                               "--frames", "1"] + list(extra), capture_output=True, text=True, timeout=300)
    for bad in ("", "x", "0,8,0", "0,8,0;1,1,1", "0,8,0;1,1,1;25", "0,8,0;1,1,1;25;0.5;", "0,8,0;1,-1,1;25;0.5", "0,8,0;1,1,1;0;0.5",
                "0,8,0;1,1,1;25;0", "nan,8,0;1,1,1;25;0.5", "0,8,0;1,1,1;inf;0.5", "0,8,0;1,1,1;25;0.5;0,-1,0", "0,8,0;1,1,1;25;0.5;0,-1,0;20",
                "0,8,0;1,1,1;25;0.5;0,0,0;20;30", "0,8,0;1,1,1;25;0.5;0,-1,0;30;20", "0,8,0;1,1,1;25;0.5;0,-1,0;20;181",
                "0,8,0;1,1,1;25;0.5;0,-1,0;20;30;7"):
        r = run("--light", bad)
        assert r.returncode == 1 and "--light" in r.stderr, (bad, r.stdout + r.stderr)
    r = run(*(["--light", "0,8,0;1,1,1;25;0.5"] * 65))
    assert r.returncode == 1 and "at most 64" in r.stderr, r.stdout + r.stderr


def test_table_check_and_folding_under_asan_ubsan(tmp_path):
    """The host's check and folding in a stand-alone program under the sanitizers; the folded records of the test lights
    equal lights_ref.fold bit for bit."""
    import vctpkg
    vct = vctpkg.load()
    exe = str(tmp_path / "lights_check")
    src = os.path.join(ROOT, "tests", "lights_check_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    lights = lr.LIGHTS + lr.many_lights() + pixel_lights()
    raw = b"".join(bytes(vct.Context._light(l)) for l in lights)
    fin, fout = str(tmp_path / "lights.bin"), str(tmp_path / "folded.bin")
    open(fin, "wb").write(raw)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "lights_check ok" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    dev = np.fromfile(fout, np.float32).reshape(len(lights), 16)
    for j, l in enumerate(lights):
        L = lr.fold(l)
        want = np.zeros(16, np.float32)
        want[0:3], want[3], want[4:7], want[7] = L["pos"], L["R2"], L["color"], L["S2"]
        if L["spot"]:
            want[8:11], want[11], want[12] = L["axis"], L["cos_outer"], L["inv_cone"]
            want[13:14] = np.array([1], np.uint32).view(np.float32)
        assert np.array_equal(dev[j].view(np.uint32), want.view(np.uint32)), j
