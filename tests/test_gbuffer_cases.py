"""The CPU side of the adversarial G-buffers (tests/gbcases.py) -- no GPU: what every case pixel IS is established here,
on the oracle, before a GPU sees it, so that test_gpu_trace_inputs.py cannot pass because both sides give NaN everywhere.

1. The oracle (V = 16, both wrap modes, and the anisotropic chains once) gives every pixel the class its builder
   declared: finite rgb, some non-finite rgb channel, or the clear colour.
2. Pixels a case does not touch keep the clean frame's bits (frame, per-cone steps, raw cones): a degenerate pixel
   spoils nothing but itself.
3. Only the explicit beyond_contract specs (beyond=True; never traced) leave the position bound of include/vct.h.
4. At least half of a family's case pixels are finite, and the placement holds the three anchor situations.
5. The derivation of the GPU test's 1-ulp bar holds on these inputs: the one inexact operation is the powf of the Phong
   term (trace.fs:213).  OpenCL's bound for pow is 16 ulp and the C library's error is below 1, so the term
   socc * spec * shadow * specColor moves by at most 17 * 2^-24 of itself -- asserted to be under a quarter of the fp16
   spacing at the pixel's value, so the fp16 rounding can at most move to the neighbouring half.
"""
import numpy as np
import pytest

import components_ref as cr
import gbcases as gc
import synth

f32 = np.float32


@pytest.fixture(scope="module")
def chains(oracle):
    l0 = synth.noise_volume(gc.V, occupancy=0.3)
    return oracle.build_mips(l0), oracle.build_mips_aniso(l0)


def params(oracle, case, wrap):
    return oracle.default_params(gc.V, G=case.G, max_distance=case.max_distance, wrap_repeat=wrap, camera_pos=gc.CAM,
                                 light_dir=gc.LIGHT)


def trace(oracle, chains, case, planes, wrap, aniso=False):
    p = params(oracle, case, wrap)
    if aniso:
        return oracle.trace_aniso(p, chains[0], chains[1], planes, nthreads=8, want_cones=True)
    return oracle.trace(p, chains[0], planes, nthreads=8, want_cones=True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_classes(case, ref, clean):
    rgb = ref["rgba32f"][:, :3]
    fin = np.isfinite(rgb).all(1)
    for c in (gc.FINITE, gc.NONFINITE_RGB, gc.DISCARDED):
        sel = case.cls == c
        if c == gc.FINITE:
            assert fin[sel].all(), (case.name, "declared finite, oracle is not", np.flatnonzero(sel & ~fin))
            assert not np.isnan(ref["cones"][sel]).any()
        elif c == gc.NONFINITE_RGB:
            assert not fin[sel].any(), (case.name, "declared non-finite, oracle is finite", np.flatnonzero(sel & fin))
        else:
            assert (ref["rgba32f"][sel] == np.array([0.5, 0.5, 0.5, 1.0], f32)).all()
            assert not ref["steps"][sel].any()
    assert not (case.cls == gc.BEYOND).any()
    keep = ~case.touched
    assert np.array_equal(bits(ref["rgba32f"][keep]), bits(clean["rgba32f"][keep]))
    assert np.array_equal(ref["rgba16f"][keep], clean["rgba16f"][keep])
    assert np.array_equal(ref["steps"][keep], clean["steps"][keep])
    assert np.array_equal(bits(ref["cones"][keep]), bits(clean["cones"][keep]))
    # NaN cones take one step each; a finite pixel's alpha is the plane's
    nan_cone = np.isnan(ref["cones"]).any(2)
    assert (ref["steps"][nan_cone] == 1).all()


def check_powf_margin(case, ref, p):
    """Item 5 of the module docstring, per finite pixel and channel."""
    comp = cr.composite(case.planes, ref["cones"], gc.CAM, gc.LIGHT, p.ambient_factor, p.shininess)
    sel = (case.cls == gc.FINITE) & comp["alive"]
    with np.errstate(all="ignore"):
        socc = f32(1.0) - ref["cones"][:, 6, 3]
        term = np.abs((socc * comp["direct"][:, 1])[:, None] * case.planes[19:22].T).astype(np.float64)
        out = np.abs(ref["rgba32f"][:, :3]).astype(np.float64)
        spacing = 2.0 ** (np.floor(np.log2(np.maximum(out, 2.0 ** -14))) - 10)          # fp16 ulp at |out|
        bad = sel[:, None] & (out < 65520.0) & ~(term * 17 * 2.0 ** -24 <= 0.25 * spacing)
    assert not bad.any(), (case.name, np.argwhere(bad))


@pytest.mark.parametrize("w,h", gc.FRAMES)
@pytest.mark.parametrize("name", gc.CASE_NAMES)
def test_oracle_gives_every_pixel_its_declared_class(oracle, chains, name, w, h):
    case = gc.get_case(name, w, h)
    assert case.planes.shape == (23, w * h) and case.planes.dtype == np.float32
    assert not gc.exceeds_position_bound(case.planes, case.G, case.max_distance).any()
    cp = case.cls[case.touched]
    assert 2 * (cp == gc.FINITE).sum() >= cp.size, (name, "fewer than half of the case pixels are finite")
    for wrap in (1, 0):
        clean = trace(oracle, chains, case, case.base, wrap)
        assert np.unique(bits(clean["cones"]).reshape(-1, 28), axis=0).shape[0] > w * h // 2      # dense enough: cones differ
        ref = trace(oracle, chains, case, case.planes, wrap)
        check_classes(case, ref, clean)
        check_powf_margin(case, ref, params(oracle, case, wrap))
        print(name, (w, h), "wrap", wrap, {c: int((cp == c).sum()) for c in np.unique(cp)},
              "non-finite fp32 values:", int((~np.isfinite(ref["rgba32f"])).sum()))


@pytest.mark.parametrize("name", gc.CASE_NAMES)
def test_anisotropic_oracle_gives_the_same_classes(oracle, chains, name):
    w, h = gc.FRAMES[1]
    case = gc.get_case(name, w, h)
    check_classes(case, trace(oracle, chains, case, case.planes, 1, aniso=True),
                  trace(oracle, chains, case, case.base, 1, aniso=True))


@pytest.mark.parametrize("w,h", gc.FRAMES)
@pytest.mark.parametrize("name", gc.CASE_NAMES)
def test_placement_and_the_position_bound(name, w, h):
    case = gc.get_case(name, w, h)
    live = ~(case.planes[18] < f32(0.5))
    img_t, img_l = case.touched.reshape(h, w), live.reshape(h, w)
    assert img_t[3, 3] and img_l[3, 3]                                                         # the live anchor at lane 27 ...
    assert img_t[:8, :8].sum() == 1 and img_l[:8, :8].all()                                    # ... of a coherent tile
    assert not img_l[3, 11] and img_t[0, 8] and img_l[0, 8]                                    # lane 27 dead, lane 0 the live case
    assert img_t[:8, 16:w].all()                                                               # a tile of case pixels only
    # beyond=True adds exactly the pixels that leave the bound, and changes nothing else
    far = gc.get_case(name, w, h, beyond=True)
    out = gc.exceeds_position_bound(far.planes, far.G, far.max_distance)
    assert np.array_equal(out, far.cls == gc.BEYOND)
    if name.startswith("positions") or name == "frame_scales":
        assert out.any()


def test_an_overflowing_determinant_is_traced(oracle, chains):
    """frame_scales holds in-contract pixels whose fp32 determinant T . (B x N) is +-inf (inv_det = 0), not only
    underflowing ones: the oracle gives each of their diffuse cones one step and NaN."""
    case = gc.get_case("frame_scales", *gc.FRAMES[0])
    N, T, B = (case.planes[k:k + 3] for k in (3, 6, 9))
    with np.errstate(all="ignore"):
        c0 = np.array([B[1] * N[2] - B[2] * N[1], B[2] * N[0] - B[0] * N[2], B[0] * N[1] - B[1] * N[0]], f32)
        det = (T[0] * c0[0] + T[1] * c0[1]) + T[2] * c0[2]
    over = np.isinf(det)
    assert over.sum() >= 3 and np.isfinite(case.planes[:12, over]).all()
    assert not gc.exceeds_position_bound(case.planes, case.G, case.max_distance)[over].any()
    assert (case.cls[over] == gc.NONFINITE_RGB).all()
    ref = trace(oracle, chains, case, case.planes, 1)
    assert np.isnan(ref["cones"][over, :6]).all() and (ref["steps"][over, :6] == 1).all()


def test_the_limit_positions_sit_on_the_bound():
    for name in ("positions_g150", "positions_g100"):
        case = gc.get_case(name, *gc.FRAMES[0])
        g = case.planes.astype(np.float64)
        reach = (np.abs(g[0:3]) + np.abs(g[3:6]) * (case.G / gc.V) + case.max_distance) / case.G
        assert reach.max() <= gc.LIMIT_GRIDS
        # the largest is the last fp32 position under the bound: one more ulp (8 or 16 world units there) leaves it
        worst = np.unravel_index(reach.argmax(), reach.shape)
        p = f32(abs(case.planes[worst[0], worst[1]]))
        assert (float(np.nextafter(p, f32(np.inf))) - float(p)) / case.G + reach.max() > gc.LIMIT_GRIDS
        # and the texel coordinate there is far inside int: (2^20 + 0.5) * 2^10 at the largest grid the library takes
        assert (gc.LIMIT_GRIDS + 0.5) * 1024 + 0.5 < 2.0 ** 31


def test_tiled_layout_and_poisoned_padding():
    w, h = gc.FRAMES[1]
    case = gc.get_case("tangent_frames", w, h)
    tiled, inside = gc.to_tiled(case.planes, w, h)
    img = case.planes.reshape(23, h, w)
    for y, x in ((0, 0), (3, 11), (12, 20), (8, 7)):
        assert np.array_equal(bits(tiled[y // 8, x // 8, :, (y % 8) * 8 + (x % 8)]), bits(img[:, y, x]))
    assert inside.sum() == w * h
    bad = gc.poison_padding(tiled, inside)
    m = np.broadcast_to(inside[:, :, None, :], tiled.shape)
    assert np.array_equal(bits(bad[m]), bits(tiled[m]))
    assert (np.isnan(bad[~m]) | (np.abs(bad[~m]) > f32(1e38))).all()          # every padding value is NaN, +-inf or 3e38
    for v in (np.nan, np.inf, -np.inf, 3e38):
        assert ((bad[~m] == f32(v)) | (np.isnan(bad[~m]) & np.isnan(f32(v)))).any()
