"""CPU: the G-buffer import (include/vct.h "G-buffer import") without a GPU -- the descriptor check, the element sizes and
the per-pixel arithmetic of csrc/vct_import_check.h in a stand-alone program with and without ASan + UBSan, bit for bit
against the numpy restatement of tests/gbuffer_import_ref.py; the tangent frame's orthonormality; the header's enums, flags
and struct against the Python mirror; and the depth reconstruction against float64."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gbuffer_import_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def build_check(tmp, sanitize):
    exe = os.path.join(str(tmp), "import_check_san" if sanitize else "import_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "import_check_main.cpp")])
    return exe


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("import_check")
    return tmp, build_check(tmp, False), build_check(tmp, True)


def test_descriptor_verdicts_with_and_without_asan_ubsan(checkers):
    _, plain, san = checkers
    for exe in (plain, san):
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert "import_check ok" in out.stdout
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def write_case(path, w, h, inp, pf, nf, af, sf, flags, shading, shadow, normal_scale, specular_constant):
    """One import in the layout tests/import_check_main.cpp reads; sf None: no specular buffer."""
    with open(path, "wb") as f:
        f.write(struct.pack("10i", w, h, pf, nf, af, 0 if sf is None else sf, flags, int(shading), int(sf is not None), int(shadow)))
        f.write(np.ascontiguousarray(inp["inv_view_proj"], f32).tobytes())
        f.write(struct.pack("5f", float(inp["depth_clear"]), normal_scale, *specular_constant))
        bufs = [inp["position"][pf], inp["normal"][nf]] + ([inp["shading_normal"][nf]] if shading else []) + [inp["albedo"][af]]
        bufs += ([] if sf is None else [inp["specular"][sf]]) + ([inp["shadow"]] if shadow else [])
        for b in bufs:
            f.write(np.ascontiguousarray(b).tobytes())


def restate_case(w, h, inp, pf, nf, af, sf, flags, shading, shadow, normal_scale, specular_constant):
    return ir.restate(w, h, inp["position"][pf], inp["normal"][nf], inp["albedo"][af],
                      shading_normal=inp["shading_normal"][nf] if shading else None,
                      specular=None if sf is None else inp["specular"][sf], shadow=inp["shadow"] if shadow else None,
                      position_format=pf, normal_format=nf, albedo_format=af, specular_format=sf or 0, flags=flags,
                      inv_view_proj=inp["inv_view_proj"], depth_clear=inp["depth_clear"], normal_scale=normal_scale,
                      specular_constant=specular_constant)


def test_per_pixel_arithmetic_equals_the_restatement_bit_for_bit(checkers):
    """Every format of every input, both flip and depth-range flags, OPAQUE, with and without the optional buffers, on
    seeded frames that hold zero / NaN / inf / axis-aligned / tied normals, the octahedral corners and s = -32768, no-surface
    pixels of both kinds and NaN depths -- the C function against numpy, NaNs at the same places (their sign and payload
    are the one thing IEEE 754 leaves open: ir.canonical_bits)."""
    tmp, plain, san = checkers
    w, h = 37, 21
    inp = ir.seeded_inputs(w, h, seed=11)
    combos = list(itertools.product(range(3), range(3), range(3), (None, 0, 1, 2)))
    assert len(combos) == 108
    seen_nan = seen_hole = 0
    for k, (pf, nf, af, sf) in enumerate(combos):
        flags = (0, 1, 2, 4, 7, 3, 5, 6)[k % 8]
        shading, shadow = bool(k & 1), bool(k & 2)
        scale = (1.0, 0.05, 2.5)[k % 3]
        const = (0.25, 0.5, -0.75)
        case, out = os.path.join(str(tmp), "case.bin"), os.path.join(str(tmp), "out.bin")
        write_case(case, w, h, inp, pf, nf, af, sf, flags, shading, shadow, scale, const)
        want = restate_case(w, h, inp, pf, nf, af, sf, flags, shading, shadow, scale, const)
        for exe in ((plain, san) if k % 4 == 0 else (plain,)):       # the sanitized build is ~10x slower: every format of every input still passes through it
            subprocess.check_call([exe, case, out], timeout=300)
            got = np.fromfile(out, f32).reshape(23, w * h)
            bad = np.nonzero((ir.canonical_bits(got) != ir.canonical_bits(want)).any(0))[0]
            assert bad.size == 0, ((pf, nf, af, sf, flags), bad[:5], got[:, bad[:1]].ravel(), want[:, bad[:1]].ravel())
        seen_nan += int(np.isnan(want).any())
        seen_hole += int((~want.any(0)).sum() > 0)
        if not shadow:
            live = want[18] != 0
            assert (want[22][live] == ir.NO_MAP_SHADOW).all()
    assert seen_nan >= 50 and seen_hole >= 60           # the adversarial values reach the planes


def test_every_half_and_every_snorm16_decodes_as_numpy_has_it(checkers):
    """All 65536 bit patterns of a half through the F16X4 colour path (planes 15-17 and 19-21 hold them as they are) and all
    65536 SNORM16 values through the octahedral path, against numpy's own conversions."""
    tmp, plain, _ = checkers
    w, h = 256, 128
    inp = ir.seeded_inputs(w, h, seed=1)
    every = np.arange(65536, dtype=np.uint16)
    inp["albedo"][ir.COLOR_F16X4] = np.tile(every, 2).view(np.float16).reshape(w * h, 4)
    inp["specular"][ir.COLOR_F16X4] = np.tile(every[::-1], 2).view(np.float16).reshape(w * h, 4)
    inp["normal"][ir.NORMAL_OCT] = np.ascontiguousarray(every.view(np.int16).reshape(2, w * h).T)
    case, out = os.path.join(str(tmp), "halves.bin"), os.path.join(str(tmp), "halves_out.bin")
    args = (w, h, inp, ir.POSITION_F32X3, ir.NORMAL_OCT, ir.COLOR_F16X4, ir.COLOR_F16X4, 0, False, False, 1.0, (0, 0, 0))
    write_case(case, *args)
    subprocess.check_call([plain, case, out], timeout=300)
    got, want = np.fromfile(out, f32).reshape(23, w * h), restate_case(*args)
    assert np.array_equal(ir.canonical_bits(got), ir.canonical_bits(want))
    assert np.array_equal(ir.canonical_bits(want[15:19].T.reshape(-1)[:65536]), ir.canonical_bits(every.view(np.float16).astype(f32)))


def test_flags_move_what_they_say():
    """FLIP_Y reads the mirrored row and nothing else; DEPTH_ZERO_TO_ONE changes only nz; OPAQUE only plane 18."""
    w, h = 37, 21
    inp = ir.seeded_inputs(w, h, seed=3)
    base = dict(shading=True, shadow=True, normal_scale=1.0, specular_constant=(0, 0, 0))
    a = restate_case(w, h, inp, ir.POSITION_F32X4, ir.NORMAL_F16X4, ir.COLOR_UNORM8X4, ir.COLOR_F16X4, 0, **base)
    b = restate_case(w, h, inp, ir.POSITION_F32X4, ir.NORMAL_F16X4, ir.COLOR_UNORM8X4, ir.COLOR_F16X4, ir.FLIP_Y, **base)
    assert np.array_equal(ir.canonical_bits(a).reshape(23, h, w), ir.canonical_bits(b).reshape(23, h, w)[:, ::-1])
    o = restate_case(w, h, inp, ir.POSITION_F32X4, ir.NORMAL_F16X4, ir.COLOR_UNORM8X4, ir.COLOR_F16X4, ir.OPAQUE, **base)
    live = a[:18].any(0) | a[19:].any(0)
    assert np.array_equal(ir.canonical_bits(np.delete(a, 18, 0)), ir.canonical_bits(np.delete(o, 18, 0)))
    assert (o[18][live] == 1).all() and (a[18][live] != 1).any()
    # a depth input under FLIP_Y: the depth comes from the mirrored row, nx / ny from the frame's own x, y
    d0 = restate_case(w, h, inp, ir.DEPTH_F32, ir.NORMAL_OCT, ir.COLOR_UNORM8X4, None, 0, **base)
    d1 = restate_case(w, h, inp, ir.DEPTH_F32, ir.NORMAL_OCT, ir.COLOR_UNORM8X4, None, ir.FLIP_Y, **base)
    assert not np.array_equal(ir.canonical_bits(d0[:3]).reshape(3, h, w), ir.canonical_bits(d1[:3]).reshape(3, h, w)[:, ::-1])
    z = restate_case(w, h, inp, ir.DEPTH_F32, ir.NORMAL_OCT, ir.COLOR_UNORM8X4, None, ir.DEPTH_ZERO_TO_ONE, **base)
    assert np.array_equal(ir.canonical_bits(d0[3:]), ir.canonical_bits(z[3:])) and not np.array_equal(d0[:3], z[:3])


def test_frame_is_orthonormal_and_right_handed():
    """For finite non-zero normals t, b, u are orthonormal to a few ulp and dot(cross(t, b), u) > 0.  Bound: u and t are
    fp32 normalisations (each component within 1.5 ulp of the exact unit vector: one rounding of the squared length, one of
    the square root, one of the reciprocal, one of the product), b is a cross product of two such vectors (two products and
    a difference per component), so every dot product and squared length is within 8 * 2^-23 ~ 1e-6 of its ideal value."""
    r = np.random.default_rng(5)
    n = np.concatenate([r.normal(size=(50000, 3)) * 10.0 ** r.uniform(-15, 15, (50000, 1)),
                        ir.ADVERSARIAL_NORMALS[np.isfinite(ir.ADVERSARIAL_NORMALS).all(1) & ir.ADVERSARIAL_NORMALS.any(1)]]).astype(f32)
    len2 = (n.astype(np.float64) ** 2).sum(1)
    n = n[(len2 < 3e38) & (len2 > 1e-30)]       # the squared length stays a normal fp32 number
    u, t, b = (v.astype(np.float64) for v in ir.frame(n))
    tol = 8 * 2.0 ** -23
    for v in (u, t, b):
        assert np.abs((v * v).sum(1) - 1.0).max() <= tol
    for p, q in ((u, t), (u, b), (t, b)):
        assert np.abs((p * q).sum(1)).max() <= tol
    assert ((np.cross(t, b) * u).sum(1) > 1.0 - 2 * tol).all()
    # u is the normal's direction
    un = n.astype(np.float64) / np.linalg.norm(n.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(u - un).max() <= tol


def test_header_values_and_struct_match_the_python_mirror():
    import vctpkg
    vct = vctpkg.load()
    hdr = open(os.path.join(ROOT, "include", "vct.h")).read()
    for name, value in re.findall(r"\b(VCT_IMPORT_[A-Z0-9_]+) = (\d+)", hdr) + re.findall(r"#define (VCT_IMPORT_[A-Z0-9_]+) (\d+)u", hdr):
        assert getattr(vct, name[4:]) == int(value), name
        assert getattr(ir, name[len("VCT_IMPORT_"):].replace("OCT_SNORM16X2", "OCT")) == int(value), name
    assert len(re.findall(r"\bVCT_IMPORT_[A-Z0-9_]+ = \d+", hdr)) == 9 and len(re.findall(r"#define VCT_IMPORT_[A-Z0-9_]+ \d+u", hdr)) == 3
    body = re.search(r"typedef struct vct_gbuffer_import \{(.*?)\} vct_gbuffer_import;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", n).strip(" *") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl).split(",")]
    assert names == [f[0] for f in vct.GBufferImport._fields_]
    # sizeof as the C compiler has it: 7 pointers, 6 x 4 bytes, 16 + 1 + 1 + 3 floats, padded to the pointers' alignment
    want = 7 * 8 + 6 * 4 + 21 * 4
    assert C.sizeof(vct.GBufferImport) == (want + 7) // 8 * 8 == 168
    src = '#include "include/vct.h"\n#include <stddef.h>\nstatic_assert(sizeof(vct_gbuffer_import) == 168 && offsetof(vct_gbuffer_import, flags) == 76 && ' \
          'offsetof(vct_gbuffer_import, specular_constant) == 152, "layout");\n'
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", "-I", ROOT, "-"], input=src, text=True, check=True, cwd=ROOT)
    assert vct.ABI_VERSION == 8 and "#define VCT_ABI_VERSION 8" in hdr


def test_depth_reconstruction_against_float64():
    """World points projected with a double-precision matrix into a depth buffer come back: the fp32 restatement against the
    same formula in float64 on the same fp32 inputs (depth, matrix).
    Bound.  r_i is a four-term fp32 dot product of m's row i with (nx, ny, nz, 1): with u = 2^-24, nx, ny, nz each carry at
    most 3u relative error from their own arithmetic (|n| <= 1), each product one more rounding and each of the three adds
    one more, so |r_i - exact| <= 8u * sum_j |m_ij| |n_j| <= 8u * |m|_inf (row-sum norm, |n_j| <= 1).  P = r_xyz / r_w:
    the quotient's error is (|dr_xyz| + |P| |dr_w|) / |r_w| plus one rounding, so
    |P_c - exact| <= 8u * |m|_inf * (1 + |P_c|) / |r_w| + u * |P_c| per pixel and axis.  A factor 2 covers second-order terms."""
    w, h = 37, 21
    inp = ir.seeded_inputs(w, h, seed=21)
    inv = inp["inv_view_proj"].astype(np.float64)
    view_proj = np.linalg.inv(inv.reshape(4, 4).T).T.reshape(16)
    r = np.random.default_rng(2)
    n = w * h
    ys, xs = np.divmod(np.arange(n), w)
    for zero_to_one in (False, True):
        # points on the pixel centres' rays: choose a view depth per pixel, unproject in float64, project for the depth value
        nx, ny = (2 * (xs + 0.5)) / w - 1, (2 * (ys + 0.5)) / h - 1
        M = inv.reshape(4, 4).T
        ndc_z = r.uniform(-0.5, 0.995, n)
        q = np.stack([nx, ny, ndc_z, np.ones(n)], 1) @ M.T
        world = q[:, :3] / q[:, 3:4]
        px, py, depth = ir.project_depth(world, view_proj, zero_to_one)
        assert np.abs(px - nx).max() < 1e-9 and np.abs(py - ny).max() < 1e-9
        depth32 = depth.astype(f32)
        flags = ir.DEPTH_ZERO_TO_ONE if zero_to_one else 0
        got = ir.restate(w, h, depth32, inp["normal"][0], inp["albedo"][0], position_format=ir.DEPTH_F32, flags=flags,
                         inv_view_proj=inp["inv_view_proj"], depth_clear=2.0)[:3].T.astype(np.float64)
        # the reference: the header's formula in float64 on the same fp32 depth and matrix
        nz = depth32.astype(np.float64) if zero_to_one else 2 * depth32.astype(np.float64) - 1
        rr = np.stack([nx, ny, nz, np.ones(n)], 1) @ M.T
        ref = rr[:, :3] / rr[:, 3:4]
        u = 2.0 ** -24
        norm_inf = np.abs(M).sum(1).max()
        bound = 2 * (8 * u * norm_inf * (1 + np.abs(ref)) / np.abs(rr[:, 3:4]) + u * np.abs(ref))      # per pixel and axis
        err = np.abs(got - ref)
        print(f"depth reconstruction (zero_to_one={zero_to_one}): worst error {err.max():.3e} (worst share of its bound "
              f"{(err / bound).max():.3f}), |m|_inf {norm_inf:.1f}, |P| up to {np.abs(ref).max():.1f}")
        assert (err <= bound).all()
        # ... and the points are the ones that were projected, to the depth buffer's own fp32 quantisation
        assert np.abs(ref - world).max() <= np.abs(world).max() * 1e-3
