"""GPU: the G-buffer import (include/vct.h "G-buffer import") -- k_gbuffer_import against the numpy restatement of
tests/gbuffer_import_ref.py over the whole format matrix from host and device memory, the library's PCF against the CPU
rasteriser's shadow term, the trace of an imported frame, material ids, tile rows, frame slots, the refusals and the timer.

Bars: planes bit-equal to the restatement with NaN equal to NaN (the sign and payload of a NaN differ between x86 and
gfx950: tests/point_query_ref.py assert_floats_match); frames bit-equal between the two routes of the library and
within the project's bar, relative L2 <= 1e-3, of the CPU oracle.  Frames are 37 x 21 (5 x 3 ragged tiles), 8 x 8 and
1 x 1 at V = 16."""
import ctypes as C
import itertools

import numpy as np
import pytest

import gbuffer_import_ref as ir
import raster_oracle
import synth
import vctpkg

pytestmark = pytest.mark.gpu

f32 = np.float32
V = 16
FRAMES = ((37, 21), (8, 8), (1, 1))
SPECULAR_CONSTANT = (0.25, 0.5, -0.75)
NMAT = 5
EMISSION = np.array([[0, 0, 0], [1.5, 0.25, 0], [0, 2, 4], [0.125, 0.125, 0.125], [3, 0, 1]], f32)
MAT_CLASS = np.array([0, 2, 1, 1, 2], np.uint8)
CLASSES = [(0.07, 20.0), (0.2, 8.0), (0.03, 60.0)]


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available()
    return vctpkg.load()


@pytest.fixture(scope="module")
def inputs():
    return {(w, h): ir.seeded_inputs(w, h, seed=11 + w, nmat=NMAT) for w, h in FRAMES}


def context(vct, w, h, **kw):
    return vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, **kw))


def invalid(vct, call, *args, **kw):
    with pytest.raises(vct.VctError) as e:
        call(*args, **kw)
    assert "(-1)" in str(e.value), str(e.value)      # VCT_ERR_INVALID
    return str(e.value)


def assert_planes(got, want, what):
    bad = np.nonzero((ir.canonical_bits(got) != ir.canonical_bits(want)).any(0))[0]
    assert bad.size == 0, (what, bad.size, bad[:5], np.nonzero(ir.canonical_bits(got)[:, bad[0]] != ir.canonical_bits(want)[:, bad[0]])[0],
                           got[:, bad[0]], want[:, bad[0]])


def select(inp, pf, nf, af, sf, shading=True, shadow=True, material=False):
    """The keyword arguments both Context.import_gbuffer and ir.restate take for one choice of formats."""
    kw = dict(position=inp["position"][pf], normal=inp["normal"][nf], albedo=inp["albedo"][af], position_format=pf, normal_format=nf,
              albedo_format=af, inv_view_proj=inp["inv_view_proj"], depth_clear=float(inp["depth_clear"]))
    if shading:
        kw["shading_normal"] = inp["shading_normal"][nf]
    if sf is not None:
        kw.update(specular=inp["specular"][sf], specular_format=sf)
    else:
        kw["specular_constant"] = SPECULAR_CONSTANT
    if shadow:
        kw["shadow"] = inp["shadow"]
    if material:
        kw["material"] = inp["material"]
    return kw


class DeviceCopies:
    """The buffers of an import's keyword arguments in device memory, each at the LEAST alignment the header promises
    to accept (an odd multiple of its scalar's size); alive until the object goes."""
    NAMES = ("position", "normal", "shading_normal", "albedo", "specular", "shadow", "material")

    def __init__(self, kw):
        import torch
        self.keep, self.kw = [], dict(kw)
        for k in self.NAMES:
            if kw.get(k) is None:
                continue
            a = np.ascontiguousarray(kw[k])
            scalar = a.dtype.itemsize if a.dtype != np.uint8 else 4       # UNORM8X4 is read as one 4-byte element
            t = torch.zeros(a.nbytes + 16, dtype=torch.uint8, device="cuda")
            t[scalar:scalar + a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()
            self.keep.append(t)
            self.kw[k] = t.data_ptr() + scalar
        torch.cuda.synchronize()


# ---- 1: planes, the whole format matrix --------------------------------------------------------------------------------
@pytest.mark.parametrize("pf", [0, 1, 2], ids=["position_f32x3", "position_f32x4", "depth_f32"])
def test_planes_equal_the_restatement_over_the_format_matrix(vct, inputs, pf):
    """3 normal x 3 albedo x (3 specular + constant) formats for this position format, each with no flag, each single flag
    and all flags, from host and from device memory, on the seeded 37 x 21 frame (5 % no-surface pixels, zero / NaN / inf /
    axis-aligned / tied normals, octahedral corners, s = -32768, NaN depth)."""
    w, h = 37, 21
    inp = inputs[(w, h)]
    combos = list(itertools.product(range(3), range(3), (None, 0, 1, 2)))
    assert len(combos) == 36
    with context(vct, w, h) as ctx:
        for k, (nf, af, sf) in enumerate(combos):
            kw = select(inp, pf, nf, af, sf, shading=bool(k & 1), shadow=bool(k & 2))
            dev = DeviceCopies(kw)
            for flags in (0, ir.FLIP_Y, ir.DEPTH_ZERO_TO_ONE, ir.OPAQUE, 7):
                scale = (1.0, 0.05, 2.5)[(k + flags) % 3]
                want = ir.restate(w, h, flags=flags, normal_scale=scale, **kw)
                for where, args in (("host", kw), ("device", dev.kw)):
                    ctx.import_gbuffer(flags=flags, normal_scale=scale, **args)
                    assert_planes(ctx.download_gbuffer(), want, (pf, nf, af, sf, flags, where))
            del dev


@pytest.mark.parametrize("w,h", FRAMES[1:], ids=["8x8", "1x1"])
def test_planes_on_one_tile_and_one_pixel(vct, inputs, w, h):
    inp = inputs[(w, h)]
    with context(vct, w, h) as ctx:
        for k, (pf, nf, af, sf) in enumerate(itertools.product(range(3), range(3), range(3), (None, 0, 1, 2))):
            flags = (0, 1, 2, 4, 7, 3, 5, 6)[k % 8]
            kw = select(inp, pf, nf, af, sf, shading=bool(k & 1), shadow=bool(k & 2))
            want = ir.restate(w, h, flags=flags, **kw)
            args = DeviceCopies(kw) if k % 2 else None
            ctx.import_gbuffer(flags=flags, **(args.kw if args else kw))
            assert_planes(ctx.download_gbuffer(), want, (pf, nf, af, sf, flags))


# ---- 2: shadow -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def atrium():
    """A 64 x 48 view of the flat atrium under a 64^2 shadow map, both from the CPU rasteriser: open sky, umbra, lit floor
    and a wide penumbra (a texel of this map is large)."""
    vctpkg.load()
    from voxel_cone_tracing_amd import scene as sc
    scene = sc.Scene(1, 0.15, 1234)
    light, S, w, h = (0.0, 1.0, 0.25), 64, 64, 48
    depth, light_vp_row = raster_oracle.shadow_map(sc, scene, light, S)
    cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
    planes = raster_oracle.gbuffer(sc, scene, cam, w, h, depth, light_vp_row).reshape(23, -1)
    return dict(w=w, h=h, depth=depth, light_vp_row=light_vp_row, planes=planes, covered=planes[18] >= 0.5)


def atrium_inputs(c, position=None):
    P = np.ascontiguousarray(c["planes"][0:3].T) if position is None else position
    p4 = np.concatenate([P, c["covered"].astype(f32)[:, None]], 1).astype(f32)
    return dict(position=p4, normal=np.ascontiguousarray(c["planes"][3:6].T), albedo=np.ascontiguousarray(c["planes"][15:19].T),
                position_format=ir.POSITION_F32X4, normal_format=ir.NORMAL_F32X3, albedo_format=ir.COLOR_F32X4)


def test_library_pcf_equals_the_rasterisers_shadow_term(vct, atrium):
    c = atrium
    w, h = c["w"], c["h"]
    assert 0.3 < c["covered"].mean() < 1.0
    lit = c["planes"][22][c["covered"]]
    assert (lit == 0).any() and (lit == ir.NO_MAP_SHADOW).any() and ((lit > 0) & (lit < ir.NO_MAP_SHADOW)).any()      # umbra, light, penumbra
    with context(vct, w, h) as ctx:
        ctx.import_gbuffer(**atrium_inputs(c))                        # no map: 25 * 0.111f wherever there is a surface
        got = ctx.download_gbuffer()
        assert (got[22][c["covered"]] == ir.NO_MAP_SHADOW).all() and not got[22][~c["covered"]].any()
        ctx.upload_shadow_map(c["depth"], c["light_vp_row"])
        for args in (atrium_inputs(c), DeviceCopies(atrium_inputs(c)).kw):
            ctx.import_gbuffer(**args)
            got = ctx.download_gbuffer()
            assert np.array_equal(got[22].view(np.uint32), c["planes"][22].view(np.uint32))
            assert np.array_equal(got[0:3].view(np.uint32), c["planes"][0:3].view(np.uint32))
        # a given shadow plane wins over the map
        given = np.random.default_rng(1).random(w * h).astype(f32)
        ctx.import_gbuffer(shadow=given, **atrium_inputs(c))
        assert np.array_equal(ctx.download_gbuffer()[22], np.where(c["covered"], given, 0))
        # the restatement's own PCF agrees with the rasteriser too (it predicts the pixels below)
        lvp = np.ascontiguousarray(np.asarray(c["light_vp_row"], f32).T).reshape(16)
        want = ir.restate(w, h, shadow_map=c["depth"], light_vp=lvp,
                          **atrium_inputs(c))
        assert np.array_equal(want[22].view(np.uint32), c["planes"][22].view(np.uint32))


def test_positions_that_are_not_finite_are_unlit_and_fetch_nothing(vct, atrium):
    c = atrium
    w, h = c["w"], c["h"]
    lvp = np.ascontiguousarray(np.asarray(c["light_vp_row"], f32).T).reshape(16)
    P = np.ascontiguousarray(c["planes"][0:3].T).copy()
    where = np.nonzero(c["covered"])[0][np.random.default_rng(3).permutation(int(c["covered"].sum()))[:12]]
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.inf, -np.inf, np.nan], [3e38, 0, 0], [-3e38, 0, 0],
                    [0, 3e38, 0], [0, -3e38, 0], [0, 0, 3e38], [3e38, 3e38, 3e38], [-3e38, 3e38, -3e38], [1e30, -1e30, 1e30]], f32)
    P[where] = odd
    with context(vct, w, h) as ctx:
        ctx.upload_shadow_map(c["depth"], c["light_vp_row"])
        ctx.import_gbuffer(**atrium_inputs(c))
        before = ctx.download_gbuffer()
        ctx.import_gbuffer(**atrium_inputs(c, P))
        got = ctx.download_gbuffer()
    want = ir.restate(w, h, shadow_map=c["depth"], light_vp=lvp,
                      **atrium_inputs(c, P))
    d = ir.light_space(P[where], lvp)
    unlit = ~np.isfinite(d).all(1)
    assert unlit[:4].all() and (~unlit).any()       # NaN and inf always; 3e38 overflows or, finite, reaches the PCF's clamps
    assert not got[22][where[unlit]].any()
    assert_planes(got, want, "odd positions")
    others = np.ones(w * h, bool)
    others[where] = False
    assert np.array_equal(got[:, others].view(np.uint32), before[:, others].view(np.uint32))
    assert np.array_equal(ir.canonical_bits(got[3:22, where]), ir.canonical_bits(before[3:22, where]))


# ---- 3: trace ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", FRAMES, ids=["37x21", "8x8", "1x1"])
def test_trace_of_an_imported_frame(vct, oracle, inputs, w, h):
    inp = inputs[(w, h)]
    chain = oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.2))
    kw = select(inp, ir.DEPTH_F32, ir.NORMAL_OCT, ir.COLOR_UNORM8X4, ir.COLOR_UNORM8X4)
    planes = ir.restate(w, h, flags=ir.FLIP_Y, **kw)
    with context(vct, w, h) as ctx:
        ctx.upload_chain(chain)
        ctx.import_gbuffer(flags=ir.FLIP_Y, **kw)
        got = ctx.trace_current()
        handed = ctx.trace(planes)                     # LINEAR, host
    assert np.array_equal(got, handed)
    ref = oracle.trace(oracle.default_params(V), chain, planes, nthreads=4)
    g32 = vct.half_to_float(got.reshape(-1, 4))
    ok = np.isfinite(ref["rgba32f"]).all(1) & np.isfinite(g32).all(1)
    live = ~(planes[18] < f32(0.5))
    assert ok[live].sum() >= 0.9 * live.sum()
    err = synth.rel_l2(g32[ok], ref["rgba32f"][ok])
    print(f"{w}x{h}: imported frame against the oracle on the restated planes: relative L2 {err:.3e} over {int(ok.sum())} pixels")
    assert err <= 1e-3


# ---- 4: material ids -----------------------------------------------------------------------------------------------------
def attach_tables(ctx):
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], f32)
    ctx.upload_triangles(tri, np.zeros(1, np.int32), np.ones((NMAT, 4), f32))
    ctx.upload_emission(EMISSION)
    ctx.set_gloss_classes(CLASSES)
    ctx.upload_material_gloss(MAT_CLASS)


@pytest.mark.parametrize("w,h", FRAMES[:2], ids=["37x21", "8x8"])
def test_material_ids_fill_the_emission_and_gloss_planes(vct, inputs, w, h):
    inp = inputs[(w, h)]
    assert (inp["material"] >= NMAT).any() and (inp["material"] < NMAT).any()
    with context(vct, w, h) as ctx:
        attach_tables(ctx)
        for pf, flags in ((ir.POSITION_F32X4, 0), (ir.DEPTH_F32, ir.FLIP_Y), (ir.POSITION_F32X3, 0)):
            kw = select(inp, pf, ir.NORMAL_F16X4, ir.COLOR_UNORM8X4, None, material=True)
            planes, em, gl = ir.restate(w, h, flags=flags, emission=EMISSION, mat_class=MAT_CLASS, **kw)
            for args in (kw, DeviceCopies(kw).kw):
                ctx.set_pixel_emission(np.full((3, w * h), 7.0, f32))
                ctx.set_pixel_gloss(np.full(w * h, 1, np.uint8))
                ctx.import_gbuffer(flags=flags, **args)
                assert_planes(ctx.download_gbuffer(), planes, "planes")
                assert np.array_equal(ctx.download_pixel_emission().view(np.uint32), em.view(np.uint32))
                assert np.array_equal(ctx.download_pixel_gloss(), gl)
            if pf != ir.POSITION_F32X3:
                holes = ~planes.any(0)
                assert holes.any() and not em[:, holes].any() and not gl[holes].any()
        assert em.any() and gl.any()


def test_without_material_ids_the_callers_planes_survive(vct, inputs):
    w, h = 37, 21
    inp = inputs[(w, h)]
    r = np.random.default_rng(8)
    em, gl = r.random((3, w * h)).astype(f32), r.integers(0, 3, w * h).astype(np.uint8)
    with context(vct, w, h) as ctx:
        attach_tables(ctx)
        ctx.set_pixel_emission(em)
        ctx.set_pixel_gloss(gl)
        kw = select(inp, ir.POSITION_F32X4, ir.NORMAL_F32X3, ir.COLOR_F16X4, ir.COLOR_F32X4)
        ctx.import_gbuffer(**kw)
        ctx.import_gbuffer(rows=(1, 2), **DeviceCopies(kw).kw)
        assert np.array_equal(ctx.download_pixel_emission(), em) and np.array_equal(ctx.download_pixel_gloss(), gl)
    # ... and a context with no tables takes material ids without planes to write
    with context(vct, w, h) as ctx:
        ctx.import_gbuffer(material=inp["material"], **kw)
        assert_planes(ctx.download_gbuffer(), ir.restate(w, h, **kw), "no tables")
        invalid(vct, ctx.download_pixel_emission)


# ---- 5: rows and slots ---------------------------------------------------------------------------------------------------
def two_sets(inp):
    a = select(inp, ir.POSITION_F32X4, ir.NORMAL_F16X4, ir.COLOR_UNORM8X4, ir.COLOR_F16X4)
    b = select(inp, ir.DEPTH_F32, ir.NORMAL_OCT, ir.COLOR_F32X4, None)
    return a, b


@pytest.mark.parametrize("flags", [0, ir.FLIP_Y], ids=["bottom_up", "flip_y"])
def test_rows_form_changes_its_tile_rows_only(vct, inputs, flags):
    w, h = 37, 21
    a, b = two_sets(inputs[(w, h)])
    want_a, want_b = ir.restate(w, h, flags=flags, **a), ir.restate(w, h, flags=flags, **b)
    mixed = want_a.reshape(23, h, w).copy()
    mixed[:, 8:16] = want_b.reshape(23, h, w)[:, 8:16]
    with context(vct, w, h) as ctx:
        for args in (b, DeviceCopies(b).kw):
            ctx.import_gbuffer(flags=flags, **a)
            ctx.import_gbuffer(flags=flags, rows=(1, 2), **args)
            assert_planes(ctx.download_gbuffer(), mixed.reshape(23, -1), "rows (1, 2)")
        ctx.import_gbuffer(flags=flags, rows=(2, 2), **b)            # an empty range is a valid import of nothing
        assert_planes(ctx.download_gbuffer(), mixed.reshape(23, -1), "rows (2, 2)")
        ctx.import_gbuffer(flags=flags, rows=(2, 3), **b)            # the ragged last row
        mixed[:, 16:] = want_b.reshape(23, h, w)[:, 16:]
        assert_planes(ctx.download_gbuffer(), mixed.reshape(23, -1), "rows (2, 3)")


def test_an_import_into_slot_1_leaves_slot_0_alone(vct, oracle, inputs):
    w, h = 37, 21
    a, b = two_sets(inputs[(w, h)])
    want_a, want_b = ir.restate(w, h, **a), ir.restate(w, h, **b)
    chain = oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.2))
    with context(vct, w, h) as ctx:
        ctx.upload_chain(chain)
        ctx.set_frames_in_flight(2)
        ctx.select_frame_slot(0)
        ctx.import_gbuffer(**a)
        frame0 = ctx.trace_current()
        ctx.select_frame_slot(1)
        ctx.import_gbuffer(**DeviceCopies(b).kw)
        frame1 = ctx.trace_current()
        assert_planes(ctx.download_gbuffer(), want_b, "slot 1")
        ctx.select_frame_slot(0)
        assert_planes(ctx.download_gbuffer(), want_a, "slot 0")
        assert np.array_equal(ctx.download_frame(), frame0) and not np.array_equal(frame0, frame1)
        assert ctx.last_gbuffer_import_ms() > 0


def tiled(planes, w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    full = np.zeros((23, ty * 8, tx * 8), f32)
    full[:, :h, :w] = planes.reshape(23, h, w)
    return np.ascontiguousarray(full.reshape(23, ty, 8, tx, 8).transpose(1, 3, 0, 2, 4)).reshape(ty * tx, 23, 64)


def test_an_import_after_a_zero_copy_trace_lands_in_the_slots_own_buffer(vct, inputs):
    import torch
    w, h = 37, 21
    a, b = two_sets(inputs[(w, h)])
    want_b = ir.restate(w, h, **b)
    theirs = tiled(synth.random_gbuffer(w * h, seed=5), w, h)
    dev = torch.from_numpy(theirs).cuda()
    with context(vct, w, h) as ctx:
        ctx.trace(dev.data_ptr(), layout=vct.GB_TILED)              # binds the caller's tiled buffer, zero-copy
        ctx.import_gbuffer(**b)
        assert_planes(ctx.download_gbuffer(), want_b, "after a zero-copy trace")
        after = ctx.trace_current()
        assert np.array_equal(after, ctx.trace(want_b))
    assert np.array_equal(dev.cpu().numpy(), theirs)                # the caller's buffer was not written


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_resident_gbuffer_unchanged(vct, inputs):
    w, h = 37, 21
    inp = inputs[(w, h)]
    a, b = two_sets(inp)
    want_a = ir.restate(w, h, **a)
    nan, inf = float("nan"), float("inf")
    L = vct.lib()
    with context(vct, w, h) as ctx:
        ctx.import_gbuffer(**a)
        bad = []
        for k in ("position", "normal", "albedo"):
            bad.append(dict(b, **{k: None}))
        for k in ("position_format", "normal_format", "albedo_format"):
            bad += [dict(b, **{k: 3}), dict(b, **{k: -1})]
        bad.append(dict(b, specular=inp["specular"][0], specular_format=5))
        bad += [dict(b, flags=8), dict(b, flags=0x80000001)]
        for i in (0, 9, 15):
            m = inp["inv_view_proj"].copy()
            m[i] = (nan, inf, -inf)[i % 3]
            bad.append(dict(b, inv_view_proj=m))
        bad += [dict(b, normal_scale=s) for s in (0.0, -1.0, nan, inf)]
        bad += [dict(b, specular_constant=c) for c in ((nan, 0, 0), (0, inf, 0), (0, 0, -inf))]
        bad += [dict(b, rows=r) for r in ((-1, 1), (0, 4), (2, 1), (4, 4))]
        for kw in bad:
            invalid(vct, ctx.import_gbuffer, **kw)
        # an unknown location, a NULL descriptor and a NULL context: only the C ABI can say those
        d = vct.GBufferImport()
        keep = [np.ascontiguousarray(b[k]) for k in ("position", "normal", "albedo")]
        d.position, d.normal, d.albedo = (x.ctypes.data for x in keep)
        d.position_format, d.normal_format, d.albedo_format = b["position_format"], b["normal_format"], b["albedo_format"]
        d.inv_view_proj[:] = [float(x) for x in inp["inv_view_proj"]]
        d.depth_clear, d.normal_scale = 1.0, 1.0
        for loc in (2, -1):
            d.location = loc
            assert L.vct_import_gbuffer(ctx._h, C.byref(d)) == -1
        d.location = vct.MEM_HOST
        assert L.vct_import_gbuffer(ctx._h, None) == -1 and L.vct_import_gbuffer_rows(ctx._h, None, 0, 1) == -1
        assert L.vct_import_gbuffer(None, C.byref(d)) == -1 and L.vct_last_gbuffer_import_ms(None, None) == -1
        assert_planes(ctx.download_gbuffer(), want_a, "after the refusals")
        assert L.vct_import_gbuffer(ctx._h, C.byref(d)) == 0        # ... and the descriptor they refused was otherwise good
        plain = {k: v for k, v in b.items() if k not in ("shading_normal", "shadow", "specular_constant")}
        assert_planes(ctx.download_gbuffer(), ir.restate(w, h, **plain), "the good descriptor")
        # the matrix and the constant are not looked at where they are not used
        ctx.import_gbuffer(**dict(a, inv_view_proj=np.full(16, nan, f32), specular_constant=(nan, nan, nan)))
        assert_planes(ctx.download_gbuffer(), want_a, "unused fields")


# ---- 7: the timer --------------------------------------------------------------------------------------------------------
def test_last_gbuffer_import_ms(vct, inputs):
    w, h = 37, 21
    a, _ = two_sets(inputs[(w, h)])
    with context(vct, w, h) as ctx:
        invalid(vct, ctx.last_gbuffer_import_ms)                      # no import yet
        ctx.import_gbuffer(**a)
        ms = ctx.last_gbuffer_import_ms()
        assert 0.0 < ms < 50.0
        ctx.set_trace_timing(False)
        ctx.import_gbuffer(**a)
        msg = invalid(vct, ctx.last_gbuffer_import_ms)
        assert "timing" in msg
        ctx.set_trace_timing(True)
        ctx.import_gbuffer(**DeviceCopies(a).kw)
        assert ctx.last_gbuffer_import_ms() > 0.0
