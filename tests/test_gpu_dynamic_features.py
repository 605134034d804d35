"""GPU: the dynamic mesh's draw, bounce and emission switches (vct_set_dynamic_draw / _bounce / _emission) outside the small
worlds of their own files, bit-equal to the CPU oracle or to a synchronised replay like those files and with their helpers.
No tolerance is involved.  What runs here and in no earlier file:

  A  k_gbuffer_shade<TEX = true, DYN = true>: dyndrawcases' room with texture coordinates, four maps (diffuse, specular,
     height, an alpha-tested lace) and the mover drawn -- the per-lane dynamic select in front of the texture-index and UV
     loads, the alpha class and the bump normal; the static alpha test together with the second visibility buffer (a
     discarded static fragment in front of, or tied with, a dynamic one); texture_mipmaps 1 and 0; both raster forms, and
     VctRasterForm::pick's six-pass automatic sampling with the mover drawn behind every sample
  B  the EMIS forms of k_dyn_tris / k_dyn_big and of k_dyn_merge at 8^3 (one brick), 16^3 and 128^3, with and without
     voxel attributes; k_bounce_list / _march / _bricks<WRAP, FASTDIV, DYN = true> at 8^3, 16^3 and 128^3 (brick_res
     indices beyond 9 bits), and their FASTDIV = 0 forms (max_alpha 0.97) in both WRAP forms at 64^3 and on the dense 16^3
     scene; emission and bounce together at 128^3

tests/test_gpu_dynamic_readers.py holds the readers with the switches on (a rank context, pixel lights, the half-rate
gather and the outputs, directional chains, the voxel view), tests/test_gpu_pipeline_features.py the random call orders
on two frame slots with the three switches (FEAT_SEEDS) and the directed draw order at full size.  The premises of A are held without a GPU
by tests/test_dynamic_draw_cases.py, those of B by tests/test_dynamic_emission_cases.py and tests/test_dynamic_bounce_cases.py;
every test asserts, on the oracle's output, the non-degeneracy of what it compares."""
import numpy as np
import pytest

import dynbouncecases as db
import dyncases as dc
import dyndrawcases as ddc
import dynemiscases as de
import emission_ref
import gloss_ref
from test_gpu_dynamic import run_pass
from test_gpu_dynamic_bounce import assert_bounced
from test_gpu_dynamic_draw import BOTH, assert_map, assert_planes, bits, draw, make_ctx, vct  # noqa: F401
from test_gpu_dynamic_emission import DYN_EM, assert_emission_planes, assert_pass, static_em
from test_gpu_dynamic_forms import grid_ctx, grid_world
from test_gpu_march_params import IEEE, expected_form, form_of

pytestmark = pytest.mark.gpu
W, H, S = ddc.W, ddc.H, ddc.SHADOW
DIRECT, BINNED = 1, 2                       # stage_counts()["raster_form"]


# ---- A. a textured static mesh with the mover drawn ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(oracle):
    """The textured room, the object at A and B, and the checker's map and planes: r[k, w, mip] for k in A, B, "S" (the room
    alone) and "DUP" (the duplicate of TIE as the only dynamic triangle), r[k, w, "plain"] without textures."""
    r = dict(static=ddc.static_mesh(), A=ddc.object_mesh("A"), B=ddc.object_mesh("B"))
    pos, mat, alb = r["A"]
    idx = ddc.PARTS["DUP"]
    r["DUP"] = (pos[idx], mat[idx], alb)
    for k in ("A", "B", "DUP"):
        r[k, "cat"] = ddc.concatenated(r["static"], r[k])
        r[k, "tex"] = ddc.textured_cat(r[k][0].shape[0], r[k][2].shape[0])
    r["S", "cat"], r["S", "tex"] = r["static"], ddc.textured_cat()
    for w, h in ddc.FRAMES:
        for k in ("A", "B", "DUP", "S"):
            r[k, w, "plain"] = ddc.reference(oracle, r[k, "cat"], w, h)
            for mip in (1, 0):
                r[k, w, mip] = ddc.reference(oracle, r[k, "cat"], w, h, tex=r[k, "tex"], mipmaps=bool(mip))
    return r


def textured_ctx(vct, r, w=W, h=H, path=None, mip=1, **kw):
    ctx = make_ctx(vct, r["static"], w, h, path=path, texture_mipmaps=mip, **kw)
    ctx.upload_mesh_uvs(ddc.room_uv())
    ctx.upload_textures(ddc.room_textures(), ddc.room_mat_tex())
    return ctx


def holes(r, k, w, mip):
    """Pixels the dynamic mesh owns in the textured room and the static mesh in the untextured one."""
    plain, tx = r[k, w, "plain"][1], r[k, w, mip][1]
    return ddc.owner_is_dynamic(tx) & ~ddc.owner_is_dynamic(plain) & (plain[18] >= 0.5)


@pytest.mark.parametrize("w,h", ddc.FRAMES)
@pytest.mark.parametrize("path", ["direct", "binned"])
@pytest.mark.parametrize("mip", [1, 0])
def test_textured_gbuffer_all_planes(vct, room, mip, path, w, h):
    big = w == W
    for k in "AB":
        depth, planes = room[k, w, mip]
        own = ddc.owner_is_dynamic(planes)
        static_px = ~own & (planes[18] >= 0.5)
        assert own.sum() >= (300 if big else 5)
        assert ((bits(planes) != bits(room[k, w, "plain"][1])).any(0) & static_px).sum() >= (1000 if big else 20)
        assert ((bits(planes) != bits(room[k, w, 1 - mip][1])).any(0) & static_px).sum() >= (500 if big else 20)
        assert np.array_equal(bits(depth), bits(room[k, w, "plain"][0]))           # the shadow pass does not alpha-test
    if big:
        assert holes(room, "A", w, mip).sum() >= 150           # (at B the object has left the occluder: a handful)
    assert (bits(room["A", w, mip][1]) != bits(room["B", w, mip][1])).any(0).sum() >= (300 if big else 5)
    with textured_ctx(vct, room, w, h, path, mip) as ctx:
        ctx.set_dynamic_mesh(*room["A"])
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        rows = (h + 7) // 8
        mid = (rows // 3, max(rows // 3 + 1, 2 * rows // 3))
        what = f"textured, mipmaps={mip}, {path}, {w}x{h}"
        for rs in (None, mid, None):            # a scissored pass between two whole ones: both buffers stay armed
            draw(ctx, w, h, rs)
            assert ctx.stage_counts()["raster_form"] == (DIRECT if path == "direct" else BINNED)
            assert_map(ctx, room["A", w, mip][0], f"{what}, rows {rs}")
            assert_planes(ctx, room["A", w, mip][1], f"{what}, rows {rs}", rs, w, h)
        for k in "BA":
            ctx.update_dynamic_positions(room[k][0])
            draw(ctx, w, h)
            assert_map(ctx, room[k, w, mip][0], f"{what}, at {k}")
            assert_planes(ctx, room[k, w, mip][1], f"{what}, at {k}", None, w, h)


@pytest.mark.parametrize("path", ["direct", "binned"])
@pytest.mark.parametrize("mip", [1, 0])
def test_textured_tie_goes_to_the_dynamic_duplicate_where_the_alpha_test_discards(vct, room, mip, path):
    """DUP ties TIE's depth on every pixel: TIE owns what its lace keeps, DUP exactly what it discards."""
    depth, planes = room["DUP", W, mip]
    own = ddc.owner_is_dynamic(planes)
    assert own.sum() >= 50 and ddc.owner_is_dynamic(room["DUP", W, "plain"][1]).sum() == 0
    tie = room["DUP", W, "plain"][1][15] == room["static"][2][6, 0]
    assert not (own & ~tie).any() and (tie & ~own).sum() >= 200
    with textured_ctx(vct, room, W, H, path, mip) as ctx:
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        ctx.set_dynamic_mesh(*room["DUP"])
        for rnd in range(2):
            draw(ctx)
            assert_map(ctx, depth, f"DUP alone, mipmaps={mip}, {path}, pass {rnd}")
            assert_planes(ctx, planes, f"DUP alone, mipmaps={mip}, {path}, pass {rnd}")


@pytest.mark.parametrize("mip", [1, 0])
def test_automatic_form_choice_with_the_mover_drawn(vct, room, mip):
    """VCT_RASTER_PATH unset and an alpha-tested map uploaded: the first six G-buffer passes are the timed samples direct,
    direct, binned, binned, direct, binned, then the verdict holds.  The object alternates A / B in between, so words left
    in either visibility buffer across a switch of forms would show."""
    assert holes(room, "A", W, mip).sum() >= 150
    with textured_ctx(vct, room, W, H, None, mip) as ctx:
        ctx.set_dynamic_mesh(*room["A"])
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        forms = []
        for i in range(8):
            k = "AB"[i & 1]
            ctx.update_dynamic_positions(room[k][0])
            draw(ctx)
            forms.append(ctx.stage_counts()["raster_form"])
            assert_map(ctx, room[k, W, mip][0], f"automatic, pass {i} at {k}")
            assert_planes(ctx, room[k, W, mip][1], f"automatic, pass {i} at {k} (form {forms[-1]})")
        assert forms[:6] == [DIRECT, DIRECT, BINNED, BINNED, DIRECT, BINNED], forms      # kAutoSeq (csrc/vct_api_raster.hip)
        assert forms[6] == forms[7] and forms[6] in (DIRECT, BINNED), forms
        rows = (H + 7) // 8
        mid = (rows // 3, 2 * rows // 3)
        ctx.update_dynamic_positions(room["A"][0])
        draw(ctx, W, H, mid)
        assert_planes(ctx, room["A", W, mip][1], "automatic, rows", mid)
        keep = np.ones(H, bool)
        keep[mid[0] * 8:mid[1] * 8] = False
        got = ctx.download_gbuffer().reshape(23, H, W)
        assert np.array_equal(bits(got[:, keep]), bits(room["B", W, mip][1].reshape(23, H, W)[:, keep])), "rows outside the scissor"
        draw(ctx)
        assert_planes(ctx, room["A", W, mip][1], "automatic, whole pass behind the rows")


def test_automatic_form_choice_starts_again_with_new_textures(vct, room):
    """A texture upload in mid-sequence restarts the sampling; the mover stays drawn through it."""
    with textured_ctx(vct, room, W, H, None, 1) as ctx:
        ctx.set_dynamic_mesh(*room["A"])
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        forms = []
        for i in range(3):
            draw(ctx)
            forms.append(ctx.stage_counts()["raster_form"])
            assert_planes(ctx, room["A", W, 1][1], f"before the upload, pass {i}")
        ctx.upload_textures(ddc.room_textures(), ddc.room_mat_tex())
        ctx.update_dynamic_positions(room["B"][0])
        for i in range(3):
            draw(ctx)
            forms.append(ctx.stage_counts()["raster_form"])
            assert_planes(ctx, room["B", W, 1][1], f"behind the upload, pass {i}")
        assert forms == [DIRECT, DIRECT, BINNED, DIRECT, DIRECT, BINNED], forms


def flat_planes(oracle, cat, planes, w, h):
    """`planes` with the albedo planes 15-18 of every covered pixel replaced by its material's table albedo, so that
    emission_ref.pixel_emission and gloss_ref.pixel_class (which name a pixel's material by its flat albedo) apply to a
    textured frame.  The material of a pixel: the one whose triangles, drawn alone, give that pixel's position bit for bit
    -- among the dynamic materials where the palette names the owner, among the static ones elsewhere."""
    pos, mat, alb, spec, frames = cat
    nstat = ddc.static_mesh()[2].shape[0]
    covered = (bits(planes[15:19]) != 0).any(0)
    own = ddc.owner_is_dynamic(planes)
    out, seen = np.array(planes, copy=True), np.zeros(planes.shape[1], bool)
    for m in range(alb.shape[0]):
        t = mat == m
        alone = (pos[t], np.zeros(int(t.sum()), np.int32), alb[m:m + 1], spec[m:m + 1], tuple(f[t] for f in frames))
        _, p = ddc.reference(oracle, alone, w, h, with_shadow=False)
        hit = covered & (p[18] >= 0.5) & (bits(p[0:3]) == bits(planes[0:3])).all(0) & (own == (m >= nstat)) & ~seen
        out[15:19, hit] = alb[m][:, None]
        seen |= hit
    assert np.array_equal(seen, covered), "a covered pixel is no material's"
    return out


@pytest.mark.parametrize("path", ["direct", "binned"])
def test_textured_emission_and_gloss_planes(vct, oracle, room, path):
    """Static emission, the dynamic table, gloss classes and a material class map over the textured room: dynamic pixels
    have class 0 and the dynamic table's emission, holes in the lace included."""
    static, cat = room["static"], room["A", "cat"]
    nstat = static[2].shape[0]
    depth, planes = room["A", W, 1]
    sem = static_em(nstat)
    classes = [(0.07, 20.0), (0.2, 8.0), (0.03, 60.0)]
    mat_class = (1 + np.arange(nstat) % 2).astype(np.uint8)
    flat = flat_planes(oracle, cat, planes, W, H)
    E = emission_ref.pixel_emission(flat, cat[2], np.concatenate([sem, DYN_EM]))
    cls = gloss_ref.pixel_class(flat, cat[2], np.concatenate([mat_class, np.zeros(3, np.uint8)]))
    _, planes_s = room["S", W, 1]
    flat_s = flat_planes(oracle, static, planes_s, W, H)
    E_off, cls_off = emission_ref.pixel_emission(flat_s, static[2], sem), gloss_ref.pixel_class(flat_s, static[2], mat_class)
    own, hole = ddc.owner_is_dynamic(planes), holes(room, "A", W, 1)
    assert hole.sum() >= 150 and (E[:, hole] > 0).any(0).sum() >= 50 and (cls[own] == 0).all()
    assert (E_off[:, hole] > 0).any(0).sum() >= 50 and (cls_off[hole] > 0).sum() >= 150      # the lace glows and is classed
    assert (cls[~own] > 0).sum() >= 1000 and (E[:, ~own] > 0).any(0).sum() >= 1000
    with textured_ctx(vct, room, W, H, path, 1) as ctx:
        ctx.upload_emission(sem)
        ctx.set_gloss_classes(classes)
        ctx.upload_material_gloss(mat_class)
        ctx.set_dynamic_mesh(*room["A"])
        ctx.set_dynamic_emission(DYN_EM)
        ctx.set_dynamic_draw(BOTH, ddc.SPECULAR)
        for rnd in range(2):
            draw(ctx)
            assert_planes(ctx, planes, f"with the tables, {path}, pass {rnd}")
            assert_emission_planes(ctx, E, f"pixel emission, {path}, pass {rnd}", W, H)
            assert np.array_equal(ctx.download_pixel_gloss(), cls), (path, rnd)
        ctx.set_dynamic_draw(0)
        draw(ctx)
        assert_planes(ctx, planes_s, f"flag off, {path}")
        assert_emission_planes(ctx, E_off, f"pixel emission, flag off, {path}", W, H)
        assert np.array_equal(ctx.download_pixel_gloss(), cls_off), path


@pytest.mark.parametrize("w,h", ddc.FRAMES)
def test_textured_flag_off_is_the_static_textured_mesh(vct, room, w, h):
    depth, planes = room["S", w, 1]
    assert (bits(planes) != bits(room["A", w, 1][1])).any(0).sum() >= (300 if w == W else 5)
    with textured_ctx(vct, room, w, h, "direct", 1) as ctx:
        ctx.set_dynamic_mesh(*room["A"])
        for flags in (0, BOTH, 0):
            ctx.set_dynamic_draw(flags, ddc.SPECULAR)
            draw(ctx, w, h)
            k = "A" if flags else "S"
            assert_map(ctx, room[k, w, 1][0], f"flags {flags}")
            assert_planes(ctx, room[k, w, 1][1], f"flags {flags}", None, w, h)


# ---- B. EMIS and the DYN bounce at other grids and under the IEEE-divide march -----------------------------------------------
GRIDS = (8, 16, 128)
EMIS_MIN = {8: (10, 9, 9), 16: (40, 30, 36), 128: (917, 907, 485)}       # (D' != D) voxels, saturating, ONE != EM
BOUNCE_MIN = {8: 10, 16: 50, 128: 1000}                                    # voxels telling whose attributes shade the layer
_BOUNCE = {}


def emis_world(oracle, v):
    w = grid_world(oracle, v)
    if "D'" not in w:
        for k in "AB":
            w["DEm", k] = de.dem(oracle, w[k][0], w[k][1], V=v)
            w["D'", k] = de.add(w["D", k][0], w["DEm", k])
        w["one"] = de.add(w["D", "A"][0], de.dem(oracle, w["A"][0], w["A"][1], de.ONE, V=v))
    return w


def bounce_want(oracle, v, k="A", l0=None, tag=None):
    key = (v, k, tag)
    if key not in _BOUNCE:
        w = grid_world(oracle, v)
        _BOUNCE[key] = db.expected(oracle, w["D", k], w["S"], l0=l0, p=oracle.default_params(v, G=dc.G))
    return _BOUNCE[key]


@pytest.mark.parametrize("attributes", [1, 0])
@pytest.mark.parametrize("v", GRIDS)
def test_emission_at_other_grid_sizes(vct, oracle, v, attributes):
    w = emis_world(oracle, v)
    S, D, Dp = w["S"][0], w["D", "A"][0], w["D'", "A"]
    changed, saturating, one_differs = EMIS_MIN[v]
    n = de.non_degeneracy(D, w["DEm", "A"])
    assert (Dp != D).any(-1).sum() >= changed and n["saturating"] >= saturating and n["same_alpha"], n
    if v == 128:
        de.assert_non_degenerate(D, w["DEm", "A"])
    assert (w["one"] != Dp).any(-1).sum() >= one_differs
    with grid_ctx(vct, w, v, attributes) as ctx:
        ctx.set_dynamic_mesh(*w["A"])
        ctx.set_dynamic_emission(de.EM)
        for k in "ABA":
            ctx.update_dynamic_positions(w[k][0])
            run_pass(ctx)
            assert_pass(oracle, ctx, w["D'", k], S, f"{v}^3, attributes={attributes}, at {k}")
        ctx.set_dynamic_emission(de.ONE)
        run_pass(ctx)
        assert_pass(oracle, ctx, w["one"], S, f"{v}^3, material 2 alone")
        ctx.set_dynamic_emission(None)
        run_pass(ctx)
        assert_pass(oracle, ctx, D, S, f"{v}^3, detached")


@pytest.mark.parametrize("v", GRIDS)
def test_bounce_at_other_grid_sizes(vct, oracle, v):
    w = grid_world(oracle, v)
    l1, steps = bounce_want(oracle, v)
    wrong, wrong_steps = db.static_attributes(oracle, w["D", "A"], w["S"], p=oracle.default_params(v, G=dc.G))
    assert db.differing(l1, wrong).sum() >= BOUNCE_MIN[v] and steps != wrong_steps
    with grid_ctx(vct, w, v, 1) as ctx:
        ctx.set_dynamic_bounce(True)
        ctx.set_dynamic_mesh(*w["A"])
        run_pass(ctx)
        ctx.bounce()
        assert_bounced(oracle, ctx, l1, steps, f"{v}^3 at A")
        if v == 128:
            ctx.bounce()
            assert_bounced(oracle, ctx, l1, steps, "128^3, the second bounce back to back")
            lb, steps_b = bounce_want(oracle, v, "B")
            assert db.differing(lb, l1).sum() >= 1000
            ctx.update_dynamic_positions(w["B"][0])
            run_pass(ctx)
            ctx.bounce()
            assert_bounced(oracle, ctx, lb, steps_b, "128^3 at B")


def test_emission_and_bounce_together_at_128(vct, oracle):
    v = 128
    w = emis_world(oracle, v)
    l0 = dc.merge(w["D'", "A"], w["S"][0])
    l1, steps = bounce_want(oracle, v, "A", l0=l0, tag="D'")
    plain, _ = bounce_want(oracle, v)
    assert db.differing(l1, plain).sum() >= 300 and db.differing(l1, l0).sum() >= 2000
    with grid_ctx(vct, w, v, 1) as ctx:
        ctx.set_dynamic_bounce(True)
        ctx.set_dynamic_mesh(*w["A"])
        ctx.set_dynamic_emission(de.EM)
        run_pass(ctx)
        assert_pass(oracle, ctx, w["D'", "A"], w["S"][0], "128^3, bounce 0")
        ctx.bounce()
        assert_bounced(oracle, ctx, l1, steps, "128^3, bounce over the chain holding D'")
        assert np.array_equal(ctx.download_dynamic_voxels()[0], w["D'", "A"])


@pytest.mark.parametrize("wrap", [1, 0])
@pytest.mark.parametrize("scene", ["world64", "dense16"])
def test_bounce_under_the_ieee_divide_march(vct, oracle, scene, wrap):
    """max_alpha 0.97: 1 - max_alpha < 2^-5, so the FASTDIV = 0 kernels run, here with the DYN argument block; the dense
    16^3 scene overflows the voxel list (k_bounce_bricks)."""
    v = 64 if scene == "world64" else 16
    static = dc.static_scene() if scene == "world64" else db.dense16_static()
    mesh = dc.dynamic_mesh(dc.A)
    p = oracle.default_params(v, G=dc.G, wrap_repeat=wrap, max_alpha=0.97)
    S3, D3 = dc.layer(oracle, *static, V=v), dc.layer(oracle, *mesh, V=v)
    d = D3[0][..., 3] > 0
    if scene == "dense16":
        assert (dc.merge(D3[0], S3[0])[..., 3] > 0).sum() > v ** 3 // 8 and d.sum() >= 50
    else:
        dc.assert_non_degenerate(D3[0], S3[0])
    l1, steps = db.expected(oracle, D3, S3, p=p)
    wrong, wrong_steps = db.static_attributes(oracle, D3, S3, p=p)
    assert steps != wrong_steps and db.differing(l1, wrong).sum() >= (300 if v == 64 else 10)
    default, default_steps = db.expected(oracle, D3, S3, p=oracle.default_params(v, G=dc.G, wrap_repeat=wrap))
    assert steps > default_steps and db.differing(l1, default).sum() >= 10       # max_alpha shows in the result
    with vct.Context(dc.config(vct, v, wrap_repeat=wrap, max_alpha=0.97)) as ctx:
        assert expected_form(ctx) == IEEE
        ctx.upload_triangles(*static)
        ctx.set_dynamic_bounce(True)
        ctx.set_dynamic_mesh(*mesh)
        run_pass(ctx)
        for rnd in range(2):
            ctx.bounce()
            assert form_of(ctx) == IEEE
            assert ctx.dynamic_bounce is True and ctx.dynamic_info()["ntri"] == dc.NTRI and ctx.dynamic_info()["bricks_used"] > 0
            assert_bounced(oracle, ctx, l1, steps, f"{scene}, wrap_repeat={wrap}, IEEE divide, bounce {rnd}")
