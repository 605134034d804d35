"""CPU: the premises of tests/test_gpu_dynamic_draw.py, held on the CPU checker's output for the concatenated mesh of
tests/dyndrawcases.py -- what keeps the GPU comparisons from passing vacuously -- and those of the textured room of
tests/test_gpu_dynamic_features.py and of the readers of tests/test_gpu_dynamic_readers.py."""
import numpy as np
import pytest

import dyndrawcases as ddc

W, H, S = ddc.W, ddc.H, ddc.SHADOW


@pytest.fixture(scope="module")
def world(oracle):
    static, dyn = ddc.static_mesh(), ddc.object_mesh("A")
    cat = ddc.concatenated(static, dyn)
    w = dict(static=static, dyn=dyn, cat=cat)
    w["depth_cat"], w["planes_cat"] = ddc.reference(oracle, cat, W, H)
    w["depth_static"], w["planes_static"] = ddc.reference(oracle, static, W, H)
    alone = ddc.concatenated(tuple(a[:0] for a in static[:4]) + (tuple(f[:0] for f in static[4]),), dyn)
    w["depth_dyn"], _ = ddc.reference(oracle, alone, W, H)
    return w


def test_palette_names_the_owner(world):
    salb = world["static"][2]
    assert (salb[:, 0] < 0.5).all() and (ddc.PALETTE[:, 0] >= 0.6).all()
    for c in ddc.PALETTE[:, :3]:
        assert not (np.abs(salb[:, :3] - c).max(1) == 0).any()
    # ... and the fourth values of the palette would fail an alpha test: the definition has none
    assert (ddc.PALETTE[:, 3] < 0.5).sum() >= 2


def test_object_is_seen_hidden_and_hiding(world):
    dyn_pix = ddc.owner_is_dynamic(world["planes_cat"])
    static_before = world["planes_static"][18] >= 0.5
    assert dyn_pix.sum() >= 300, dyn_pix.sum()
    assert (dyn_pix & static_before).sum() >= 300                  # the object hides static surface
    assert (world["planes_cat"][18][dyn_pix] == 1.0).all()          # alpha plane 1 whatever the table says
    # partly hidden behind the static occluder: pixels the object alone would own show the occluder's colour
    pos, mat, alb = world["dyn"]
    big = ddc.PARTS["BIG"]
    none = tuple(a[:0] for a in world["static"][:4]) + (tuple(f[:0] for f in world["static"][4]),)
    from oracle import pyoracle
    _, alone = ddc.reference(pyoracle, ddc.concatenated(none, (pos[big], mat[big], alb)), W, H, with_shadow=False)
    would = alone[18] >= 0.5
    occluder_red = world["static"][2][4:6, 0]
    hidden = would & np.isin(world["planes_cat"][15], occluder_red)
    assert hidden.sum() >= 100 and (would & dyn_pix).sum() >= 300, (hidden.sum(), (would & dyn_pix).sum())


def test_exact_depth_tie_goes_to_the_static_mesh(world, oracle):
    pos, mat, alb = world["dyn"]
    dup = ddc.PARTS["DUP"][0]
    assert np.array_equal(pos[dup], world["static"][0][6])
    tie_red = world["static"][2][6, 0]
    owned = (world["planes_cat"][18] >= 0.5) & (world["planes_cat"][15] == tie_red)
    assert owned.sum() >= 50
    # with the static triangle removed the same pixels show the dynamic duplicate: the tie is real
    keep = np.arange(world["static"][0].shape[0]) != 6
    st = tuple(a[keep] for a in world["static"][:2]) + world["static"][2:4] + (tuple(f[keep] for f in world["static"][4]),)
    _, planes = ddc.reference(oracle, ddc.concatenated(st, world["dyn"]), W, H)
    assert ddc.owner_is_dynamic(planes)[owned].all()
    assert np.array_equal(planes[0:3][:, owned].view(np.uint32), world["planes_cat"][0:3][:, owned].view(np.uint32))


def test_shadow_map_premises(world):
    dc_, ds, dd = world["depth_cat"], world["depth_static"], world["depth_dyn"]
    assert (dc_.view(np.uint32) != ds.view(np.uint32)).sum() >= 300
    assert np.array_equal(dc_, np.minimum(ds, dd))
    # the object's shadow reaches the frame: static pixels whose PCF plane changes
    stat = ~ddc.owner_is_dynamic(world["planes_cat"]) & (world["planes_cat"][18] >= 0.5)
    assert (world["planes_cat"][22][stat] != world["planes_static"][22][stat]).sum() >= 50


def test_work_classes_and_near_clip(world):
    pos = world["dyn"][0]
    for (w, h, vp, what) in ((W, H, ddc.camera(W, H), "frame"), (S, S, ddc.light_vp(), "shadow map")):
        classes = {ddc.work_class(b) for bs in ddc.boxes(pos, vp, w, h) for b in bs}
        assert classes == {0, 1, 2, 3}, (what, classes)
    bx = ddc.boxes(pos, ddc.camera(W, H), W, H)
    for name, cls in (("BIG", 3), ("WAVE", 2), ("GROUP", 1), ("SMALL", 0)):
        for t in ddc.PARTS[name]:
            assert [ddc.work_class(b) for b in bx[t]] == [cls], (name, bx[t])
    # away from the class bounds: the float64 restatement of the fp32 set-up cannot flip a class
    for bs in (bx[t] for n in ("BIG", "WAVE", "GROUP", "SMALL") for t in ddc.PARTS[n]):
        for b in bs:
            assert all(abs(b - lim) > 0.1 * lim for lim in (ddc.SMALL, ddc.GROUP, ddc.WAVE)), b
    near = ddc.PARTS["NEAR"][0]
    assert len(bx[near]) == 2, bx[near]


# ---- the textured room of tests/test_gpu_dynamic_features.py ---------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def without_alpha_tested(static):
    """The room without the occluder and TIE, the triangles whose diffuse map is the lace."""
    keep = np.ones(static[0].shape[0], bool)
    keep[4:7] = False
    return (static[0][keep], np.arange(keep.sum(), dtype=np.int32), static[2][keep], static[3][keep],
            tuple(f[keep] for f in static[4]))


@pytest.fixture(scope="module")
def textured(oracle, world):
    dyn = world["dyn"]
    tex = ddc.textured_cat(dyn[0].shape[0], dyn[2].shape[0])
    t = dict(tex=tex)
    for w, h in ddc.FRAMES:
        t[w, "plain"] = ddc.reference(oracle, world["cat"], w, h)
        for mip in (True, False):
            t[w, mip] = ddc.reference(oracle, world["cat"], w, h, tex=tex, mipmaps=mip)
    return t


def test_textured_room_inputs():
    texs, uv, mt = ddc.room_textures(), ddc.room_uv(), ddc.room_mat_tex()
    assert [t.shape for t in texs] == [(8, 16, 4), (8, 8, 4), (4, 4, 4), (16, 16, 4)]
    assert all(t[..., 0].max() < 128 for t in texs)                       # owner_is_dynamic still tells the owner
    lace = texs[ddc.LACE_TEX][..., 3]
    assert set(np.unique(lace)) == {0, 255} and (lace == 0).sum() == 21       # sums 0, 3, .., 12: 1 + 4 + 7 + 6 + 3
    assert all((t[..., 3] == 255).all() for i, t in enumerate(texs) if i != ddc.LACE_TEX)
    static = ddc.static_mesh()
    assert uv.shape == (static[0].shape[0], 6) and mt.shape == (static[2].shape[0], 3)
    assert (mt[7:] == -1).all() and not uv[7:].any()                       # the LOW patch stays untextured
    assert (mt[:, 0] >= 0).sum() == 7 and (mt[:, 1] >= 0).sum() == 3 and (mt[:, 2] >= 0).sum() == 2
    u, m, _ = ddc.textured_cat(5, 3)
    assert not u[9:].any() and (m[9:] == -1).all() and u.shape[0] == 14 and m.shape[0] == 12


def test_textured_holes_show_the_dynamic_mesh(oracle, world, textured):
    W_ = ddc.W
    (_, plain), (_, tx) = textured[W_, "plain"], textured[W_, True]
    own_plain, own = ddc.owner_is_dynamic(plain), ddc.owner_is_dynamic(tx)
    holes = own & ~own_plain & (plain[18] >= 0.5)
    assert holes.sum() >= 150, holes.sum()                              # holes in the occluder and in TIE (measured: 348)
    assert (own_plain & ~own).sum() == 0
    for mip in (True, False):                                           # each sampler state is held on its own
        _, p = textured[W_, mip]
        o = ddc.owner_is_dynamic(p)
        # a dynamic pixel's 23 planes know nothing of textures: where the untextured room shows the object too, its planes;
        # in a hole, the planes of the untextured room without the alpha-tested triangles (under the same shadow map)
        assert np.array_equal(bits(p)[:, o & own_plain], bits(plain)[:, o & own_plain])
        open_room = ddc.concatenated(without_alpha_tested(world["static"]), world["dyn"])
        through = oracle.render_gbuffer(ddc.mesh_of(oracle, open_room), ddc.camera(W_, ddc.H), W_, ddc.H,
                                        textured[W_, mip][0], ddc.light_vp())
        assert ddc.owner_is_dynamic(through)[o].all()
        assert np.array_equal(bits(p)[:, o], bits(through)[:, o])
        assert (p[18][o] == 1.0).all()


def test_textured_tie_goes_to_the_static_mesh_where_its_alpha_test_keeps_it(oracle, world):
    """DUP as the only dynamic triangle: without textures it owns nothing; with the lace on TIE it owns exactly the pixels
    of TIE that the alpha test discards."""
    pos, mat, alb = world["dyn"]
    idx = ddc.PARTS["DUP"]
    cat = ddc.concatenated(world["static"], (pos[idx], mat[idx], alb))
    tex = ddc.textured_cat(1, alb.shape[0])
    _, plain = ddc.reference(oracle, cat, W, H)
    tie = (plain[18] >= 0.5) & (plain[15] == world["static"][2][6, 0])
    assert ddc.owner_is_dynamic(plain).sum() == 0 and tie.sum() >= 300
    for mip in (True, False):
        _, p = ddc.reference(oracle, cat, W, H, tex=tex, mipmaps=mip)
        own = ddc.owner_is_dynamic(p)
        assert own.sum() >= 50, own.sum()                              # measured: 116
        assert not (own & ~tie).any()                                   # only where TIE was
        kept = tie & ~own
        assert kept.sum() >= 200
        # the kept pixels are TIE's: its diffuse map's colour (red < 0.5), its depth; the others the duplicate's flat colour
        assert (p[15][kept] < 0.55).all() and np.array_equal(bits(p[0:3][:, kept]), bits(plain[0:3][:, kept]))
        assert np.array_equal(bits(p[0:3][:, own]), bits(plain[0:3][:, own]))          # the very same positions: a real tie


def test_textures_show_on_static_pixels_and_leave_the_shadow_map_alone(textured):
    for (w, _), (changed, mips) in zip(ddc.FRAMES, ((1000, 500), (20, 20))):
        (d0, plain), (d1, tx), (d2, nomip) = textured[w, "plain"], textured[w, True], textured[w, False]
        # the shadow pass does not alpha-test and reads no texture
        assert np.array_equal(bits(d0), bits(d1)) and np.array_equal(bits(d0), bits(d2))
        own = ddc.owner_is_dynamic(tx)
        assert np.array_equal(own, ddc.owner_is_dynamic(nomip))
        assert ((bits(tx) != bits(plain)).any(0) & ~own).sum() >= changed
        assert ((bits(tx) != bits(nomip)).any(0) & ~own).sum() >= mips
        # bump-mapped normals (the floor's height map) and a mapped specular colour (the wall, TIE) are in the frame
        st = ~own & (tx[18] >= 0.5)
        assert ((bits(tx[3:15]) != bits(plain[3:15])).any(0) & st).sum() >= (200 if w == ddc.W else 5)
        assert ((bits(tx[19:22]) != bits(plain[19:22])).any(0) & st).sum() >= (200 if w == ddc.W else 5)


def test_offenders_and_frames():
    off = ddc.offenders()
    assert not ddc.in_contract(off).any()
    v = ddc.first_beyond()
    lim = np.float32(ddc.VERTEX_LIMIT_GRIDS) * np.float32(ddc.G)
    assert np.float32(v * np.float32(ddc.MS)) > lim and np.float32(np.nextafter(v, np.float32(0)) * np.float32(ddc.MS)) <= lim
    assert ddc.in_contract(ddc.object_mesh("A")[0]).all() and ddc.in_contract(ddc.object_mesh("B")[0]).all()
    n, t, b = ddc.dynamic_frames(ddc.object_mesh("A")[0])
    for f in (n, t, b):
        assert np.isfinite(f).all() and np.allclose(np.linalg.norm(f.reshape(-1, 3, 3)[:, 0], axis=1), 1.0, atol=1e-5)
    assert np.abs((n.reshape(-1, 3, 3)[:, 0] * t.reshape(-1, 3, 3)[:, 0]).sum(1)).max() < 1e-5


# ---- the readers of tests/test_gpu_dynamic_readers.py -------------------------------------------------------------------------------
def test_object_lights_reach_dynamic_and_static_pixels(oracle, world):
    import lights_ref as lr
    pos, mat, alb, spec, frames = world["static"]
    cat = ddc.concatenated((pos, mat, alb, np.zeros_like(spec), frames), world["dyn"], specular=None)
    _, planes = ddc.reference(oracle, cat, W, H)
    assert not planes[19:22].any()                                  # no specular colour anywhere: the lit planes hold no powf
    own = ddc.owner_is_dynamic(planes)
    lights = ddc.object_lights()
    assert len(lights) == 8 and sum(1 for l in lights if l.get("flags", 0)) >= 3
    lit = lr.lit_planes(planes, lights, (0.0, 0.0, 0.0), 20.0)
    reach = [int(((lr.lit_planes(planes, [l], (0.0, 0.0, 0.0), 20.0) > 0).any(0) & own).sum()) for l in lights]
    print((lit[:, own] > 0).any(0).sum(), (lit[:, ~own] > 0).any(0).sum(), reach)
    assert (lit[:, own] > 0).any(0).sum() >= 100 and (lit[:, ~own] > 0).any(0).sum() >= 100
    assert sum(r >= 10 for r in reach) >= 4


def test_adjacent_dynamic_faces_split_the_half_rate_quads(world):
    """Rate 2 over the drawn planes at one world unit per voxel: quads that straddle two flat-shaded dynamic triangles fail
    the normal test, so dynamic pixels are in the fill set (they march their own cones), beside anchors and interpolated ones."""
    import diffuse_rate_ref as dr
    planes = world["planes_cat"]
    own = ddc.owner_is_dynamic(planes)
    cls = dr.classify(planes, W, H, np.float32(1.0))
    interp = cls["alive"] & ~cls["marched"]
    print(int((cls["fill"] & own).sum()), int((interp & own).sum()), int((cls["anchor"] & own).sum()), int((interp & ~own).sum()))
    assert (cls["fill"] & own).sum() >= 20
    assert (interp & own).sum() >= 300 and (cls["anchor"] & own).sum() >= 300 and (interp & ~own).sum() >= 1000
