"""CPU: the premises of tests/test_gpu_dynamic_draw.py, held on the CPU checker's output for the concatenated mesh of
tests/dyndrawcases.py -- what keeps the GPU comparisons from passing vacuously."""
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
