"""GPU: the half-rate diffuse gather (include/vct.h vct_set_diffuse_rate(ctx, 2)) against the numpy restatement
(tests/diffuse_rate_ref.py) applied to the oracle's full-rate cones.  Every case first shows, on the restatement
alone, that it holds what it claims to exercise."""
import numpy as np
import pytest

import components_ref as cr
import diffuse_rate_ref as dr
import synth

pytestmark = pytest.mark.gpu

CAM, LIGHT = (3.0, 4.0, -2.0), (0.2, 1.0, 0.3)
ALL_AOV = cr.AOV_INDIRECT_DIFFUSE | cr.AOV_INDIRECT_SPECULAR | cr.AOV_DIRECT


@pytest.fixture(scope="module")
def vct():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import vctpkg
    return vctpkg.load()


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle
    return pyoracle


_chains = {}


def _case(oracle, V, w, h, planes):
    if V not in _chains:
        _chains[V] = oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.06))
    p = oracle.default_params(V, camera_pos=CAM, light_dir=LIGHT)
    ref = oracle.trace(p, _chains[V], planes, nthreads=8, want_cones=True)
    return dict(V=V, w=w, h=h, chain=_chains[V], planes=planes, params=p, ref=ref, vs=np.float32(p.G) / np.float32(V))


@pytest.fixture(scope="module")
def floor(oracle):
    return _case(oracle, 64, 256, 192, synth.coherent_gbuffer(256, 192))


@pytest.fixture(scope="module")
def mixed(oracle):
    return _case(oracle, 32, 128, 96, dr.mixed_gbuffer(128, 96))


def _ctx(vct, s, **kw):
    ctx = vct.Context(vct.default_config(voxel_dim=s["V"], width=s["w"], height=s["h"], **kw))
    ctx.set_camera_position(CAM)
    ctx.set_light_direction(LIGHT)
    ctx.upload_chain(s["chain"])
    return ctx


def _restate(s, mask=cr.SHOW_ALL, aov=0):
    p = s["params"]
    return dr.restate(s["planes"], s["w"], s["h"], s["vs"], s["ref"], CAM, LIGHT, p.ambient_factor, p.shininess, mask, aov)


def _f16(u16):
    return np.asarray(u16, np.uint16).reshape(-1, 4)


def _assert_f16_matches(vct, got, want32, what):
    """test_gpu_components' bars: relative L2 <= 1e-4 and >= 99.9 % of the fp16 values equal."""
    want16 = cr.to_f16_bits(want32)
    l2 = synth.rel_l2(vct.half_to_float(_f16(got)), vct.half_to_float(want16))
    eq = (_f16(got) == want16).mean()
    print(f"{what}: rel-L2 {l2:.3e}, fp16 equal {eq:.6f}")
    assert l2 <= 1e-4, what
    assert eq >= 0.999, what


def _check_against_restatement(vct, ctx, s, want, what):
    """Frame, marched set, cones on it, step count and marched_pixels of the rate-2 trace just made by a context with
    debug_outputs."""
    frame = ctx.download_frame()
    st, cones = ctx.steps(), ctx.cones()
    got_marched = st[:, :6].astype(np.int64).sum(1) > 0
    stepping = want["steps"][:, :6].astype(np.int64).sum(1) > 0        # (a marched pixel whose cones all take 0 steps shows none)
    assert np.array_equal(got_marched, stepping), what
    assert np.array_equal(st, want["steps"]), what
    alive = want["cls"]["alive"]
    assert np.array_equal(cones[alive], want["cones"][alive]), what
    assert ctx.last_step_count() == want["total_steps"], what
    assert ctx.diffuse_rate() == (2, int(want["marched"].sum())), what
    _assert_f16_matches(vct, frame, want["rgba32f"], what)


def test_coherent_floor(vct, floor):
    want = _restate(floor, aov=cr.AOV_INDIRECT_DIFFUSE)
    cls = want["cls"]
    cw, ch = 128, 96
    assert np.array_equal(cls["marched"], cls["anchor"]) and cls["anchor"].sum() == cw * ch and not cls["fill"].any()
    assert (want["steps"][cls["anchor"], :6].astype(np.int64).sum(1) > 0).all()
    with _ctx(vct, floor, debug_outputs=1) as ctx:
        ctx.set_diffuse_rate(2)
        ctx.set_aov_outputs(vct.AOV_INDIRECT_DIFFUSE)
        ctx.trace(floor["planes"])
        _check_against_restatement(vct, ctx, floor, want, "floor")
        assert ctx.diffuse_rate() == (2, cw * ch)
        anchors = cls["anchor"]
        assert np.array_equal(ctx.cones()[anchors], floor["ref"]["cones"][anchors])
        _assert_f16_matches(vct, ctx.download_aov(vct.AOV_INDIRECT_DIFFUSE), want["ind"], "floor indirect diffuse")
        assert ctx.last_step_count() < floor["ref"]["total_steps"]


def test_mixed_case(vct, mixed):
    want = _restate(mixed, aov=cr.AOV_INDIRECT_DIFFUSE)
    cls = want["cls"]
    interp = cls["alive"] & ~cls["marched"]
    assert cls["anchor"].any() and cls["fill"].any()
    assert (interp & (cls["W"] == 16)).any() and (interp & (cls["W"] < 16)).any() and (cls["W"][interp] > 0).all()
    assert set(np.unique(cls["code"])) == {0, 1, 2, 3, dr.NO_ANCHOR}
    with _ctx(vct, mixed, debug_outputs=1) as ctx:
        ctx.set_diffuse_rate(2)
        ctx.set_aov_outputs(vct.AOV_INDIRECT_DIFFUSE)
        ctx.trace(mixed["planes"])
        _check_against_restatement(vct, ctx, mixed, want, "mixed")
        m = want["marched"]
        assert np.array_equal(ctx.cones()[m], mixed["ref"]["cones"][m])
        _assert_f16_matches(vct, ctx.download_aov(vct.AOV_INDIRECT_DIFFUSE), want["ind"], "mixed indirect diffuse")


def test_random_gbuffer_marches_everything(vct, oracle):
    """Unrelated neighbours: every live pixel is an anchor or a fill pixel, so the frame is rate 1's, bit for bit.  (Size
    and seed are ones at which no candidate passes the acceptance test by chance -- shown on the restatement first.)"""
    V, w, h = 64, 40, 24
    planes = synth.random_gbuffer(w * h, seed=4, discard_frac=0.05)
    cls = dr.classify(planes, w, h, np.float32(150.0) / np.float32(V))
    assert np.array_equal(cls["marched"], cls["alive"]) and cls["fill"].sum() > cls["anchor"].sum() > 0
    s = dict(V=V, w=w, h=h, chain=oracle.build_mips(synth.noise_volume(V, seed=7, occupancy=0.06)))
    with _ctx(vct, s) as ctx:
        base = ctx.trace(planes)
        steps = ctx.last_step_count()
        ctx.set_diffuse_rate(2)
        assert np.array_equal(ctx.trace(planes), base)
        assert ctx.last_step_count() == steps
        assert ctx.diffuse_rate() == (2, int(cls["alive"].sum()))


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 3), (17, 9), (37, 21), (40, 40)])
def test_sizes(vct, oracle, w, h):
    planes = synth.coherent_gbuffer(w, h, seed=3)
    planes[18, np.random.default_rng(w * 100 + h).uniform(size=w * h) < 0.1] = 0.0
    s = _case(oracle, 32, w, h, planes)
    want = _restate(s)
    assert w * h < 16 or (want["cls"]["alive"] & ~want["marched"]).any()
    with _ctx(vct, s, debug_outputs=1) as ctx:
        ctx.set_diffuse_rate(2)
        ctx.trace(planes)
        _check_against_restatement(vct, ctx, s, want, (w, h))


MASKS = [cr.SHOW_DIFFUSE | cr.SHOW_SPECULAR,                                       # direct only: nothing marched
         cr.SHOW_SPECULAR | cr.SHOW_INDIRECT_SPECULAR,                             # specular only
         cr.SHOW_INDIRECT_DIFFUSE,
         cr.SHOW_AMBIENT_OCCLUSION | cr.SHOW_DIFFUSE,
         cr.SHOW_ALL & ~cr.SHOW_INDIRECT_SPECULAR]


@pytest.mark.parametrize("mask", MASKS)
def test_masks(vct, mixed, mask):
    want = _restate(mixed, mask)
    dif, _ = cr.marched_groups(mask)
    assert want["marched"].any() == dif
    with _ctx(vct, mixed, debug_outputs=1) as ctx:
        ctx.set_diffuse_rate(2)
        ctx.set_lighting_components(mask)
        ctx.trace(mixed["planes"])
        _check_against_restatement(vct, ctx, mixed, want, mask)
        if mask == cr.SHOW_DIFFUSE | cr.SHOW_SPECULAR:
            assert ctx.last_step_count() == 0 and ctx.diffuse_rate() == (2, 0)


def test_all_outputs_on(vct, mixed):
    want = _restate(mixed, cr.SHOW_DIFFUSE, ALL_AOV)            # the outputs alone make both groups march
    assert want["marched"].any()
    alive = want["cls"]["alive"]
    with _ctx(vct, mixed, debug_outputs=1) as ctx:
        ctx.set_diffuse_rate(2)
        ctx.set_lighting_components(cr.SHOW_DIFFUSE)
        ctx.set_aov_outputs(ALL_AOV)
        ctx.trace(mixed["planes"])
        _check_against_restatement(vct, ctx, mixed, want, "outputs")
        _assert_f16_matches(vct, ctx.download_aov(vct.AOV_INDIRECT_DIFFUSE), want["ind"], "indirect diffuse")
        isp = _f16(ctx.download_aov(vct.AOV_INDIRECT_SPECULAR))
        assert np.array_equal(isp[alive], cr.to_f16_bits(mixed["ref"]["cones"][:, 6, :])[alive])
        _assert_f16_matches(vct, ctx.download_aov(vct.AOV_DIRECT), want["direct"], "direct")
        for bit in (vct.AOV_INDIRECT_DIFFUSE, vct.AOV_INDIRECT_SPECULAR, vct.AOV_DIRECT):
            assert (_f16(ctx.download_aov(bit))[~alive] == 0).all()


def test_back_to_rate_1(vct, mixed):
    with _ctx(vct, mixed) as ctx, _ctx(vct, mixed) as never:
        base = never.trace(mixed["planes"])
        steps = never.last_step_count()
        ctx.set_diffuse_rate(2)
        half = ctx.trace(mixed["planes"])
        assert not np.array_equal(half, base) and ctx.last_step_count() < steps
        ctx.set_diffuse_rate(1)
        assert np.array_equal(ctx.trace(mixed["planes"]), base)
        assert ctx.last_step_count() == steps == mixed["ref"]["total_steps"]
        assert ctx.diffuse_rate() == (1, 0)
        assert ctx.last_row_steps().sum() == steps
        ctx.set_diffuse_rate(2)                                   # and forth again: fresh buffers, the same frame
        assert np.array_equal(ctx.trace(mixed["planes"]), half)


def test_two_frame_slots(vct, mixed):
    with _ctx(vct, mixed) as ctx:
        ctx.set_diffuse_rate(2)
        one = ctx.trace(mixed["planes"])
        steps, marched = ctx.last_step_count(), ctx.diffuse_rate()[1]
        ctx.set_frames_in_flight(2)                               # the second slot gets its own buffers
        for k in range(4):
            ctx.select_frame_slot(k & 1)
            ctx.trace(mixed["planes"])
        ctx.synchronize()
        for slot in (0, 1):
            ctx.select_frame_slot(slot)
            assert np.array_equal(ctx.download_frame(), one)
            assert ctx.last_step_count() == steps and ctx.diffuse_rate() == (2, marched)
        ctx.set_diffuse_rate(1)                                   # frees both slots' buffers
        ctx.set_diffuse_rate(2)                                   # ... and allocates them for both
        for slot in (1, 0):
            ctx.select_frame_slot(slot)
            assert np.array_equal(ctx.trace(mixed["planes"]), one)
        ctx.set_frames_in_flight(1)
        assert np.array_equal(ctx.trace(mixed["planes"]), one)


def test_gi_pass_equals_staged_calls(vct):
    from voxel_cone_tracing_amd import scene as sc
    V, w, h, S = 64, 160, 96, 512
    light = (0.0, 1.0, 0.25)
    cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
    lvp, vp = sc.light_view_proj(light), sc.camera_view_proj(cam, w, h)
    with vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S)) as ctx:
        ctx.upload_scene(sc.Scene(sc.ATRIUM, 1.0, 1234))
        ctx.set_camera_position(tuple(cam.position))
        ctx.set_light_direction(light)
        ctx.render_shadow_map(lvp)
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        ctx.render_gbuffer(vp)
        full = ctx.trace_current()
        full_steps = ctx.last_step_count()
        ctx.set_diffuse_rate(2)
        staged = ctx.trace_current()
        steps, marched = ctx.last_step_count(), ctx.diffuse_rate()[1]
        alive = int((ctx.download_gbuffer()[18] >= 0.5).sum())
        assert 0 < marched < alive and steps < full_steps and not np.array_equal(staged, full)
        ctx.trace_resident(); ctx.synchronize()
        assert np.array_equal(ctx.download_frame(), staged)
        ctx.gi_pass(lvp, vp); ctx.synchronize()
        assert np.array_equal(ctx.download_frame(), staged)
        assert ctx.last_step_count() == steps and ctx.diffuse_rate() == (2, marched)
        ms = ctx.last_diffuse_rate_ms()
        assert len(ms) == 4 and all(m >= 0.0 for m in ms) and sum(ms) == pytest.approx(ctx.last_trace_ms(), abs=2e-3)


def test_refusals(vct, mixed):
    planes = mixed["planes"]
    VctError = vct.VctError
    with _ctx(vct, mixed) as ctx:
        for rate in (0, 3, 4, -1):
            with pytest.raises(VctError):
                ctx.set_diffuse_rate(rate)
        for variant in (1, 2, 3, 4):
            ctx.set_trace_variant(variant)
            with pytest.raises(VctError):
                ctx.set_diffuse_rate(2)
            ctx.set_trace_variant(0)
        ctx.set_footprint_records(True)
        with pytest.raises(VctError):
            ctx.set_diffuse_rate(2)
        ctx.set_footprint_records(False)
        ctx.comm_init(vct.comm_unique_id(), 0, 1)
        with pytest.raises(VctError):
            ctx.set_diffuse_rate(2)
        ctx.comm_destroy()
        assert ctx.diffuse_rate()[0] == 1
        ctx.set_diffuse_rate(2)
        want = ctx.trace(planes)
        for variant in (1, 2, 3, 4):
            with pytest.raises(VctError):
                ctx.set_trace_variant(variant)
        with pytest.raises(VctError):
            ctx.set_footprint_records(True)
        with pytest.raises(VctError):
            ctx.comm_init(vct.comm_unique_id(), 0, 1)
        with pytest.raises(VctError):
            ctx.trace(planes, rows=(0, 12))                          # vct_trace_slab, even of the whole frame
        with pytest.raises(VctError):
            ctx.trace(planes, rows=(2, 5))
        with pytest.raises(VctError):
            ctx.trace_gbuffer_rows(0, 12)
        with pytest.raises(VctError):
            ctx.trace_gbuffer_strided(0, 12, 2)
        with pytest.raises(VctError):
            ctx.last_row_steps()
        with pytest.raises(VctError):
            ctx.selftest_interleaved(2)
        assert ctx.diffuse_rate()[0] == 2
        assert np.array_equal(ctx.trace(planes), want)                # still usable, and still rate 2
        assert np.array_equal(ctx.trace_current(), want)
    with vct.Context(vct.default_config(voxel_dim=32, width=64, height=32, anisotropic_mips=1)) as ctx:
        with pytest.raises(VctError):
            ctx.set_diffuse_rate(2)
        ctx.set_diffuse_rate(1)
