"""Two frames in flight (vct_set_frames_in_flight / vct_select_frame_slot, include/vct.h): consecutive frames on
alternate frame slots -- own stream, G-buffer, frame, step counts -- must give exactly the frames the one-slot context
gives, whatever is in flight: a moving camera (G-buffer passes sharing the raster scratch), a moving light (stages that
rewrite the shadow map and the chain between frames), the one-call GI pass, slot-local vct_last_* values.
The reference has no counterpart in code: its frames overlap inside the GL driver (R/main.cpp:77-94 never waits)."""
import numpy as np
import pytest

import vctpkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available()
    return vctpkg.load()


def make(vct, w=328, h=200, V=64, detail=0.15, **cfg):
    from voxel_cone_tracing_amd import scene as sc
    scene = sc.Scene(sc.ATRIUM, detail, 1234)
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=512, **cfg))
    ctx.set_light_direction((0.0, 1.0, 0.25))
    ctx.upload_triangles(scene.pos, scene.material, scene.albedo)
    ctx.upload_mesh_attributes(*scene.frames(), scene.specular)
    return ctx, sc


def cameras(sc, w, h, n):
    out = []
    for k in range(n):
        cam = sc.default_camera(position=(-56.0 + 3.0 * k, -9.0 + 0.5 * k, 2.0 - 0.7 * k), yaw=4.0 * k, pitch=8.0 - k)
        out.append((tuple(cam.position), sc.camera_view_proj(cam, w, h)))
    return out


def lights(n):
    return [(0.15 * k, 1.0, 0.25 - 0.1 * k) for k in range(n)]


@pytest.mark.parametrize("size", ["small", "configs[1]"])
def test_moving_camera_two_frames_in_flight_equals_one(vct, size):
    """(configs[1]: BASELINE's headline size -- the 257 k-triangle atrium, 256^3, 1920x1080 -- where a frame's raster and
    trace really are in flight beside the previous frame's.)"""
    w, h, n = (328, 200, 7) if size == "small" else (1920, 1080, 7)
    ctx, sc = make(vct, w, h) if size == "small" else make(vct, w, h, V=256, detail=1.0)
    ctx.render_shadow_map(sc.light_view_proj((0.0, 1.0, 0.25)))
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    cams = cameras(sc, w, h, n)
    want, want_steps = [], []
    for pos, vp in cams:                       # one slot: frame after frame, read back each
        ctx.set_camera_position(pos)
        ctx.render_gbuffer(vp)
        want.append(ctx.trace_current())
        want_steps.append(ctx.last_step_count())
    ctx.set_frames_in_flight(2)
    assert ctx.frames_in_flight() == (2, 0)
    got = [None] * n
    # frames k and k + 1 are both issued before frame k is read back: two in flight at every moment
    for k, (pos, vp) in enumerate(cams):
        ctx.select_frame_slot(k & 1)
        ctx.set_camera_position(pos)
        ctx.render_gbuffer(vp)
        ctx.trace_resident()
        if k >= 1:
            ctx.select_frame_slot((k - 1) & 1)
            got[k - 1] = ctx.download_frame()
            assert ctx.last_step_count() == want_steps[k - 1]          # the slot's own step counts
    ctx.select_frame_slot((n - 1) & 1)
    got[n - 1] = ctx.download_frame()
    for k in range(n):
        assert np.array_equal(got[k], want[k]), f"frame {k}"
    # many frames without any read-back in between (nothing throttles the host), then both slots' last frames
    for rep in range(40):
        k = rep % n
        ctx.select_frame_slot(rep & 1)
        ctx.set_camera_position(cams[k][0])
        ctx.render_gbuffer(cams[k][1])
        ctx.trace_resident()
    ctx.synchronize()
    ctx.select_frame_slot(1)
    assert np.array_equal(ctx.download_frame(), want[39 % n])
    ctx.select_frame_slot(0)
    assert np.array_equal(ctx.download_frame(), want[38 % n])
    # back to one slot: still the same frames
    ctx.set_frames_in_flight(1)
    assert ctx.frames_in_flight() == (1, 0)
    ctx.set_camera_position(cams[2][0]); ctx.render_gbuffer(cams[2][1])
    assert np.array_equal(ctx.trace_current(), want[2])
    ctx.close()


def test_moving_light_between_frames_in_flight(vct):
    """Every frame re-renders the shadow map, re-voxelizes, injects and rebuilds the mips -- stages that rewrite what the
    other slot's trace is still reading.  The library orders them (pipeline_join + the switch-time wait): same frames."""
    w, h, n = 328, 200, 6
    ctx, sc = make(vct, w, h)
    cams = cameras(sc, w, h, n)
    Ls = lights(n)

    def frame(k):
        ctx.set_light_direction(Ls[k])
        ctx.set_camera_position(cams[k][0])
        ctx.render_shadow_map(sc.light_view_proj(Ls[k]))
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        ctx.render_gbuffer(cams[k][1])

    want = []
    for k in range(n):
        frame(k)
        want.append(ctx.trace_current())
    ctx.set_frames_in_flight(2)
    got = [None] * n
    for k in range(n):
        ctx.select_frame_slot(k & 1)
        frame(k)
        ctx.trace_resident()
        if k >= 1:
            ctx.select_frame_slot((k - 1) & 1)
            got[k - 1] = ctx.download_frame()
    ctx.select_frame_slot((n - 1) & 1)
    got[n - 1] = ctx.download_frame()
    for k in range(n):
        assert np.array_equal(got[k], want[k]), f"frame {k}"
    # the same through the one-call pass (its G-buffer raster runs on the auxiliary stream)
    got2 = [None] * n
    for k in range(n):
        ctx.select_frame_slot(k & 1)
        ctx.set_light_direction(Ls[k]); ctx.set_camera_position(cams[k][0])
        ctx.gi_pass(sc.light_view_proj(Ls[k]), cams[k][1])
        if k >= 1:
            ctx.select_frame_slot((k - 1) & 1)
            got2[k - 1] = ctx.download_frame()
    ctx.select_frame_slot((n - 1) & 1)
    got2[n - 1] = ctx.download_frame()
    for k in range(n):
        assert np.array_equal(got2[k], want[k]), f"gi_pass frame {k}"
    ctx.close()


def test_cone_apertures_change_between_frames_in_flight(vct):
    """A new step table is uploaded while the other slot's trace may still read the old one: the upload waits for it."""
    w, h = 328, 200
    ctx, sc = make(vct, w, h)
    ctx.render_shadow_map(sc.light_view_proj((0.0, 1.0, 0.25)))
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    pos, vp = cameras(sc, w, h, 1)[0]
    ctx.set_camera_position(pos)
    ctx.render_gbuffer(vp)
    aps = [(0.577, 0.07), (0.577, 0.2), (0.45, 0.105), (0.577, 0.07)]
    want = []
    for td, ts in aps:
        ctx.set_cone_apertures(td, ts)
        want.append(ctx.trace_current())
    ctx.set_frames_in_flight(2)
    ctx.select_frame_slot(1); ctx.render_gbuffer(vp); ctx.select_frame_slot(0)
    got = []
    for k, (td, ts) in enumerate(aps):
        ctx.select_frame_slot(k & 1)
        ctx.set_cone_apertures(td, ts)
        for _ in range(3):
            ctx.trace_resident()
    # (frames k = 2, 3 are the last of their slots)
    ctx.select_frame_slot(0); got.append(ctx.download_frame())
    ctx.select_frame_slot(1); got.append(ctx.download_frame())
    assert np.array_equal(got[0], want[2]) and np.array_equal(got[1], want[3])
    ctx.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_call_orders_give_what_a_synchronised_context_gives(vct, seed):
    """Producers (shadow map, voxelize / inject / mips, the one-call pass), G-buffer passes, traces, slot switches and
    read-backs in a random order on a two-slot context, against the same calls on a context that waits for the GPU after
    every call (nothing ever in flight there, so no ordering can go wrong).  What the library skips -- one cross-stream
    wait per slot selection, the switch's own wait counting as the join -- must not show.  (Checked against mutated
    builds: without the producers' joins, or without the wait of the slot switch, this test fails and the tests above do
    not -- at their sizes the GPU is done before the host's next call.  A build without the host-side drains passes
    everything: hipFree and the runtime's copy from pageable memory wait for the device by themselves -- 570 us of host
    time for "trace, switch, new apertures, trace" either way -- so the drains are a guarantee, not an observable.)"""
    rng = np.random.default_rng(seed)
    # a whole 1080p frame: its trace runs for a few hundred microseconds, long enough for the calls behind it to be issued
    # while it is still running
    w, h = 1920, 1080
    cams_n, lights_n = 5, 5
    # the call list first, so that the asynchronous context runs it without a pause
    ops = [("produce", 0)]
    slot, traced, has_gb = 0, [False, False], [False, False]
    for rnd in range(12):
        s0 = int(rng.integers(2))
        ops.append(("switch", s0)); slot = s0
        has_gb[slot] = True
        # a frame on slot s0, with or without new shared state in front of it ...
        r = rng.random()
        if r < 0.2 and traced[slot]:
            ops.append(("produce", int(rng.integers(lights_n))))        # new shared state and nothing else
        elif r < 0.4:
            ops.append(("gi", int(rng.integers(lights_n)), int(rng.integers(cams_n))))
            traced[slot] = True
        else:
            if r < 0.6:
                ops.append(("produce", int(rng.integers(lights_n))))
            ops.append(("gbuffer", int(rng.integers(cams_n)))); ops.append(("trace",))
            traced[slot] = True
        # ... and, while its trace is still running, the other slot: shared state rewritten at once (the case the joins are
        # for -- nothing was produced on s0 since the switch, so the switch itself waits for nothing), or only read
        ops.append(("switch", 1 - s0)); slot = 1 - s0
        if rng.random() < 0.3:
            ops.append(("apertures", int(rng.integers(3))))       # a new step table while the other slot's trace reads the old one
        if has_gb[slot] and rng.random() < 0.5:
            # the resident G-buffer traced again at once: if s0's frame came with new shared state, this trace must wait for
            # it (the switch's wait), and nothing but that wait makes it
            ops.append(("trace",)); traced[slot] = True
            ops.append(("read",))
        r = rng.random()
        if r < 0.12:
            # a new mesh: buffers the other slot's kernels may still read are freed and re-allocated (the host waits: drain)
            ops.append(("remesh", int(rng.integers(2)))); ops.append(("produce", int(rng.integers(lights_n))))
        elif r < 0.4:
            ops.append(("produce", int(rng.integers(lights_n))))
        elif r < 0.6:
            ops.append(("gi", int(rng.integers(lights_n)), int(rng.integers(cams_n)))); traced[slot] = has_gb[slot] = True
        if rng.random() < 0.6:
            ops.append(("gbuffer", int(rng.integers(cams_n)))); ops.append(("trace",)); traced[slot] = True
            has_gb[slot] = True
        if rng.random() < 0.5 and traced[slot]:
            ops.append(("read",))
        ops.append(("switch", s0)); slot = s0
        ops.append(("read",))

    def run(sync):
        c, sc = make(vct, w, h, V=128)
        meshes = [sc.Scene(sc.ATRIUM, 0.15, 1234), sc.Scene(sc.ATRIUM, 0.2, 99)]
        aps = [(0.577, 0.07), (0.577, 0.2), (0.45, 0.105)]
        cams = cameras(sc, w, h, cams_n)
        Ls = lights(lights_n)
        c.set_frames_in_flight(2)
        frames = []
        for op in ops:
            if op[0] == "produce":
                c.set_light_direction(Ls[op[1]])
                c.render_shadow_map(sc.light_view_proj(Ls[op[1]]))
                c.voxelize(); c.inject_light(); c.build_mips()
            elif op[0] == "gi":
                c.set_light_direction(Ls[op[1]]); c.set_camera_position(cams[op[2]][0])
                c.gi_pass(sc.light_view_proj(Ls[op[1]]), cams[op[2]][1])
            elif op[0] == "gbuffer":
                c.set_camera_position(cams[op[1]][0]); c.render_gbuffer(cams[op[1]][1])
            elif op[0] == "trace":
                c.trace_resident()
            elif op[0] == "switch":
                c.select_frame_slot(op[1])
            elif op[0] == "remesh":
                m = meshes[op[1]]
                c.upload_triangles(m.pos, m.material, m.albedo)
                c.upload_mesh_attributes(*m.frames(), m.specular)
            elif op[0] == "apertures":
                c.set_cone_apertures(*aps[op[1]])
            elif op[0] == "read":
                frames.append((c.download_frame(), c.last_step_count()))
            if sync:
                c.synchronize()
        c.close()
        return frames

    got, want = run(False), run(True)
    assert len(got) == len(want) >= 12
    for k, ((fa, sa), (fb, sb)) in enumerate(zip(got, want)):
        assert np.array_equal(fa, fb), f"seed {seed}: read-back {k} differs"
        assert sa == sb


@pytest.mark.parametrize("shape", ["frame", "shadow"])
def test_one_call_passes_back_to_back_into_their_own_targets(vct, shape):
    """vct_gi_pass forks its main draw onto a second stream: the draw must wait for the previous pass (fork), its shading
    kernel for the shadow map of THIS pass, the trace for the G-buffer (join).  Passes with a moving light and camera are
    issued back to back, each frame into its own device buffer (vct_set_frame_target), and compared with the same passes
    run one at a time.  "frame": 1080p, where the previous trace is still running when the next pass is issued; "shadow":
    a small frame under a 4096^2 shadow map of the whole atrium, where the main draw's visibility raster is done long
    before the shadow pass.  (Mutated builds: without the join "frame" fails, without the shadow wait "shadow" fails --
    neither was noticed by the small passes of the other tests, which run to completion before the host's next call.
    Without the fork wait everything passes: the shading kernel, the draw's only writer of the G-buffer, is already
    behind this pass's shadow map and thereby behind the previous trace; the wait stays as a guarantee.)"""
    import torch
    from voxel_cone_tracing_amd import scene as sc
    if shape == "frame":
        w, h, V, S, detail = 1920, 1080, 128, 512, 0.15
    else:
        w, h, V, S, detail = 200, 120, 64, 4096, 1.0
    scene = sc.Scene(sc.ATRIUM, detail, 1234)
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
    ctx.upload_triangles(scene.pos, scene.material, scene.albedo)
    ctx.upload_mesh_attributes(*scene.frames(), scene.specular)
    n = 6
    cams = cameras(sc, w, h, n)
    Ls = lights(n)

    def one(k):
        ctx.set_light_direction(Ls[k]); ctx.set_camera_position(cams[k][0])
        ctx.gi_pass(sc.light_view_proj(Ls[k]), cams[k][1])

    want = []
    for k in range(n):
        one(k)
        want.append(ctx.download_frame())
    targets = [torch.zeros((h, w, 4), dtype=torch.float16, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    for rep in range(3):
        for k in range(n):
            ctx.set_frame_target(targets[k].data_ptr())
            one(k)
        ctx.synchronize()
        for k in range(n):
            got = targets[k].cpu().numpy().view(np.uint16)
            assert np.array_equal(got.reshape(want[k].shape), want[k].view(np.uint16).reshape(want[k].shape)), f"{shape}: pass {k} (round {rep})"
    ctx.set_frame_target(None)
    ctx.close()


def test_trace_timing_switch(vct):
    """vct_set_trace_timing(0): march launches without the two timing events -- same frame, same step count;
    vct_last_trace_ms then refuses (it has nothing to read) until a launch is timed again."""
    w, h = 328, 200
    ctx, sc = make(vct, w, h)
    ctx.render_shadow_map(sc.light_view_proj((0.0, 1.0, 0.25)))
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    pos, vp = cameras(sc, w, h, 1)[0]
    ctx.set_camera_position(pos); ctx.render_gbuffer(vp)
    want = ctx.trace_current()
    steps = ctx.last_step_count()
    assert ctx.last_trace_ms() > 0.0
    ctx.set_trace_timing(False)
    ctx.trace_resident()
    assert np.array_equal(ctx.download_frame(), want) and ctx.last_step_count() == steps
    with pytest.raises(vct.VctError):
        ctx.last_trace_ms()
    ctx.set_frames_in_flight(2)                      # the switch is the context's, the "was timed" flag the slot's
    ctx.select_frame_slot(1); ctx.render_gbuffer(vp); ctx.trace_resident()
    with pytest.raises(vct.VctError):
        ctx.last_trace_ms()
    ctx.set_trace_timing(True)
    ctx.trace_resident()
    assert ctx.last_trace_ms() > 0.0 and np.array_equal(ctx.download_frame(), want)
    ctx.select_frame_slot(0)
    with pytest.raises(vct.VctError):
        ctx.last_trace_ms()                          # slot 0's last launch was not timed
    ctx.close()


def test_what_two_frames_in_flight_refuses(vct):
    ctx, sc = make(vct, 64, 48, 32)
    with pytest.raises(vct.VctError):
        ctx.set_frames_in_flight(3)
    with pytest.raises(vct.VctError):
        ctx.select_frame_slot(1)                     # one slot only
    ctx.set_frames_in_flight(2)
    with pytest.raises(vct.VctError):
        ctx.set_trace_variant(4)
    ctx.select_frame_slot(1)
    with pytest.raises(vct.VctError):                # slot 1 has no G-buffer yet
        ctx.trace_resident()
    ctx.set_frames_in_flight(1)                      # from slot 1: slot 0's set comes back
    assert ctx.frames_in_flight() == (1, 0)
    ctx.close()
    dbg, _ = make(vct, 64, 48, 32, debug_outputs=1)
    with pytest.raises(vct.VctError):
        dbg.set_frames_in_flight(2)
    dbg.close()


def test_rank_context_with_two_frames_in_flight(vct):
    """A rank of a multi-GPU frame (1-rank RCCL communicator: the native step's whole data path) with two frame slots: slab
    k + 1 is traced on the other slot's stream while slab k drains; every gathered frame equals the plain frame, with a
    moving camera, through both gather buffers and both slots; vct_comm_sync waits for both streams."""
    w, h, n = 328, 200, 6
    ctx, sc = make(vct, w, h)
    ctx.render_shadow_map(sc.light_view_proj((0.0, 1.0, 0.25)))
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    cams = cameras(sc, w, h, n)
    want = []
    for pos, vp in cams:
        ctx.set_camera_position(pos); ctx.render_gbuffer(vp)
        want.append(ctx.trace_current())
    ctx.comm_init(vct.comm_unique_id(), 0, 1)
    ctx.set_frames_in_flight(2)                      # (after the communicator exists: both orders are allowed)
    r0, r1 = ctx.comm_slab()
    for k, (pos, vp) in enumerate(cams):
        ctx.select_frame_slot(k & 1)
        ctx.set_camera_position(pos)
        ctx.render_gbuffer_rows(vp, r0, r1)
        ctx.frame_step()
        if k >= 1 and k % 2 == 1:                    # read frame k back while nothing newer is in flight behind it
            ctx.comm_sync()
            assert np.array_equal(ctx.comm_download_frame(), want[k]), f"frame {k}"
    for rep in range(30):                            # no read-back in between
        k = rep % n
        ctx.select_frame_slot(rep & 1)
        ctx.set_camera_position(cams[k][0]); ctx.render_gbuffer_rows(cams[k][1], r0, r1)
        ctx.frame_step()
    ctx.comm_sync()
    assert np.array_equal(ctx.comm_download_frame(), want[29 % n])
    ctx.comm_destroy()
    ctx.select_frame_slot(0)
    ctx.set_camera_position(cams[1][0]); ctx.render_gbuffer(cams[1][1])
    assert np.array_equal(ctx.trace_current(), want[1])
    ctx.close()


def test_second_slot_is_released(vct):
    """Enabling and disabling the second slot leaves no memory behind (190 MB per 1080p slot would add up), its raster
    scratch included: every second slot rasterises a G-buffer before it goes."""
    import torch
    ctx, sc = make(vct, 1920, 1080, 32)
    vp = cameras(sc, 1920, 1080, 1)[0][1]
    ctx.render_shadow_map(sc.light_view_proj((0.0, 1.0, 0.25)))
    ctx.render_gbuffer(vp)                           # shared state (shadow map, alpha classes) exists before the baseline
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        ctx.set_frames_in_flight(2)
        assert free0 - torch.cuda.mem_get_info()[0] > 150 << 20
        ctx.select_frame_slot(1)
        ctx.render_gbuffer(vp)                       # allocates slot 1's raster scratch
        ctx.set_frames_in_flight(1)
    assert abs(free0 - torch.cuda.mem_get_info()[0]) < 8 << 20
    ctx.set_frames_in_flight(2)
    ctx.select_frame_slot(1)
    ctx.render_gbuffer(vp)
    ctx.close()                                      # destroy with the second slot alive
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)


def test_facade_demo_with_two_frames_in_flight_prints_the_same_checksum():
    """vct_demo (the reference application's call sequence through host/Voxel_Cone_Tracing.h) with FramesInFlight = 2: a moving
    camera, frames never read back in the loop -- the last frame's checksum and step count equal the one-slot run's."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "voxel-cone-tracing_amd", "vct_demo")
    args = ["--scene", "procedural:atrium", "--voxels", "64", "--size", "640x360", "--shadow", "1024", "--frames", "14"]
    one = subprocess.run([demo] + args, capture_output=True, text=True, timeout=600)
    two = subprocess.run([demo] + args + ["--frames-in-flight", "2"], capture_output=True, text=True, timeout=600)
    assert one.returncode == 0 and two.returncode == 0, one.stdout + one.stderr + two.stdout + two.stderr

    def last(txt):
        ln = [l for l in txt.splitlines() if l.startswith("frames=")][-1]
        return [t for t in ln.split() if t.startswith(("fnv1a=", "cone_steps="))]
    assert "2 frames in flight" in two.stdout and last(one.stdout) == last(two.stdout)
    # ... and with the whole GI pass per frame (moving light path of the facade)
    dl1 = subprocess.run([demo] + args + ["--dynamic-light"], capture_output=True, text=True, timeout=600)
    dl2 = subprocess.run([demo] + args + ["--dynamic-light", "--frames-in-flight", "2"], capture_output=True, text=True, timeout=600)
    assert dl1.returncode == 0 and dl2.returncode == 0, dl1.stdout + dl2.stdout + dl2.stderr
    # (the option really was taken -- vct_demo once paired its arguments two by two and lost it behind --dynamic-light)
    assert "2 frames in flight" in dl2.stdout and last(dl1.stdout) == last(dl2.stdout)


def test_bench_plain_run_dumps_the_frame_of_its_last_step(tmp_path):
    """bench.py without --full: the headline line only, and --dump-outputs writes the frame of the last timed step --
    the same frame the --full run of the same arguments computes (its extra measurements run after the dump)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--width", "320",
            "--height", "180", "--voxel-dim", "64", "--scene-detail", "0.15", "--shadow-size", "512"]
    lines = {}
    for form in ("plain", "full"):
        extra = ["--full", "--cpu-seconds", "0", "--no-sweep"] if form == "full" else []
        out = subprocess.run(base + extra + ["--dump-outputs", str(tmp_path / form)], capture_output=True, text=True,
                             timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        got = [ln for ln in out.stdout.split("\n") if ln.strip()]
        assert len(got) == 1, got
        lines[form] = json.loads(got[0])
    plain, full = lines["plain"], lines["full"]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain and key in full, key
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["metric"] == full["metric"] and plain["unit"] == full["unit"] == "Mcones/s"
    assert "roofline" not in plain and "gi_pass_ms" not in plain and "roofline" in full and "gi_pass_ms" in full
    a, b = np.load(tmp_path / "plain" / "frame.npy"), np.load(tmp_path / "full" / "frame.npy")
    assert a.dtype == np.float32 and a.shape == (180, 320, 4) and np.isfinite(a).all() and (a != 0).any()
    assert np.array_equal(a, b)
