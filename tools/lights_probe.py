"""ON THE GPU BOX: what local lights cost (include/vct.h "local lights"), HIP events on the context's stream.

configs[1] (procedural atrium, 256^3, 1920x1080) with 1, 8 and 64 lights placed inside the atrium (seeded; every other one
a spot).  Per light count, medians over ROUNDS rounds that alternate detached / attached on ONE context:
  * the two kernels' own times (vct_last_lights_ms: k_light_voxels behind the resolve, k_light_pixels in front of the trace);
  * vct_inject_light without and with lights (events around the call: resolve, + k_light_voxels);
  * one resident step (vct_trace_resident, trace timing off as in a frame loop; STEPS steps between two events)
    without and with lights: with them the step is k_light_pixels + the COMP trace kernel with planes.
The frame and the chain with lights differ from those without (asserted), and the detached ones are bit for bit those
of the first detached round (asserted).
STEP_ONLY=1: only the detached resident step, through entry points every earlier version of the library has -- run it from
a checkout of the parent commit and from this tree alternately to compare the two (tools/lights_probe.sh does).
Writes lights_probe.txt (or lights_probe_step.txt) to $OUT (default: tool_out/)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vctpkg  # noqa: E402

vct = vctpkg.load()
from voxel_cone_tracing_amd import scene as sc  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "9"))
STEPS = int(os.environ.get("STEPS", "40"))
STEP_ONLY = os.environ.get("STEP_ONLY", "0") == "1"
COUNTS = [int(x) for x in os.environ.get("COUNTS", "1,8,64").split(",")]
light = (0.0, 1.0, 0.25)
w, h, S, V = 1920, 1080, 4096, 256


def ev():
    return torch.cuda.Event(enable_timing=True)


def stats(v):
    v = np.array(v)
    return f"{np.median(v):.4f} ms (min {v.min():.4f} max {v.max():.4f})"


def atrium_lights(n, seed=7):
    """n lights inside the atrium's hall (world units; the camera of configs[1] stands at (-56, -9, 2))."""
    r = np.random.default_rng(seed)
    out = []
    for i in range(n):
        pos = (float(r.uniform(-55.0, 55.0)), float(r.uniform(-15.0, 15.0)), float(r.uniform(-20.0, 20.0)))
        col = tuple(float(c) for c in r.uniform(20.0, 80.0, 3))
        d = dict(position=pos, color=col, radius=25.0, source_radius=0.5)
        if i % 2:
            axis = r.normal(size=3)
            d.update(direction=tuple(float(c) for c in axis), cos_inner=0.9, cos_outer=0.5, flags=1)
        out.append(d)
    return out


scene = sc.Scene(sc.ATRIUM, 1.0, 1234)
cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(light)
cfg = dict(voxel_dim=V, width=w, height=h, shadow_map_size=S)
if not STEP_ONLY:
    cfg["voxel_attributes"] = 1
ctx = vct.Context(vct.default_config(**cfg))
ctx.upload_scene(scene)
ctx.set_camera_position(tuple(cam.position))
ctx.set_light_direction(light)
ctx.render_shadow_map(lvp)
st = torch.cuda.ExternalStream(ctx.stream())


def voxel_pass():
    """ms of vct_inject_light (events around it), between a voxelize and a mip build"""
    e = [ev(), ev()]
    ctx.voxelize()
    with torch.cuda.stream(st):
        e[0].record(); ctx.inject_light(); e[1].record()
    ctx.build_mips()
    ctx.synchronize()
    return e[0].elapsed_time(e[1])


def step_ms():
    """ms per resident step: STEPS steps between two events, trace timing off"""
    ctx.set_trace_timing(False)
    e = [ev(), ev()]
    for _ in range(5):
        ctx.trace_resident()
    with torch.cuda.stream(st):
        e[0].record()
        for _ in range(STEPS):
            ctx.trace_resident()
        e[1].record()
    ctx.synchronize()
    ctx.set_trace_timing(True)
    return e[0].elapsed_time(e[1]) / STEPS


for _ in range(3):
    voxel_pass()
ctx.render_gbuffer(vp)
ctx.trace_resident()
ctx.synchronize()

out_dir = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out_dir, exist_ok=True)
if STEP_ONLY:
    v = [step_ms() for _ in range(ROUNDS)]
    txt = f"lights_probe step only ({os.environ.get('LABEL', 'this tree')}): {w}x{h}, atrium {V}^3, resident step {stats(v)}"
    print(txt)
    with open(os.path.join(out_dir, "lights_probe_step.txt"), "a") as f:
        f.write(txt + "\n")
    sys.exit(0)

lines = [f"lights_probe: atrium {V}^3, {w}x{h}, shadow map {S}^2, {ROUNDS} alternating rounds, {STEPS} steps per step sample"]
chain0 = frame0 = None
for n in COUNTS:
    lights = atrium_lights(n)
    t = {k: [] for k in ("inj0", "inj1", "step0", "step1", "kvox", "kpix", "trace0", "trace1")}
    for r in range(ROUNDS):
        ctx.set_lights(None)
        voxel_pass()
        t["inj0"].append(voxel_pass())
        t["step0"].append(step_ms())
        ctx.trace_resident(); ctx.synchronize()
        t["trace0"].append(ctx.last_trace_ms())
        if r == 0:
            c, f = ctx.download_chain(), ctx.download_frame()
            if chain0 is None:
                chain0, frame0 = c, f
            assert np.array_equal(c, chain0) and np.array_equal(f, frame0), "detached is not what it was"
        ctx.set_lights(lights)
        voxel_pass()
        t["inj1"].append(voxel_pass())
        t["step1"].append(step_ms())
        ctx.trace_resident(); ctx.synchronize()
        t["trace1"].append(ctx.last_trace_ms())
        ms = ctx.last_lights_ms()
        t["kvox"].append(ms[0]); t["kpix"].append(ms[1])
        if r == 0:
            assert not np.array_equal(ctx.download_chain(), chain0), "the lights changed nothing in the chain"
            assert not np.array_equal(ctx.download_frame(), frame0), "the lights changed nothing in the frame"
    c = ctx.stage_counts()
    lines += [f"{n} light(s): brick slots {c['accumulator_bricks']}",
              f"  k_light_voxels {stats(t['kvox'])}   k_light_pixels {stats(t['kpix'])}",
              f"  inject        detached {stats(t['inj0'])}   attached {stats(t['inj1'])}   "
              f"difference {(np.median(t['inj1']) - np.median(t['inj0'])) * 1e3:+.1f} us",
              f"  resident step detached {stats(t['step0'])}   attached {stats(t['step1'])}   "
              f"difference {(np.median(t['step1']) - np.median(t['step0'])) * 1e3:+.1f} us",
              f"  trace kernel  detached (plain) {stats(t['trace0'])}   attached (COMP, planes) {stats(t['trace1'])}"]
ctx.set_lights(None)
ctx.close()
txt = "\n".join(lines)
print(txt)
with open(os.path.join(out_dir, "lights_probe.txt"), "w") as f:
    f.write(txt + "\n")
