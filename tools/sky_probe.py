"""ON THE GPU BOX: what an attached sky costs the screen trace (include/vct.h "sky light").

Two scenes at 1920x1080, whole-frame resident traces of one G-buffer on one context each:
  configs[1]: the procedural atrium at 256^3
  the procedural Bistro-class street (configs[4]'s scene) at 256^3
with two arms that alternate on the one context (switching is vct_set_sky, outside the timed region):
  (a) nothing attached      the kernels of every build before sky light
  (b) a gradient sky        the SKY instantiation: the same march, one epilogue per cone
Step times: timing events off, torch events around STEPS back-to-back traces.  Kernel times: a separate loop with the
timing events on (vct_last_trace_ms).  Executed steps per arm from vct_last_step_count: they must be equal.
Writes sky_probe.txt to $OUT (default: tool_out/)."""
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

w, h, S, V = 1920, 1080, 4096, 256
ROUNDS = int(os.environ.get("ROUNDS", "7"))
STEPS = int(os.environ.get("STEPS", "20"))
light = (0.0, 1.0, 0.25)
SKY = sc.sky_gradient((0.3, 0.5, 1.0), (0.8, 0.8, 0.8), (0.1, 0.1, 0.1))
SCENES = [("atrium (configs[1])", sc.ATRIUM, sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)),
          ("street (configs[4]'s scene)", sc.BISTRO, sc.default_camera(position=(-58.0, -19.0, 1.5), yaw=0.0, pitch=12.0))]


def stats(v):
    v = np.array(v)
    return f"{np.median(v):.4f} ms (min {v.min():.4f} max {v.max():.4f})"


class Arm:
    def __init__(self, label, sky):
        self.label, self.sky = label, sky
        self.step, self.kernel, self.steps = [], [], None


def probe(label, kind, cam):
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
    scene = sc.Scene(kind, 1.0, 1234)
    ctx.upload_scene(scene)
    ctx.set_camera_position(tuple(cam.position))
    ctx.set_light_direction(light)
    ctx.render_shadow_map(sc.light_view_proj(light))
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    ctx.render_gbuffer(sc.camera_view_proj(cam, w, h))
    live = ~(ctx.download_gbuffer()[18] < np.float32(0.5))
    stream = torch.cuda.ExternalStream(ctx.stream())
    arms = [Arm("(a) nothing attached", None), Arm("(b) gradient sky", SKY)]

    def select(a):
        ctx.set_sky(a.sky)
        ctx.synchronize()

    def run_steps(a, record):
        ctx.set_trace_timing(False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.trace_resident()
        ctx.synchronize()
        e0.record(stream)
        for _ in range(STEPS):
            ctx.trace_resident()
        e1.record(stream)
        e1.synchronize()
        if record:
            a.step.append(e0.elapsed_time(e1) / STEPS)
        a.steps = ctx.last_step_count()

    def run_kernel(a, record):
        ctx.set_trace_timing(True)
        for _ in range(STEPS if record else 2):
            ctx.trace_resident()
            ms = ctx.last_trace_ms()
            if record:
                a.kernel.append(ms)

    for a in arms:                                   # warm-up: both arms once
        select(a)
        run_steps(a, False)
        run_kernel(a, False)
    for r in range(ROUNDS):
        for a in (arms if r % 2 == 0 else arms[::-1]):
            select(a)
            run_steps(a, True)
    for r in range(2):
        for a in (arms if r % 2 == 0 else arms[::-1]):
            select(a)
            run_kernel(a, True)
    lines = [f"{label}: {V}^3 {w}x{h}, {scene.ntri} triangles, live pixels {int(live.sum())} of {w * h}"]
    base_step, base_kernel = np.median(arms[0].step), np.median(arms[0].kernel)
    for a in arms:
        lines.append(f"  {a.label:24s} step {stats(a.step)} {100.0 * (np.median(a.step) / base_step - 1.0):+6.2f} %   "
                     f"kernel {stats(a.kernel)} {100.0 * (np.median(a.kernel) / base_kernel - 1.0):+6.2f} %   steps {a.steps}")
    assert arms[0].steps == arms[1].steps, "the sky marches nothing"
    ctx.close()
    return lines


lines = [f"sky_probe: {ROUNDS} alternating rounds of {STEPS} steps; kernel times over {2 * STEPS} launches"]
for label, kind, cam in SCENES:
    lines += probe(label, kind, cam)
txt = "\n".join(lines)
print(txt)
out = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "sky_probe.txt"), "w") as f:
    f.write(txt + "\n")
