"""ON THE GPU BOX: what gloss classes cost the screen trace (include/vct.h "per-material gloss").

configs[1] (procedural atrium, 256^3, 1920x1080), whole-frame resident traces of one G-buffer on one context:
  (a) nothing attached                                        the kernels of every build before gloss classes
  (b) one class equal to config.tan_specular / shininess      prices the GLOSS instantiation itself (same marches)
  (c) the scene's materials dealt over 0.07 / 0.105 / 0.2     the realistic case: classes meet only where materials meet
  (d) a per-pixel checkerboard of those three classes         the worst case: every tile marches three times
and, to read march length apart from the cost of an extra class-march, one class alone at 0.105 and at 0.2.
The arms alternate on the one context (switching is vct_set_gloss_classes + vct_set_pixel_gloss, outside the timed
region).  Step times: timing events off, torch events around STEPS back-to-back traces.  Kernel times: a separate loop
with the timing events on (vct_last_trace_ms).  Executed steps per arm from vct_last_step_count.
Writes gloss_probe.txt to $OUT (default: tool_out/)."""
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
cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
THREE = [(0.07, 20.0), (0.105, 8.0), (0.2, 4.0)]


def stats(v):
    v = np.array(v)
    return f"{np.median(v):.4f} ms (min {v.min():.4f} max {v.max():.4f})"


ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
scene = sc.Scene(sc.ATRIUM, 1.0, 1234)
ctx.upload_scene(scene)
ctx.set_camera_position(tuple(cam.position))
ctx.set_light_direction(light)
ctx.render_shadow_map(sc.light_view_proj(light))
ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
vp = sc.camera_view_proj(cam, w, h)
# the plane of case (c) from the G-buffer pass itself: material m is class m % 3
ctx.set_gloss_classes(THREE)
ctx.upload_material_gloss((np.arange(scene.nmat) % 3).astype(np.uint8))
ctx.render_gbuffer(vp)
by_material = ctx.download_pixel_gloss()
ctx.upload_material_gloss(None)
ctx.set_gloss_classes(None)
live = ~(ctx.download_gbuffer()[18] < np.float32(0.5))
y, x = np.divmod(np.arange(w * h), w)
checker = ((x + y) % 3).astype(np.uint8)
tiles = (by_material.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64), live.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64))
per_tile = np.array([len(set(c[m].tolist())) for c, m in zip(*tiles)])
cfg_class = (ctx.cfg.tan_specular, ctx.cfg.shininess)


class Arm:
    def __init__(self, label, classes, plane):
        self.label, self.classes, self.plane = label, classes, plane
        self.step, self.kernel, self.steps, self.division = [], [], None, None

    def select(self):
        ctx.set_gloss_classes(self.classes)
        if self.classes:
            ctx.set_pixel_gloss(self.plane)
        ctx.synchronize()


arms = [Arm("(a) nothing attached", None, None),
        Arm("(b) one class = config", [cfg_class], None),
        Arm("(c) materials over 3 classes", THREE, by_material),
        Arm("(d) per-pixel checkerboard", THREE, checker),
        Arm("    one class 0.105 / 8", [THREE[1]], None),
        Arm("    one class 0.2 / 4", [THREE[2]], None)]
stream = torch.cuda.ExternalStream(ctx.stream())


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
    a.division = ctx.stage_counts()["march_division"]


def run_kernel(a, record):
    ctx.set_trace_timing(True)
    for _ in range(STEPS if record else 2):
        ctx.trace_resident()
        ms = ctx.last_trace_ms()
        if record:
            a.kernel.append(ms)


for a in arms:                                   # warm-up: every arm once, first-use divisor checks included
    a.select()
    run_steps(a, False)
    run_kernel(a, False)
for r in range(ROUNDS):
    for a in (arms if r % 2 == 0 else arms[::-1]):
        a.select()
        run_steps(a, True)
for r in range(2):
    for a in (arms if r % 2 == 0 else arms[::-1]):
        a.select()
        run_kernel(a, True)

lines = [f"gloss_probe: atrium {V}^3 {w}x{h}, {ROUNDS} alternating rounds of {STEPS} steps; kernel times over {2 * STEPS} launches",
         f"live pixels {int(live.sum())} of {w * h}; case (c): {scene.nmat} materials, class m % 3; tiles with live pixels "
         f"{int((per_tile > 0).sum())}, of them with 1 / 2 / 3 classes: {int((per_tile == 1).sum())} / {int((per_tile == 2).sum())} / {int((per_tile == 3).sum())}"]
ctx.set_gloss_classes(THREE)
lines.append(f"gloss classes {[list(map(float, c)) for c in THREE]}, march steps of their tables {ctx.get_gloss_classes()[1].tolist()}")
base_step, base_kernel, base_steps = np.median(arms[0].step), np.median(arms[0].kernel), arms[0].steps
for a in arms:
    lines.append(f"  {a.label:32s} step {stats(a.step)} {100.0 * (np.median(a.step) / base_step - 1.0):+6.1f} %   "
                 f"kernel {stats(a.kernel)} {100.0 * (np.median(a.kernel) / base_kernel - 1.0):+6.1f} %   "
                 f"steps {a.steps} ({100.0 * (a.steps / base_steps - 1.0):+.1f} %)  division form {a.division}")
assert arms[1].steps == arms[0].steps, "one class equal to the config marches what the plain trace marches"
ctx.close()
txt = "\n".join(lines)
print(txt)
out = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "gloss_probe.txt"), "w") as f:
    f.write(txt + "\n")
