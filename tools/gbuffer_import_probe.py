"""ON THE GPU BOX: what the G-buffer import costs (include/vct.h "G-buffer import").

The procedural atrium at 256^3, 1920x1080, one context.  The G-buffer the library rasterised is read back once and
packed into two sets of renderer buffers in device memory:
  (a) DEPTH_F32 + octahedral SNORM16x2 normal + UNORM8x4 albedo + UNORM8x4 specular       16 B per pixel
  (b) POSITION_F32X3 + F16X4 geometric and shading normals + UNORM8x4 albedo and specular   36 B per pixel
each imported with a given fp32 shadow plane (+ 4 B) and with the library's PCF against the context's shadow map.
Beside them, on the same frame:
  the whole G-buffer pass of vct_render_gbuffer (visibility + k_gbuffer_shade; the shade kernel has no timer of its own),
  k_tile_gbuffer: vct_trace_slab over NO tile rows of the frame as 23 LINEAR device planes -- the tiling kernel and no
  march -- which moves 92 B in and 92 B out per pixel: the route a caller with its own G-buffer had before the import.
The arms alternate in one run after each was warmed.  Two clocks: torch events on the slot's stream around the call
(every arm: the same method, it includes the launch gap) and, for the imports, vct_last_gbuffer_import_ms (the kernel
alone).  Bytes over time are the algorithmic bytes of the import (inputs read once + 92 B written; the PCF's fetches
are not counted), as a share of the 8 TB/s HBM peak.
Also printed: the relative L2 between the frame traced from the rasterised G-buffer and from its re-import through (b)
with the given shadow plane -- the cost of fp16 normals, 8-bit colours and a synthesised tangent frame.
Writes gbuffer_import_probe.txt to $OUT (default: tool_out/)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gbuffer_import_ref as ir  # noqa: E402
import synth  # noqa: E402
import vctpkg  # noqa: E402

vct = vctpkg.load()
from voxel_cone_tracing_amd import scene as sc  # noqa: E402

w, h, S, V = 1920, 1080, 4096, 256
ROUNDS = int(os.environ.get("ROUNDS", "9"))
REPS = int(os.environ.get("REPS", "10"))
HBM_PEAK = 8.0e12
light = (0.0, 1.0, 0.25)
npix = w * h


def stats(v):
    v = np.array(v)
    return f"{np.median(v):.4f} ms (min {v.min():.4f} max {v.max():.4f})"


ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
scene = sc.Scene(sc.ATRIUM, 1.0, 1234)
cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
view_proj = sc.camera_view_proj(cam, w, h)
ctx.upload_scene(scene)
ctx.set_camera_position(tuple(cam.position))
ctx.set_light_direction(light)
ctx.render_shadow_map(sc.light_view_proj(light))
ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
ctx.render_gbuffer(view_proj)
planes = ctx.download_gbuffer()
native = ctx.trace_current()
covered = planes[18] >= np.float32(0.5)
scale = float(ctx.cfg.model_scale)

# the renderer's buffers
P = np.ascontiguousarray(planes[0:3].T)
_, _, depth = ir.project_depth(P, view_proj)
depth = np.where(covered, depth, 1.0).astype(np.float32)
geo, shd = planes[3:6].T / np.float32(scale), planes[12:15].T
albedo = ir.pack_color(planes[15:19].T, ir.COLOR_UNORM8X4, w, h)
specular = ir.pack_color(np.concatenate([planes[19:22].T, np.ones((npix, 1), np.float32)], 1), ir.COLOR_UNORM8X4, w, h)
host = dict(depth=depth, oct=ir.oct_encode(geo), position=P, geo16=ir.pack_vectors(planes[3:6].T, ir.NORMAL_F16X4, w, h),
            shd16=ir.pack_vectors(shd, ir.NORMAL_F16X4, w, h), albedo=albedo, specular=specular, shadow=np.ascontiguousarray(planes[22]),
            linear=planes)
dev = {k: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda() for k, v in host.items()}
ptr = {k: t.data_ptr() for k, t in dev.items()}
torch.cuda.synchronize()
colours = dict(albedo=ptr["albedo"], albedo_format=ir.COLOR_UNORM8X4, specular=ptr["specular"], specular_format=ir.COLOR_UNORM8X4)
set_a = dict(position=ptr["depth"], position_format=ir.DEPTH_F32, normal=ptr["oct"], normal_format=ir.NORMAL_OCT,
             inv_view_proj=sc.invert_matrix(view_proj), depth_clear=1.0, normal_scale=scale, **colours)
set_b = dict(position=ptr["position"], position_format=ir.POSITION_F32X3, normal=ptr["geo16"], shading_normal=ptr["shd16"],
             normal_format=ir.NORMAL_F16X4, normal_scale=scale, **colours)
stream = torch.cuda.ExternalStream(ctx.stream())
frame_ptr, _ = ctx.frame_device()


class Arm:
    def __init__(self, label, call, bytes_per_pixel=None, own_timer=False):
        self.label, self.call, self.bytes, self.own_timer = label, call, bytes_per_pixel, own_timer
        self.bracket, self.kernel = [], []


arms = [
    Arm("(a) depth + oct + unorm8 x2, given shadow", lambda: ctx.import_gbuffer(shadow=ptr["shadow"], **set_a), 16 + 4 + 92, True),
    Arm("(a) depth + oct + unorm8 x2, library PCF", lambda: ctx.import_gbuffer(**set_a), 16 + 92, True),
    Arm("(b) f32x3 + f16x4 x2 + unorm8 x2, given shadow", lambda: ctx.import_gbuffer(shadow=ptr["shadow"], **set_b), 36 + 4 + 92, True),
    Arm("(b) f32x3 + f16x4 x2 + unorm8 x2, library PCF", lambda: ctx.import_gbuffer(**set_b), 36 + 92, True),
    Arm("vct_render_gbuffer (visibility + shade)", lambda: ctx.render_gbuffer(view_proj)),
    Arm("k_tile_gbuffer (23 LINEAR device planes)", lambda: ctx.trace(ptr["linear"], rows=(0, 0), out_device_ptr=frame_ptr), 92 + 92),
]


def run(a, record):
    for _ in range(REPS if record else 2):
        ctx.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        a.call()
        e1.record(stream)
        e1.synchronize()
        if record:
            a.bracket.append(e0.elapsed_time(e1))
            if a.own_timer:
                a.kernel.append(ctx.last_gbuffer_import_ms())


for a in arms:
    run(a, False)
for r in range(ROUNDS):
    for a in (arms if r % 2 == 0 else arms[::-1]):
        run(a, True)

lines = [f"gbuffer_import_probe: atrium {V}^3 {w}x{h}, {scene.ntri} triangles, covered pixels {int(covered.sum())} of {npix}; "
         f"{ROUNDS} alternating rounds of {REPS} calls"]
for a in arms:
    t = np.median(a.kernel) if a.kernel else np.median(a.bracket)
    line = f"  {a.label:52s} bracketed {stats(a.bracket)}"
    if a.kernel:
        line += f"   kernel {stats(a.kernel)}"
    if a.bytes:
        line += f"   {a.bytes} B/pixel = {a.bytes * npix / (t * 1e-3) / 1e12:.2f} TB/s = {100.0 * a.bytes * npix / (t * 1e-3) / HBM_PEAK:.0f} % of HBM peak"
    lines.append(line)
tile = np.median(arms[5].bracket)
for a in arms[:4]:
    lines.append(f"  {a.label:52s} bracketed / k_tile_gbuffer bracketed = {np.median(a.bracket) / tile:.2f}")

# what the compact formats cost the frame: (b) with the given shadow plane against the rasterised G-buffer
ctx.import_gbuffer(shadow=ptr["shadow"], **set_b)
again = ctx.trace_current()
a32, n32 = vct.half_to_float(again.reshape(-1, 4)), vct.half_to_float(native.reshape(-1, 4))
ok = np.isfinite(a32).all(1) & np.isfinite(n32).all(1)
lines.append(f"  frame of the re-import through (b) against the frame of the rasterised G-buffer: relative L2 {synth.rel_l2(a32[ok], n32[ok]):.3e} "
             f"({int(ok.sum())} of {npix} pixels finite in both)")
ctx.import_gbuffer(shadow=ptr["shadow"], **set_a)
again = ctx.trace_current()
a32 = vct.half_to_float(again.reshape(-1, 4))
ok = np.isfinite(a32).all(1) & np.isfinite(n32).all(1)
lines.append(f"  ... through (a) (depth reconstruction, octahedral normal, no shading normal): relative L2 {synth.rel_l2(a32[ok], n32[ok]):.3e}")
ctx.close()
txt = "\n".join(lines)
print(txt)
out = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "gbuffer_import_probe.txt"), "w") as f:
    f.write(txt + "\n")
