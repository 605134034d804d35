"""ON THE GPU BOX: what emissive materials cost (include/vct.h "emissive materials"), HIP events on the context's stream.

Two scenes -- configs[1] (procedural atrium, 256^3, 1920x1080) and the street at 1024^3 (1920x1080) -- with one material
made emissive.  Per scene, medians over ROUNDS alternating rounds with the smallest and largest sample:
  * voxelize / inject / mips with and without the emission pool (the inject stage is where the pool is read), and the
    bytes the extra read explains: touched bricks x 2 KiB;
  * the one-off pool build: the first voxelize after vct_upload_emission against the ones after it;
  * the G-buffer pass with and without the pixel-emission planes;
  * a trace step with planes (and one output on) against the same step with VCT_SHOW_ALL, that output on and no planes
    -- the COMP kernel both times, so the difference is the composite's add and the 12 B per pixel; beside them the plain
    kernel and the COMP kernel with planes alone.
The frame with emission differs from the one without (asserted).
Writes emission_probe.txt to $OUT (default: tool_out/)."""
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
light = (0.0, 1.0, 0.25)
w, h, S = 1920, 1080, 4096
SCENES = [("configs[1]: atrium 256^3", sc.ATRIUM, 1.0, 256, dict(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0), 1),
          ("street 1024^3", sc.BISTRO, 1.0, 1024, dict(position=(-58.0, -19.0, 1.5), yaw=0.0, pitch=12.0), 10)]
if os.environ.get("SCENES"):
    SCENES = [s for i, s in enumerate(SCENES) if str(i) in os.environ["SCENES"].split(",")]


def ev():
    return torch.cuda.Event(enable_timing=True)


def stats(v):
    v = np.array(v)
    return f"{np.median(v):.4f} ms (min {v.min():.4f} max {v.max():.4f})"


lines = [f"emission_probe: {w}x{h}, shadow map {S}^2, {ROUNDS} alternating rounds"]
for label, kind, detail, V, camkw, emitter in SCENES:
    scene = sc.Scene(kind, detail, 1234)
    cam = sc.default_camera(**camkw)
    vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(light)
    table = np.zeros((scene.nmat, 3), np.float32)
    table[emitter] = (1.0, 0.9, 0.7)
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
    ctx.upload_scene(scene)
    ctx.set_camera_position(tuple(cam.position))
    ctx.set_light_direction(light)
    ctx.render_shadow_map(lvp)
    st = torch.cuda.ExternalStream(ctx.stream())
    t = {k: [] for k in ("vox0", "inj0", "mip0", "vox1", "inj1", "mip1", "gb0", "gb1", "tr_aov", "tr_planes", "tr_planes_aov", "tr_plain")}
    first = []

    def voxel_pass(tag):
        e = [ev() for _ in range(4)]
        with torch.cuda.stream(st):
            e[0].record(); ctx.voxelize(); e[1].record(); ctx.inject_light(); e[2].record(); ctx.build_mips(); e[3].record()
        ctx.synchronize()
        d = [e[i].elapsed_time(e[i + 1]) for i in range(3)]
        if tag is not None:
            for k, v in zip(("vox", "inj", "mip"), d):
                t[k + tag].append(v)
        return d

    def frame_pass(tag):
        e = [ev() for _ in range(2)]
        with torch.cuda.stream(st):
            e[0].record(); ctx.render_gbuffer(vp); e[1].record()
        ctx.trace_resident()
        ctx.synchronize()
        t["gb" + tag].append(e[0].elapsed_time(e[1]))
        return ctx.last_trace_ms()

    for _ in range(3):
        voxel_pass(None)
    for r in range(ROUNDS):
        # without emission: plain kernels; and the COMP kernel with one output on, no planes
        ctx.upload_emission(None)
        voxel_pass(None)
        voxel_pass("0")
        t["tr_plain"].append(frame_pass("0"))
        ctx.set_aov_outputs(vct.AOV_DIRECT)
        ctx.trace_resident(); ctx.synchronize()
        t["tr_aov"].append(ctx.last_trace_ms())
        ctx.set_aov_outputs(0)
        frame0 = ctx.download_frame() if r == 0 else None
        # with emission: the first pass builds the pool
        ctx.upload_emission(table)
        first.append(voxel_pass(None)[0])
        voxel_pass("1")
        t["tr_planes"].append(frame_pass("1"))
        ctx.set_aov_outputs(vct.AOV_DIRECT)
        ctx.trace_resident(); ctx.synchronize()
        t["tr_planes_aov"].append(ctx.last_trace_ms())
        ctx.set_aov_outputs(0)
        if r == 0:
            assert not np.array_equal(ctx.download_frame(), frame0), "the emission changed nothing in the frame"
    c = ctx.stage_counts()
    bricks = c["touched_bricks"]
    extra_us = (np.median(t["inj1"]) - np.median(t["inj0"])) * 1e3
    lines += [f"{label}: {scene.ntri} triangles, emitter = material {emitter}, touched bricks {bricks}, brick slots {c['accumulator_bricks']}",
              f"  voxelize  without {stats(t['vox0'])}   with the pool {stats(t['vox1'])}",
              f"  inject    without {stats(t['inj0'])}   with the pool {stats(t['inj1'])}   "
              f"difference {extra_us:+.1f} us for {bricks * 2048 / 1e6:.1f} MB more read"
              + (f" = {bricks * 2048 / extra_us / 1e6:.2f} TB/s" if extra_us > 0 else ""),
              f"  mips      without {stats(t['mip0'])}   with {stats(t['mip1'])}",
              f"  pool build (first voxelize after the upload, minus the median of the later ones): "
              f"{np.median(first) - np.median(t['vox1']):.4f} ms (first: {stats(first)})",
              f"  G-buffer  without planes {stats(t['gb0'])}   with planes {stats(t['gb1'])}",
              f"  trace     plain kernel {stats(t['tr_plain'])}   COMP kernel, one output, no planes {stats(t['tr_aov'])}   "
              f"COMP kernel with planes {stats(t['tr_planes'])}   with planes and the output {stats(t['tr_planes_aov'])}"]
    ctx.close()
    del ctx, scene
txt = "\n".join(lines)
print(txt)
out = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "emission_probe.txt"), "w") as f:
    f.write(txt + "\n")
