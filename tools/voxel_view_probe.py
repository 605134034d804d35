"""ON THE GPU BOX: the voxel view (vct_render_voxels) with and without its empty-space skip.

Cases: configs[1] (procedural atrium, 256^3, 1920x1080), levels 0 and 3, and the Bistro-class street at 1024^3 /
3840x2160, level 0 (CASES=atrium or CASES=street in the environment runs one of them).  Per case and level: the view
from the bench camera, warmed up (the first view also builds the occupancy words), then ROUNDS rounds that alternate
the two instantiations of the walk kernel on the same context (VCT_VOXVIEW_SKIP is read per call); a round is PER_ROUND
views, each timed by the library's own events around the walk kernel (vct_last_voxel_view_ms); the figure is the median
over all views of an arm, with the smallest and largest.  The two arms' frames are compared bit for bit, and the occupancy
rebuild is timed apart by torch events around the first view after the chain's generation changed.
Writes voxel_view_probe.txt to $OUT (default: tool_out/)."""
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

ROUNDS, PER_ROUND = 6, 5
light = (0.0, 1.0, 0.25)
CASES = {
    "atrium": ("atrium 256^3 1920x1080 (configs[1])", sc.ATRIUM, 256, 1920, 1080, (0, 3),
               sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)),
    "street": ("street 1024^3 3840x2160 (configs[4])", sc.BISTRO, 1024, 3840, 2160, (0,),
               sc.default_camera(position=(-58.0, -19.0, 1.5), yaw=0.0, pitch=12.0)),
}


def arm(ctx, m, level, skip, n):
    os.environ["VCT_VOXVIEW_SKIP"] = "1" if skip else "0"
    out = []
    for _ in range(n):
        ctx.render_voxels(m, vct.VOXVIEW_CURRENT, level)
        out.append(ctx.last_voxel_view_ms())
    return out


lines = [f"voxel_view_probe: {ROUNDS} alternating rounds x {PER_ROUND} views per arm, device ms of the walk kernel"]
for key in os.environ.get("CASES", "atrium,street").split(","):
    label, kind, V, w, h, levels, cam = CASES[key]
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=4096))
    ctx.upload_scene(sc.Scene(kind, 1.0, 1234))
    ctx.set_light_direction(light)
    ctx.render_shadow_map(sc.light_view_proj(light))
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    ctx.synchronize()
    m = sc.invert_matrix(sc.camera_view_proj(cam, w, h))
    stream = torch.cuda.ExternalStream(ctx.stream())
    lines.append(f"{label}: {ctx.stage_counts()['touched_bricks']} of {(V // 8) ** 3} bricks of level 0 occupied")
    for level in levels:
        os.environ["VCT_VOXVIEW_SKIP"] = "1"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx.render_voxels(m, vct.VOXVIEW_CURRENT, level)          # occupancy build + walk
        e1.record(stream)
        e1.synchronize()
        first = e0.elapsed_time(e1)
        frames = {}
        for skip in (True, False):
            arm(ctx, m, level, skip, 3)                             # warm-up of both instantiations
            frames[skip] = ctx.download_frame()
        same = bool(np.array_equal(frames[True], frames[False]))
        shown = float((frames[True][..., 3] != 0).mean())
        t = {True: [], False: []}
        for r in range(ROUNDS):
            for skip in ((True, False) if r % 2 == 0 else (False, True)):
                t[skip] += arm(ctx, m, level, skip, PER_ROUND)
        a, b = np.array(t[True]), np.array(t[False])
        lines += [
            f"  level {level} (N = {V >> level}): pixels with alpha != 0: {100.0 * shown:.1f} %; frames of the two arms equal: {same}",
            f"    first view (occupancy build + walk, torch events): {first:.3f} ms",
            f"    skip     {np.median(a):.4f} ms (min {a.min():.4f} max {a.max():.4f})",
            f"    no skip  {np.median(b):.4f} ms (min {b.min():.4f} max {b.max():.4f})   skip / no skip = {np.median(a) / np.median(b):.3f}",
        ]
        print("\n".join(lines[-4:]), flush=True)
    ctx.close()
os.environ.pop("VCT_VOXVIEW_SKIP", None)
txt = "\n".join(lines)
print(txt)
out = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "voxel_view_probe.txt"), "w") as f:
    f.write(txt + "\n")
