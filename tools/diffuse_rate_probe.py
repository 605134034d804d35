"""ON THE GPU BOX: the half-rate diffuse gather (vct_set_diffuse_rate) against rate 1, whole passes.

Cases: configs[1] (procedural atrium, 256^3, 1920x1080) and the Bistro-class street at 1920x1080 (256^3).  Per case,
rounds that alternate rate 1 and rate 2; a pass is timed by torch events around PER_ROUND vct_trace_resident calls
with the library's own timing events OFF (they cost a launch ~7 us each), so the figure holds every launch of the pass
and the gaps between them.  The four launches of a rate-2 pass are then timed apart with the timing events on
(vct_last_diffuse_rate_ms).  Also: executed steps, the share of fill pixels, and the rate-2 frame against the rate-1
frame of the same run (relative L2, largest difference of 16x16-block means, of the RGB channels).
VCT_DIFFUSE_RATE_WAVES=2 in the environment selects the two-wave march.  Writes diffuse_rate_probe.txt to $OUT
(default: tool_out/)."""
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

w, h, S = 1920, 1080, 4096
ROUNDS, PER_ROUND = 8, 10
light = (0.0, 1.0, 0.25)
CASES = [
    ("atrium 256^3 1080p (configs[1])", sc.ATRIUM, 256, sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)),
    ("street 256^3 1080p", sc.BISTRO, 256, sc.default_camera(position=(-58.0, -19.0, 1.5), yaw=0.0, pitch=12.0)),
]


def block_means(frame):
    f = vct.half_to_float(frame).reshape(h, w, 4)[: h // 16 * 16, : w // 16 * 16, :3]
    return f.reshape(h // 16, 16, w // 16, 16, 3).mean(axis=(1, 3))


lines = [f"diffuse_rate_probe: {w}x{h}, {ROUNDS} alternating rounds x {PER_ROUND} passes, march waves "
         f"{os.environ.get('VCT_DIFFUSE_RATE_WAVES', '1')}"]
for label, kind, V, cam in CASES:
    ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
    ctx.upload_scene(sc.Scene(kind, 1.0, 1234))
    ctx.set_camera_position(tuple(cam.position))
    ctx.set_light_direction(light)
    ctx.render_shadow_map(sc.light_view_proj(light))
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
    ctx.render_gbuffer(sc.camera_view_proj(cam, w, h))
    live = np.zeros(((h + 1) // 2 * 2, (w + 1) // 2 * 2), bool)
    live[:h, :w] = (ctx.download_gbuffer()[18] >= 0.5).reshape(h, w)
    alive = int(live.sum())
    anchors = int(live.reshape(live.shape[0] // 2, 2, live.shape[1] // 2, 2).any(axis=(1, 3)).sum())
    stream = torch.cuda.ExternalStream(ctx.stream())
    frames, steps, marched, times = {}, {}, {}, {1: [], 2: []}
    for rate in (1, 2):                                   # warm-up and the figures that do not vary
        ctx.set_diffuse_rate(rate)
        frames[rate] = ctx.trace_current()
        steps[rate] = ctx.last_step_count()
        marched[rate] = ctx.diffuse_rate()[1]
        for _ in range(10):
            ctx.trace_resident()
        ctx.synchronize()
    ctx.set_trace_timing(False)
    for r in range(ROUNDS):
        for rate in ((1, 2) if r % 2 == 0 else (2, 1)):
            ctx.set_diffuse_rate(rate)                    # (allocates / frees: outside the timed region)
            ctx.trace_resident()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(PER_ROUND):
                ctx.trace_resident()
            e1.record(stream)
            e1.synchronize()
            times[rate].append(e0.elapsed_time(e1) / PER_ROUND)
    ctx.set_trace_timing(True)
    ctx.set_diffuse_rate(2)
    parts = []
    for _ in range(30):
        ctx.trace_resident()
        parts.append(ctx.last_diffuse_rate_ms())
    parts = np.median(np.array(parts), axis=0)
    ctx.set_diffuse_rate(1)
    k1 = []
    for _ in range(30):
        ctx.trace_resident()
        k1.append(ctx.last_trace_ms())
    a, b = vct.half_to_float(frames[2]).reshape(-1, 4)[:, :3], vct.half_to_float(frames[1]).reshape(-1, 4)[:, :3]
    rel = float(np.linalg.norm((a - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))
    blk = float(np.abs(block_means(frames[2]) - block_means(frames[1])).max())
    t1, t2 = np.array(times[1]), np.array(times[2])
    lines += [
        f"{label}: live pixels {alive}",
        f"  rate 1  {np.median(t1):.4f} ms per pass (min {t1.min():.4f} max {t1.max():.4f})  steps {steps[1]}  "
        f"kernel {np.median(k1):.4f} ms",
        f"  rate 2  {np.median(t2):.4f} ms per pass (min {t2.min():.4f} max {t2.max():.4f})  steps {steps[2]}  "
        f"marched pixels {marched[2]} = {anchors} anchors + {marched[2] - anchors} fill "
        f"({100.0 * (marched[2] - anchors) / max(alive, 1):.2f} % of the live pixels)  "
        f"vs rate 1 {100.0 * (np.median(t2) / np.median(t1) - 1.0):+.1f} %",
        f"  rate 2 launches (ms, timing events on): coarse march {parts[0]:.4f}  resolve {parts[1]:.4f}  "
        f"fill march {parts[2]:.4f}  specular trace + composite {parts[3]:.4f}  sum {parts.sum():.4f}",
        f"  rate-2 frame vs rate-1 frame (RGB): rel-L2 {rel:.3e}  largest 16x16 block-mean difference {blk:.3e}",
    ]
    ctx.close()
txt = "\n".join(lines)
print(txt)
out = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "diffuse_rate_probe.txt"), "w") as f:
    f.write(txt + "\n")
