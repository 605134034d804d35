"""ON THE GPU BOX: point queries (vct_gather_points) against the screen trace's diffuse-only launch, and the sort flag.

configs[1] (procedural atrium, 256^3, 1920x1080): the frame's live pixels are sent as gather points in four orders --
tile order (the screen trace's own: 8x8 tiles, lane = pixel of the tile), linear row order, shuffled by a fixed
permutation, and shuffled with VCT_QUERY_SORT_CELLS -- next to the screen trace with the specular terms switched off
(vct_set_lighting_components: the six diffuse cones of every live pixel, the same march).  The executed steps of every
arm must equal that launch's: asserted.  Then a 64^3 ambient-cube grid over the scene's bounds (1.57 M gathers) with and
without the flag.

Per arm: device time of the march kernel alone (vct_last_point_query_ms) and of the whole call (torch events on the
context's stream around it: key kernel + sort + march), points and outputs resident in HBM.  All arms are warmed up,
then ROUNDS rounds alternate them on one context; medians with the smallest and largest sample.
Writes point_query_probe.txt to $OUT (default: tool_out/)."""
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
light = (0.0, 1.0, 0.25)
cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
DIFFUSE_ONLY = vct.SHOW_DIFFUSE | vct.SHOW_INDIRECT_DIFFUSE | vct.SHOW_AMBIENT_OCCLUSION


def stats(v):
    v = np.array(v)
    return f"{np.median(v):.4f} ms (min {v.min():.4f} max {v.max():.4f})"


class Arm:
    def __init__(self, label, pts, sort):
        self.label, self.sort, self.n = label, sort, pts.shape[0]
        self.pts = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
        self.out = torch.zeros((self.n, 4), dtype=torch.float32, device="cuda")
        self.march, self.call, self.steps = [], [], None

    def run(self, ctx, stream, record=True):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx.gather_points(self.pts.data_ptr(), n=self.n, out_device_ptr=self.out.data_ptr(), sort=self.sort)
        e1.record(stream)
        e1.synchronize()
        if record:
            self.march.append(ctx.last_point_query_ms())
            self.call.append(e0.elapsed_time(e1))
        self.steps = ctx.last_point_query()[1]


def alternate(ctx, stream, arms, extra=None):
    for a in arms:
        a.run(ctx, stream, record=False)
        a.run(ctx, stream, record=False)
    for r in range(ROUNDS):
        order = arms if r % 2 == 0 else arms[::-1]
        for a in order:
            a.run(ctx, stream)
        if extra:
            extra()


lines = [f"point_query_probe: atrium {V}^3 {w}x{h}, {ROUNDS} alternating rounds"]
ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
scene = sc.Scene(sc.ATRIUM, 1.0, 1234)
ctx.upload_scene(scene)
ctx.set_camera_position(tuple(cam.position))
ctx.set_light_direction(light)
ctx.render_shadow_map(sc.light_view_proj(light))
ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
ctx.render_gbuffer(sc.camera_view_proj(cam, w, h))
planes = ctx.download_gbuffer()
live = ~(planes[18] < np.float32(0.5))
pix = np.flatnonzero(live)
pts_linear = np.ascontiguousarray(planes[0:12].T[pix])
ys, xs = pix // w, pix % w
tile_key = ((ys >> 3) * ((w + 7) // 8) + (xs >> 3)) * 64 + ((ys & 7) << 3 | (xs & 7))
pts_tile = pts_linear[np.argsort(tile_key, kind="stable")]
pts_shuffled = pts_linear[np.random.default_rng(1).permutation(pts_linear.shape[0])]
del planes

ctx.set_lighting_components(DIFFUSE_ONLY)
trace_ms = []
for _ in range(5):
    ctx.trace_resident()
ctx.synchronize()
trace_steps = ctx.last_step_count()


def time_trace():
    ctx.trace_resident()
    trace_ms.append(ctx.last_trace_ms())


stream = torch.cuda.ExternalStream(ctx.stream())
arms = [Arm("tile order", pts_tile, False), Arm("linear row order", pts_linear, False), Arm("shuffled", pts_shuffled, False),
        Arm("shuffled + SORT_CELLS", pts_shuffled, True)]
alternate(ctx, stream, arms, time_trace)
lines.append(f"live pixels {pix.size}; screen trace, diffuse cones only: kernel {stats(trace_ms)}  steps {trace_steps}")
for a in arms:
    assert a.steps == trace_steps, (a.label, a.steps, trace_steps)
    m = np.median(a.march)
    lines.append(f"  {a.label:24s} march {stats(a.march)}  whole call {stats(a.call)}  steps {a.steps}  "
                 f"march vs trace {100.0 * (m / np.median(trace_ms) - 1.0):+.1f} %  {a.steps / m / 1e6:.1f} Gsteps/s")
ref = arms[0].out.cpu().numpy()
order_tile = np.argsort(tile_key, kind="stable")
lin = arms[1].out.cpu().numpy()
assert np.array_equal(ref.view(np.uint32), lin[order_tile].view(np.uint32)), "tile-order and linear-order results differ"
assert np.array_equal(arms[2].out.cpu().numpy().view(np.uint32), arms[3].out.cpu().numpy().view(np.uint32)), "the sort changed a result"

# 64^3 ambient cubes over the scene's bounds
P = np.asarray(scene.pos, np.float32).reshape(-1, 3) * np.float32(ctx.cfg.model_scale)
lo, hi = P.min(0), P.max(0)
N = 64
c = (np.arange(N, dtype=np.float32) + np.float32(0.5)) / np.float32(N)
zz, yy, xx = np.meshgrid(c, c, c, indexing="ij")
centres = np.stack([lo[0] + (hi[0] - lo[0]) * xx, lo[1] + (hi[1] - lo[1]) * yy, lo[2] + (hi[2] - lo[2]) * zz], axis=-1).reshape(-1, 3)
frames = np.zeros((6, 9), np.float32)          # normal, tangent, bitangent of the six faces: t x b = n
for f in range(6):
    a, s = f // 2, (-1.0 if f & 1 else 1.0)
    n = np.zeros(3); n[a] = s
    t = np.cross([1.0, 0, 0] if a == 1 else [0, 1.0, 0], n)
    frames[f] = np.concatenate([n, t, np.cross(n, t)])
cubes = np.concatenate([np.repeat(centres[:, None, :], 6, axis=1), np.broadcast_to(frames, (centres.shape[0], 6, 9))], axis=2)
cubes = np.ascontiguousarray(cubes.reshape(-1, 12), np.float32)
carms = [Arm("ambient cubes 64^3", cubes, False), Arm("ambient cubes 64^3 + SORT_CELLS", cubes, True)]
alternate(ctx, stream, carms)
lines.append(f"ambient cubes: {cubes.shape[0]} gathers over the scene's bounds, probe-major order (six faces of a probe in a row)")
for a in carms:
    m = np.median(a.march)
    lines.append(f"  {a.label:32s} march {stats(a.march)}  whole call {stats(a.call)}  (keys + sort: "
                 f"{np.median(np.array(a.call) - np.array(a.march)):.4f} ms)  steps {a.steps}  {a.steps / m / 1e6:.1f} Gsteps/s")
assert carms[0].steps == carms[1].steps
assert np.array_equal(carms[0].out.cpu().numpy().view(np.uint32), carms[1].out.cpu().numpy().view(np.uint32))
ctx.close()
txt = "\n".join(lines)
print(txt)
out = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "point_query_probe.txt"), "w") as f:
    f.write(txt + "\n")
