"""ON THE GPU BOX: what drawing the dynamic mesh costs (include/vct.h "dynamic mesh", vct_set_dynamic_draw), what it costs
with the flags off, and what the only earlier route cost.

The procedural atrium at 256^3, 1920 x 1080, a 4096^2 shadow map, one context.  A mover -- a tessellated box of 972,
10,092 and 99,372 triangles, 6 world units across, above the floor in view of the camera, its positions in device memory
-- and per mover, medians over ROUNDS alternating rounds, HIP events on the context's stream:
  * vct_render_shadow_map and vct_render_gbuffer with both flags on against both flags off, same context, same mesh;
  * vct_update_dynamic_positions with the flags on (copy + k_dyn_draw_prepare) against off (copy): the prepare kernel;
  * wall time of update + the two passes drawn, against the route a caller had: vct_upload_triangles +
    vct_upload_mesh_attributes of scene and mover as ONE mesh, then the same two passes.
The drawn G-buffer differs from the static one and the flags-off G-buffer is bit for bit the detached one (asserted).
COMPAT=1: only the two passes detached and attached with the flags off, through entry points the parent commit has -- run
from a checkout of the parent and from this tree alternately (tools/dynamic_draw_probe.sh does).
EMISSION_ONLY=1: only vct_render_gbuffer with the 10,092-triangle mover drawn, without and with an emission table on the
mover (vct_set_dynamic_emission), alternating: what the DYN shade kernel pays for the pixel-emission planes.
Writes dynamic_draw_probe.txt (or dynamic_draw_probe_compat.txt / dynamic_draw_probe_emission.txt) to $OUT (default: tool_out/)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vctpkg  # noqa: E402

vct = vctpkg.load()
from voxel_cone_tracing_amd import scene as sc  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "9"))
REPS = int(os.environ.get("REPS", "10"))          # passes per timed bracket
COMPAT = os.environ.get("COMPAT", "0") == "1"
SIDES = [int(x) for x in os.environ.get("SIDES", "9,29,91").split(",")]       # 12 n^2 triangles: 972, 10092, 99372
light = (0.0, 1.0, 0.25)
w, h, S, V = 1920, 1080, 4096, 256
MS = 0.05


def ev():
    return torch.cuda.Event(enable_timing=True)


def stats(v):
    v = np.array(v)
    return f"{np.median(v):.4f} ms (min {v.min():.4f} max {v.max():.4f})"


def box(n, size):
    """A cube of edge `size` (model units) about the origin, every face n x n quads, outward CCW: [12 n^2, 3, 3] float64."""
    g = np.linspace(-0.5 * size, 0.5 * size, n + 1)
    a0, b0 = np.meshgrid(g[:-1], g[:-1], indexing="ij")
    a1, b1 = np.meshgrid(g[1:], g[1:], indexing="ij")
    quads = np.stack([np.stack([a0, b0], -1), np.stack([a1, b0], -1), np.stack([a1, b1], -1), np.stack([a0, b1], -1)], 2).reshape(-1, 4, 2)
    faces = []
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            order = ([0, 1, 2], [0, 2, 3]) if sgn > 0 else ([0, 2, 1], [0, 3, 2])
            tris = np.concatenate([quads[:, order[0]], quads[:, order[1]]])
            f = np.zeros((tris.shape[0], 3, 3))
            f[..., (axis + 1) % 3] = tris[..., 0]
            f[..., (axis + 2) % 3] = tris[..., 1]
            f[..., axis] = sgn * 0.5 * size
            faces.append(f)
    return np.concatenate(faces)


scene = sc.Scene(sc.ATRIUM, 1.0, 1234)
cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(light)
ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
ctx.upload_scene(scene)
ctx.set_camera_position(tuple(cam.position))
ctx.set_light_direction(light)
st = torch.cuda.ExternalStream(ctx.stream())


def timed(fn, reps=REPS):
    """Device ms per call of fn, REPS calls in one bracket of events on the context's stream."""
    ctx.synchronize()
    e = [ev(), ev()]
    with torch.cuda.stream(st):
        e[0].record()
        for _ in range(reps):
            fn()
        e[1].record()
    ctx.synchronize()
    return e[0].elapsed_time(e[1]) / reps


def wall(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def shadow():
    ctx.render_shadow_map(lvp)


def gbuffer():
    ctx.render_gbuffer(vp)


def mover(n):
    tris = box(n, 6.0 / MS)
    mat = (np.arange(tris.shape[0]) % 3).astype(np.int32)
    alb = np.array([[0.9, 0.2, 0.2, 1.0], [0.2, 0.9, 0.2, 1.0], [0.2, 0.2, 0.9, 1.0]], np.float32)
    path = [np.array([x, -9.0, 1.0]) / MS for x in np.linspace(-40.0, -20.0, 8)]
    host = [np.ascontiguousarray((tris + c[None, None, :]).reshape(-1, 9), np.float32) for c in path]
    return host, mat, alb


for _ in range(3):
    shadow(); gbuffer()
ctx.synchronize()
out_dir = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out_dir, exist_ok=True)

if COMPAT:
    host, mat, alb = mover(29)
    t = {k: [] for k in ("s0", "g0", "s1", "g1")}
    for r in range(ROUNDS):
        ctx.set_dynamic_mesh(None)
        shadow(); gbuffer()
        t["s0"].append(timed(shadow)); t["g0"].append(timed(gbuffer))
        ctx.set_dynamic_mesh(host[0], mat, alb)
        shadow(); gbuffer()
        t["s1"].append(timed(shadow)); t["g1"].append(timed(gbuffer))
    txt = (f"dynamic_draw_probe compat ({os.environ.get('LABEL', 'this tree')}): detached shadow {stats(t['s0'])}  gbuffer {stats(t['g0'])} | "
           f"attached, not drawn shadow {stats(t['s1'])}  gbuffer {stats(t['g1'])}")
    print(txt)
    with open(os.path.join(out_dir, "dynamic_draw_probe_compat.txt"), "a") as f:
        f.write(txt + "\n")
    sys.exit(0)

BOTH = vct.DYNAMIC_DRAW_SHADOW | vct.DYNAMIC_DRAW_GBUFFER
if os.environ.get("EMISSION_ONLY", "0") == "1":
    # vct_render_gbuffer with the mover drawn: without an emission table on the mover, with one (vct_set_dynamic_emission:
    # the DYN shade kernel also writes the pixel-emission planes), alternating; the 10,092-triangle box
    host, mat, alb = mover(29)
    table = np.array([[0.9, 0.35, 0.1], [0.0, 0.0, 0.0], [0.25, 2.0, 0.6]], np.float32)
    ctx.set_dynamic_mesh(host[0], mat, alb)
    ctx.set_dynamic_draw(BOTH, (0.2, 0.2, 0.2))
    t = {k: [] for k in ("plain", "table")}
    for r in range(ROUNDS):
        ctx.set_dynamic_emission(None)
        shadow(); gbuffer()
        t["plain"].append(timed(gbuffer))
        ctx.set_dynamic_emission(table)
        shadow(); gbuffer()
        t["table"].append(timed(gbuffer))
    lit = int((ctx.download_pixel_emission() > 0).any(0).sum())
    txt = (f"dynamic_draw_probe emission: atrium {w}x{h}, mover of {host[0].shape[0]} triangles drawn: vct_render_gbuffer without a table "
           f"{stats(t['plain'])}   with a table {stats(t['table'])} ({lit} emitting pixels)   +{np.median(t['table']) - np.median(t['plain']):.4f} ms")
    print(txt)
    with open(os.path.join(out_dir, "dynamic_draw_probe_emission.txt"), "w") as f:
        f.write(txt + "\n")
    sys.exit(0)
lines = [f"dynamic_draw_probe: atrium {V}^3 ({scene.pos.shape[0]} static triangles), {w}x{h}, shadow map {S}^2, "
         f"{ROUNDS} alternating rounds of {REPS} passes"]
shadow(); gbuffer()
gb_static = ctx.download_gbuffer()
frames = scene.frames()
for n in SIDES:
    host, mat, alb = mover(n)
    ntri = host[0].shape[0]
    dev = [torch.from_numpy(a).cuda() for a in host]
    torch.cuda.synchronize()
    ctx.set_dynamic_mesh(host[0], mat, alb)
    t = {k: [] for k in ("s_off", "g_off", "s_on", "g_on", "u_off", "u_on", "w_draw", "w_up")}
    for r in range(ROUNDS):
        k = r % len(dev)
        ctx.set_dynamic_draw(0)
        shadow(); gbuffer()
        if r == 0:
            assert np.array_equal(ctx.download_gbuffer().view(np.uint32), gb_static.view(np.uint32)), "flags off is not the static G-buffer"
        t["s_off"].append(timed(shadow)); t["g_off"].append(timed(gbuffer))
        t["u_off"].append(timed(lambda: ctx.update_dynamic_positions(dev[k].data_ptr())))
        ctx.set_dynamic_draw(BOTH, (0.2, 0.2, 0.2))
        shadow(); gbuffer()
        if r == 0:
            shown = (ctx.download_gbuffer().view(np.uint32) != gb_static.view(np.uint32)).any(0).sum()
            assert shown > 1000, "the mover is not in the frame"
        t["s_on"].append(timed(shadow)); t["g_on"].append(timed(gbuffer))
        t["u_on"].append(timed(lambda: ctx.update_dynamic_positions(dev[k].data_ptr())))
        t["w_draw"].append(wall(lambda: (ctx.update_dynamic_positions(dev[k].data_ptr()), shadow(), gbuffer())))
    ctx.set_dynamic_draw(0)
    ctx.set_dynamic_mesh(None)
    # the earlier route: scene and mover as one mesh, triangles and attributes again
    spec = np.concatenate([scene.specular.reshape(-1, 3), np.full((3, 3), 0.2, np.float32)])
    material = np.concatenate([scene.material, mat + scene.albedo.reshape(-1, 4).shape[0]]).astype(np.int32)
    albedo = np.concatenate([scene.albedo.reshape(-1, 4), alb])
    mover_frames = [np.tile(np.array(v, np.float32), (ntri, 3)) for v in ((0, 1, 0), (1, 0, 0), (0, 0, 1))]
    fr = [np.concatenate([np.asarray(a, np.float32).reshape(-1, 9), b]) for a, b in zip(frames, mover_frames)]
    for r in range(ROUNDS):
        pos = np.concatenate([scene.pos.reshape(-1, 9), host[r % len(host)]])
        t["w_up"].append(wall(lambda: (ctx.upload_triangles(pos, material, albedo), ctx.upload_mesh_attributes(*fr, spec),
                                       shadow(), gbuffer())))
    ctx.upload_scene(scene)
    shadow(); gbuffer()
    prep = np.median(t["u_on"]) - np.median(t["u_off"])
    lines += [f"mover of {ntri} triangles ({int(shown)} pixels differ from the static frame)",
              f"  vct_render_shadow_map   flags off {stats(t['s_off'])}   both flags {stats(t['s_on'])}   +{np.median(t['s_on']) - np.median(t['s_off']):.4f} ms",
              f"  vct_render_gbuffer      flags off {stats(t['g_off'])}   both flags {stats(t['g_on'])}   +{np.median(t['g_on']) - np.median(t['g_off']):.4f} ms",
              f"  vct_update_dynamic_positions (device pointer)   copy {stats(t['u_off'])}   copy + prepare {stats(t['u_on'])}   prepare ~{prep:.4f} ms",
              f"  wall: update + two passes drawn {stats(t['w_draw'])}   upload as one mesh + two passes {stats(t['w_up'])}   "
              f"drawn / re-upload {np.median(t['w_draw']) / np.median(t['w_up']):.3f}"]
    print("\n".join(lines[-5:]), flush=True)
ctx.close()
with open(os.path.join(out_dir, "dynamic_draw_probe.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
