"""ON THE GPU BOX: what the second bounce costs over a chain the dynamic mesh was merged into (include/vct.h "dynamic
mesh", vct_set_dynamic_bounce), beside the plain bounce of the same context.

The procedural atrium at V^3 (default 256; V=512 is BASELINE configs[2]' grid) with voxel attributes and its 4096^2
shadow map, one context.  Movers as in tools/dynamic_probe.py: a tessellated box of 972 / 10,092 / 99,372 triangles, 6
world units across, above the floor.  Per mover, ROUNDS alternating rounds, each bracket HIP events around BOUNCES
vct_bounce calls after a warm-up:
  * vct_bounce detached (the parent's kernels), and attached with the switch on (the DYN kernels + the table kernel);
    ms per bounce, executed steps (vct_last_step_count), ms per million steps;
  * for the ~10 k mover the caller's alternative: vct_upload_triangles of scene + mover as ONE mesh, then pass + bounce,
    in wall time (only the triangles are uploaded again: a lower bound) against update + pass + bounce attached.
MODE=detached: only the plain bounce and the resident step, through entry points every earlier version has -- run from a
checkout of the parent commit and from this tree alternately (tools/dynamic_bounce_probe.sh does).
MODE=loop: nothing but LOOP attached bounces, for a kernel trace of the table kernel alone (the .sh runs it under the
profiler in a run of its own).
Writes dynamic_bounce_probe.txt (or _detached.txt) to $OUT (default: tool_out/)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vctpkg  # noqa: E402

vct = vctpkg.load()
from voxel_cone_tracing_amd import scene as sc  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "7"))
BOUNCES = int(os.environ.get("BOUNCES", "10"))
STEPS = int(os.environ.get("STEPS", "40"))
MODE = os.environ.get("MODE", "full")
SIDES = [int(x) for x in os.environ.get("SIDES", "9,29,91").split(",")]       # 12 n^2 triangles: 972, 10092, 99372
V = int(os.environ.get("V", "256"))
light = (0.0, 1.0, 0.25)
w, h, S = 1920, 1080, 4096
MS = 0.05


def ev():
    return torch.cuda.Event(enable_timing=True)


def stats(v, unit="ms"):
    v = np.array(v)
    return f"{np.median(v):.4f} {unit} (min {v.min():.4f} max {v.max():.4f})"


def box(n, size):
    """A cube of edge `size` (model units) about the origin, every face n x n quads: [12 n^2, 3, 3] float64."""
    g = np.linspace(-0.5 * size, 0.5 * size, n + 1)
    a0, b0 = np.meshgrid(g[:-1], g[:-1], indexing="ij")
    a1, b1 = np.meshgrid(g[1:], g[1:], indexing="ij")
    quads = np.stack([np.stack([a0, b0], -1), np.stack([a1, b0], -1), np.stack([a1, b1], -1), np.stack([a0, b1], -1)], 2).reshape(-1, 4, 2)
    tris = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]])
    faces = []
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            f = np.zeros((tris.shape[0], 3, 3))
            f[..., (axis + 1) % 3] = tris[..., 0]
            f[..., (axis + 2) % 3] = tris[..., 1]
            f[..., axis] = sgn * 0.5 * size
            faces.append(f)
    return np.concatenate(faces)


scene = sc.Scene(sc.ATRIUM, 1.0, 1234)
cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(light)
ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S, voxel_attributes=1))
ctx.upload_scene(scene)
ctx.set_camera_position(tuple(cam.position))
ctx.set_light_direction(light)
ctx.render_shadow_map(lvp)
st = torch.cuda.ExternalStream(ctx.stream())


def run_pass():
    ctx.voxelize(); ctx.inject_light(); ctx.build_mips()


def bounce_ms():
    """(ms per bounce over BOUNCES bounces between two events, executed steps of one)"""
    for _ in range(3):
        ctx.bounce()
    ctx.synchronize()
    e = [ev(), ev()]
    with torch.cuda.stream(st):
        e[0].record()
        for _ in range(BOUNCES):
            ctx.bounce()
        e[1].record()
    ctx.synchronize()
    return e[0].elapsed_time(e[1]) / BOUNCES, ctx.last_step_count()


def step_ms():
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


def wall(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


run_pass()
ctx.render_gbuffer(vp)
ctx.trace_resident()
ctx.synchronize()
out_dir = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out_dir, exist_ok=True)

if MODE == "detached":
    b, s = [], []
    for _ in range(ROUNDS):
        run_pass()
        b.append(bounce_ms())
        run_pass()
        ctx.render_gbuffer(vp)
        s.append(step_ms())
    txt = (f"dynamic_bounce_probe detached ({os.environ.get('LABEL', 'this tree')}): atrium {V}^3, {w}x{h}: bounce "
           f"{stats([x[0] for x in b])}, {b[0][1]} steps; resident step {stats(s)}")
    print(txt)
    with open(os.path.join(out_dir, "dynamic_bounce_probe_detached.txt"), "a") as f:
        f.write(txt + "\n")
    sys.exit(0)

alb = np.array([[0.9, 0.2, 0.2, 1.0], [0.2, 0.9, 0.2, 1.0], [0.2, 0.2, 0.9, 1.0]], np.float32)
centre = np.array([0.0, -9.0, 1.0]) / MS


def mover(n, c=centre):
    tris = box(n, 6.0 / MS)
    return np.ascontiguousarray((tris + c[None, None, :]).reshape(-1, 9), np.float32), (np.arange(tris.shape[0]) % 3).astype(np.int32)


if MODE == "loop":
    pos, mat = mover(SIDES[len(SIDES) // 2])
    ctx.set_dynamic_bounce(True)
    ctx.set_dynamic_mesh(pos, mat, alb)
    run_pass()
    for _ in range(int(os.environ.get("LOOP", "30"))):
        ctx.bounce()
    ctx.synchronize()
    sys.exit(0)

ctx.set_dynamic_bounce(True)
lines = [f"dynamic_bounce_probe: atrium {V}^3 ({scene.pos.shape[0]} static triangles), shadow map {S}^2, {ROUNDS} alternating rounds, "
         f"{BOUNCES} bounces per bracket"]
for n in SIDES:
    pos, mat = mover(n)
    ntri = pos.shape[0]
    t = {k: [] for k in ("det", "att")}
    steps = {}
    for r in range(ROUNDS):
        ctx.set_dynamic_mesh(None)
        run_pass()
        ms, steps["det"] = bounce_ms()
        t["det"].append(ms)
        if r == 0:
            chain_det = ctx.download_chain()
        ctx.set_dynamic_mesh(pos, mat, alb)
        run_pass()
        ms, steps["att"] = bounce_ms()
        t["att"].append(ms)
        info = ctx.dynamic_info()
        assert not info["left_out"], info
        if r == 0:
            assert not np.array_equal(ctx.download_chain(), chain_det), "the mover changed nothing in the bounce chain"
    rate = {k: np.array(t[k]) / (steps[k] * 1e-6) for k in t}
    lines += [f"mover of {ntri} triangles: bricks {info['bricks_used']} of {info['max_bricks']} slots, {info['fragments']} fragments",
              f"  vct_bounce detached     {stats(t['det'])}   {steps['det']} steps   {stats(rate['det'], 'ms/Msteps')}",
              f"  vct_bounce attached, on {stats(t['att'])}   {steps['att']} steps   {stats(rate['att'], 'ms/Msteps')}"]
    print("\n".join(lines[-3:]), flush=True)
    if n == SIDES[len(SIDES) // 2]:
        # the route a caller had: scene + mover as one mesh, uploaded again, then pass + bounce
        path = [mover(n, centre + np.array([x, 0.0, 0.0]) / MS)[0] for x in np.linspace(-20.0, 20.0, 6)]
        dev = [torch.from_numpy(a).cuda() for a in path]
        torch.cuda.synchronize()
        t_up, t_at = [], []
        for r in range(ROUNDS):
            k = r % len(path)

            def attached():
                ctx.update_dynamic_positions(dev[k].data_ptr()); run_pass(); ctx.bounce()
            ctx.set_dynamic_mesh(path[0], mat, alb)
            wall(attached)
            t_at.append(wall(attached))
            ctx.set_dynamic_mesh(None)
            one = np.concatenate([scene.pos.reshape(-1, 9), path[k]])
            material = np.concatenate([scene.material, mat + scene.albedo.shape[0]]).astype(np.int32)
            albedo = np.concatenate([scene.albedo.reshape(-1, 4), alb])

            def reupload():
                ctx.upload_triangles(one, material, albedo); run_pass(); ctx.bounce()
            t_up.append(wall(reupload))
        ctx.upload_scene(scene)
        run_pass()
        lines += [f"  update + pass + bounce attached, wall      {stats(t_at)}",
                  f"  re-upload as one mesh + pass + bounce, wall {stats(t_up)}",
                  f"  attached / re-upload wall: {np.median(t_at) / np.median(t_up):.3f}"]
        print("\n".join(lines[-3:]), flush=True)
ctx.close()
with open(os.path.join(out_dir, "dynamic_bounce_probe.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
