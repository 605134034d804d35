"""ON THE GPU BOX: what corner normals on the dynamic mesh cost (include/vct.h "dynamic mesh", Normals).

The set-up of tools/dynamic_skin_probe.py: the procedural atrium at 256^3, 1080p, a 4096^2 shadow map, one context, a
mover -- a tessellated box of 972, 10,092 and 99,372 triangles, 6 world units across -- in the hall, both draw flags on.
The corner normals are unit(p - centre): a rounded box, every corner within 55 degrees of its face.  After a warm-up,
ROUNDS alternating rounds per arm, HIP events on the context's stream around 10 updates per bracket, medians with min and
max of the time per update:
  * the three prepare kernels behind an update with and without normals: positions (a device pointer: a device-to-device
    copy + k_dyn_draw_prepare<POS>), 64 parts and 64 bones (the matrix copy + the mover's form of the kernel);
  * update (64 bones) + vct_render_shadow_map + vct_render_gbuffer, wall time to the end of the stream;
  * the resident step (vct_trace_resident) over the smooth G-buffer against the faceted one at diffuse rate 1 and 2, with
    the executed steps and, at rate 2, the pixels that marched their own diffuse cones.
BASELINE_ONLY=1 (LABEL=name): only entry points the parent commit has -- the shadow stage, the G-buffer stage and the
resident step, detached and with the 10,092-triangle mover attached and drawn without normals; one line per figure is
appended to $OUT/dynamic_normals_baseline.txt.  tools/dynamic_normals_probe.sh alternates that mode between this tree and
a built checkout of the parent.  Writes dynamic_normals_probe.txt to $OUT (default: tool_out/)."""
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

ROUNDS = int(os.environ.get("ROUNDS", "7"))
SIDES = [int(x) for x in os.environ.get("SIDES", "9,29,91").split(",")]       # 12 n^2 triangles: 972, 10092, 99372
BASELINE_ONLY = os.environ.get("BASELINE_ONLY", "0") == "1"
LABEL = os.environ.get("LABEL", "this tree")
PER = 10                       # updates per bracket
N = 64                         # parts, bones
light = (0.0, 1.0, 0.25)
w, h, S, V = 1920, 1080, 4096, 256
MS = 0.05
f32 = np.float32


def ev():
    return torch.cuda.Event(enable_timing=True)


def stats(v):
    v = np.array(v)
    return f"{np.median(v):.4f} ms ({v.min():.4f} - {v.max():.4f})"


# the mover, the influences and the matrices of tools/dynamic_skin_probe.py (that file runs its probe when imported)
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


def chain_influences(tris, size, nb):
    """(bone int32 [ntri, 3, 4], weight float32 [ntri, 3, 4]): the two bones of a chain of nb next to each corner's x."""
    u = np.clip(tris[..., 0] / size + 0.5, 0.0, 1.0) * (nb - 1)
    b0 = np.minimum(np.floor(u).astype(np.int32), nb - 2)
    fr = (u - b0).astype(f32)
    bone = np.stack([b0, b0 + 1, b0, b0], -1).astype(np.int32)
    weight = np.stack([1.0 - fr, fr, np.zeros_like(fr), np.zeros_like(fr)], -1).astype(f32)
    return np.ascontiguousarray(bone), np.ascontiguousarray(weight)


def chain_matrices(nb, centre, twist_deg):
    """float32 [nb, 12]: bone b turns by twist_deg * b / (nb - 1) about the x axis through the origin, then moves to centre."""
    t = np.deg2rad(twist_deg) * np.arange(nb) / max(nb - 1, 1)
    m = np.zeros((nb, 3, 4))
    m[:, 0, 0] = 1.0
    m[:, 1, 1] = m[:, 2, 2] = np.cos(t)
    m[:, 1, 2] = -np.sin(t)
    m[:, 2, 1] = np.sin(t)
    m[:, :, 3] = centre
    return np.ascontiguousarray(m.astype(f32).reshape(nb, 12))


scene = sc.Scene(sc.ATRIUM, 1.0, 1234)
cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(light)
ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
ctx.upload_scene(scene)
ctx.set_camera_position(tuple(cam.position))
ctx.set_light_direction(light)
ctx.set_trace_timing(False)
st = torch.cuda.ExternalStream(ctx.stream())
out_dir = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out_dir, exist_ok=True)
size = 6.0 / MS
centre = np.array([0.0, -9.0, 1.0]) / MS
ALB = np.array([[0.9, 0.2, 0.2, 1.0], [0.2, 0.9, 0.2, 1.0], [0.2, 0.2, 0.9, 1.0]], f32)


def bracket(call, n=PER):
    """(event ms, wall ms to the end of the stream) per call of n calls issued back to back"""
    ctx.synchronize()
    e = [ev(), ev()]
    t0 = time.perf_counter()
    with torch.cuda.stream(st):
        e[0].record()
        for _ in range(n):
            call()
        e[1].record()
    ctx.synchronize()
    return e[0].elapsed_time(e[1]) / n, (time.perf_counter() - t0) * 1e3 / n


def mover(n):
    tris = box(n, size)
    rest = np.ascontiguousarray(tris.reshape(-1, 9), f32)
    placed = np.ascontiguousarray((tris + centre[None, None, :]).reshape(-1, 9), f32)
    mat = (np.arange(tris.shape[0]) % 3).astype(np.int32)
    nrm = tris / np.linalg.norm(tris, axis=-1, keepdims=True)
    return tris, rest, placed, mat, np.ascontiguousarray(nrm.astype(f32))


def stages():
    ctx.render_shadow_map(lvp)
    ctx.render_gbuffer(vp)


def baseline():
    """shadow stage, G-buffer stage, resident step: detached, then attached and drawn without normals"""
    lines = []
    _, _, placed, mat, _ = mover(29)
    for state in ("detached", "attached, no normals"):
        if state != "detached":
            ctx.set_dynamic_draw(3)
            ctx.set_dynamic_mesh(placed, mat, ALB)
        ctx.gi_pass(lvp, vp)
        ctx.synchronize()
        figs = {"shadow stage": [], "G-buffer stage": [], "resident step": []}
        for r in range(ROUNDS + 1):
            for name, call in (("shadow stage", lambda: ctx.render_shadow_map(lvp)), ("G-buffer stage", lambda: ctx.render_gbuffer(vp)),
                               ("resident step", ctx.trace_resident)):
                v = bracket(call)[0]
                if r:
                    figs[name].append(v)
        for name, v in figs.items():
            lines.append(f"{LABEL:10s} {state:22s} {name:15s} {stats(v)}")
    with open(os.path.join(out_dir, "dynamic_normals_baseline.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def probe():
    out = [f"dynamic_normals_probe: atrium {V}^3 ({scene.pos.shape[0]} static triangles), {w} x {h}, shadow map {S}^2, {ROUNDS} alternating "
           f"rounds, {PER} updates per bracket, medians (min - max) per update"]
    ctx.set_dynamic_draw(3)
    for n in SIDES:
        tris, rest, placed, mat, nrm = mover(n)
        ntri = tris.shape[0]
        first = len(out)
        out.append(f"mover of {ntri} triangles ({ntri * 36} bytes of positions, {ntri * 36} of corner normals):")
        ctx.set_dynamic_mesh(placed, mat, ALB)
        dev = torch.from_numpy(placed).cuda()
        torch.cuda.synchronize()
        bone, weight = chain_influences(tris, size, N)
        part = (np.arange(ntri) * N // ntri).astype(np.int32)
        m_parts, m_skin = chain_matrices(N, centre, 0.0), chain_matrices(N, centre, 90.0)
        arms = (("positions (device pointer)", None, lambda: ctx.update_dynamic_positions(int(dev.data_ptr()))),
                ("64 parts", lambda: ctx.set_dynamic_parts(part, N), lambda: ctx.update_dynamic_transforms(m_parts)),
                ("64 bones", lambda: ctx.set_dynamic_skin(bone, weight, N), lambda: ctx.update_dynamic_transforms(m_skin)))
        for name, attach, update in arms:
            ctx.set_dynamic_normals(None)
            ctx.set_dynamic_parts(None); ctx.set_dynamic_skin(None, None)
            if attach:
                ctx.update_dynamic_positions(rest)
                attach()
            t = {False: [], True: []}
            for r in range(ROUNDS + 1):
                for on in (False, True):
                    ctx.set_dynamic_normals(nrm if on else None)
                    v = bracket(update)[0]
                    if r:                                     # round 0 warms up
                        t[on].append(v)
            out.append(f"  update, {name:27s} without normals {stats(t[False])}   with {stats(t[True])}")
        # the skin is still attached: update + both drawn stages, then the resident step over either G-buffer
        wall = {False: [], True: []}
        for r in range(ROUNDS + 1):
            for on in (False, True):
                ctx.set_dynamic_normals(nrm if on else None)
                v = bracket(lambda: (ctx.update_dynamic_transforms(m_skin), stages()), 1)[1]
                if r:
                    wall[on].append(v)
        out.append(f"  update (64 bones) + shadow stage + G-buffer stage, wall: without normals {stats(wall[False])}   with {stats(wall[True])}")
        ctx.set_dynamic_normals(None)
        ctx.gi_pass(lvp, vp)                                  # the chain with the mover in it
        for rate in (1, 2):
            ctx.set_diffuse_rate(rate)
            t, steps, marched = {False: [], True: []}, {}, {}
            for r in range(ROUNDS + 1):
                for on in (False, True):
                    ctx.set_dynamic_normals(nrm if on else None)
                    ctx.render_gbuffer(vp)
                    v = bracket(ctx.trace_resident, 3)[0]
                    if r:
                        t[on].append(v)
                    steps[on], marched[on] = ctx.last_step_count(), ctx.diffuse_rate()[1]      # (both wait for the stream)
            extra = f"; pixels marching their own diffuse cones {marched[False]} / {marched[True]}" if rate == 2 else ""
            out.append(f"  resident step, rate {rate}: faceted {stats(t[False])}   smooth {stats(t[True])}; executed steps "
                       f"{steps[False]} / {steps[True]}{extra}")
        ctx.set_diffuse_rate(1)
        ctx.set_dynamic_mesh(None)
        print("\n".join(out[first:]), flush=True)
    with open(os.path.join(out_dir, "dynamic_normals_probe.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


ctx.gi_pass(lvp, vp)
ctx.synchronize()
if BASELINE_ONLY:
    baseline()
else:
    probe()
ctx.close()
