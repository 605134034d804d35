"""ON THE GPU BOX: what skinning the dynamic mesh on the device costs (include/vct.h "dynamic mesh", Skin), and what the
route a caller had before costs -- linear-blend skinning in NumPy plus vct_update_dynamic_positions.

The set-up of tools/dynamic_probe.py: the procedural atrium at 256^3 with its 4096^2 shadow map, one context, a mover -- a
tessellated box of 972, 10,092 and 99,372 triangles, 6 world units across -- crossing the hall.  The box is skinned to a
chain of NB bones along its x axis: a corner at u in [0, 1] along the box blends the two bones next to u (slots 2 and 3
point at the first with weight 0); bone b's matrix is the frame's translation and a rotation about x that grows with b: the
box twists.  Per mover, ROUNDS alternating rounds, medians with min and max:
  * the kernels, by vct_last_dynamic_transform_ms: k_dyn_skin (NB = 2, 64, 4096) and the skin form of the prepare kernel
    (both draw flags on) against k_dyn_transform and the PARTS prepare with 64 parts -- the arms alternate on the context,
    each attaching its mover in turn (the kernels are k_dyn_move<DYN_SRC_SKIN> and k_dyn_move<DYN_SRC_PARTS> now; the
    printed labels keep the old names so that new lines compare with the logged ones);
  * update + vct_voxelize + vct_inject_light + vct_build_mips as events, the host's time inside the calls, and the wall
    time to the end of the stream: matrices (NB = 64) against positions skinned by NumPy on the host (its time apart and
    included) against positions that are already in host memory.
KERNELS_ONLY=1: the first group alone.  Writes $SKIN_FILE (default dynamic_skin_probe.txt) to $OUT (default: tool_out/).
The detached pass and the resident step against a checkout of the parent commit are tools/dynamic_probe.py's
DETACHED_ONLY mode (tools/dynamic_skin_probe.sh runs both)."""
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
SIDES = [int(x) for x in os.environ.get("SIDES", "9,29,91").split(",")]       # 12 n^2 triangles: 972, 10092, 99372
BONES = [int(x) for x in os.environ.get("BONES", "2,64,4096").split(",")]
light = (0.0, 1.0, 0.25)
w, h, S, V = 1920, 1080, 4096, 256
MS = 0.05
KERNELS_ONLY = os.environ.get("KERNELS_ONLY", "0") == "1"      # the kernel arms alone (an A/B of two builds of the library)
NPOS = 8
f32 = np.float32


def ev():
    return torch.cuda.Event(enable_timing=True)


def stats(v):
    v = np.array(v)
    return f"{np.median(v):.4f} ms ({v.min():.4f} - {v.max():.4f})"


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


def numpy_skin(rest, bone, weight, m):
    """Linear-blend skinning as a caller writes it in NumPy (float32, no care for the operation order): [ntri, 9]."""
    M = m.reshape(-1, 3, 4)[bone.reshape(-1, 4)]                                   # [corners, 4, 3, 4]
    B = np.einsum("ck,ckrj->crj", weight.reshape(-1, 4), M)
    p = rest.reshape(-1, 3)
    return np.ascontiguousarray((np.einsum("crj,cj->cr", B[..., :3], p) + B[..., 3]).reshape(-1, 9), f32)


scene = sc.Scene(sc.ATRIUM, 1.0, 1234)
cam = sc.default_camera(position=(-56.0, -9.0, 2.0), yaw=0.0, pitch=8.0)
vp, lvp = sc.camera_view_proj(cam, w, h), sc.light_view_proj(light)
ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
ctx.upload_scene(scene)
ctx.set_camera_position(tuple(cam.position))
ctx.set_light_direction(light)
ctx.render_shadow_map(lvp)
ctx.set_trace_timing(True)
st = torch.cuda.ExternalStream(ctx.stream())


def timed_pass(before=None):
    """(event ms, host ms of the calls, wall ms to the end of the stream) of [before +] voxelize + inject + mips"""
    ctx.synchronize()
    e = [ev(), ev()]
    t0 = time.perf_counter()
    with torch.cuda.stream(st):
        e[0].record()
        if before:
            before()
        ctx.voxelize(); ctx.inject_light(); ctx.build_mips()
        e[1].record()
    t1 = time.perf_counter()
    ctx.synchronize()
    t2 = time.perf_counter()
    return e[0].elapsed_time(e[1]), (t1 - t0) * 1e3, (t2 - t0) * 1e3


for _ in range(3):
    timed_pass()
out_dir = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out_dir, exist_ok=True)
out = [f"dynamic_skin_probe: atrium {V}^3 ({scene.pos.shape[0]} static triangles), shadow map {S}^2, {ROUNDS} alternating rounds, "
       f"medians (min - max)"]
size = 6.0 / MS
for n in SIDES:
    tris = box(n, size)
    ntri = tris.shape[0]
    mat = (np.arange(ntri) % 3).astype(np.int32)
    alb = np.array([[0.9, 0.2, 0.2, 1.0], [0.2, 0.9, 0.2, 1.0], [0.2, 0.2, 0.9, 1.0]], f32)
    path = [np.array([x, -9.0, 1.0]) / MS for x in np.linspace(-30.0, 30.0, NPOS)]
    rest = np.ascontiguousarray(tris.reshape(-1, 9), f32)
    infl = {nb: chain_influences(tris, size, nb) for nb in BONES}
    part64 = (np.arange(ntri) * 64 // ntri).astype(np.int32)
    kern = {f"k_dyn_skin {nb} bones": [] for nb in BONES}
    kern.update({"k_dyn_transform 64 parts": [], "skin prepare 64 bones": [], "PARTS prepare 64 parts": []})
    routes = ("matrices, 64 bones", "NumPy skinning + host positions", "host positions as they are")
    t = {r: {k: [] for k in ("ev", "host", "wall")} for r in routes}
    t_numpy = []
    ctx.set_dynamic_mesh(np.ascontiguousarray((tris + path[0][None, None, :]).reshape(-1, 9), f32), mat, alb)
    checked = False
    for r in range(ROUNDS):
        k = 2 + r % (NPOS - 2)
        # -- the kernels, arms alternating: each attaches its mover, runs one warm-up update and the measured one
        for nb in BONES:
            ctx.update_dynamic_positions(rest)
            ctx.set_dynamic_skin(*infl[nb], nb)
            for kk in (1, k):
                ctx.update_dynamic_transforms(chain_matrices(nb, path[kk], 90.0))
                ctx.synchronize()
            kern[f"k_dyn_skin {nb} bones"].append(ctx.last_dynamic_transform_ms())
            if nb == 64:
                ctx.set_dynamic_draw(3)
                for kk in (1, k):
                    ctx.update_dynamic_transforms(chain_matrices(nb, path[kk], 90.0))
                    ctx.synchronize()
                kern["skin prepare 64 bones"].append(ctx.last_dynamic_transform_ms())
                ctx.set_dynamic_draw(0)
            if not checked and nb == 2:          # the device's positions against the caller's own skinning: the same to rounding
                got = ctx.download_dynamic_positions()
                ref = numpy_skin(rest, *infl[nb], chain_matrices(nb, path[k], 90.0))
                assert np.allclose(got, ref, rtol=1e-4, atol=1e-2), float(np.abs(got - ref).max())
                checked = True
            ctx.set_dynamic_skin(None, None)
        ctx.update_dynamic_positions(rest)
        ctx.set_dynamic_parts(part64, 64)
        for draw, name in ((0, "k_dyn_transform 64 parts"), (3, "PARTS prepare 64 parts")):
            ctx.set_dynamic_draw(draw)
            for kk in (1, k):
                ctx.update_dynamic_transforms(chain_matrices(64, path[kk], 0.0))
                ctx.synchronize()
            kern[name].append(ctx.last_dynamic_transform_ms())
        ctx.set_dynamic_draw(0)
        ctx.set_dynamic_parts(None)
        if KERNELS_ONLY:
            continue
        # -- the routes, alternating
        bone, weight = infl[64]
        m1, mk = chain_matrices(64, path[1], 90.0), chain_matrices(64, path[k], 90.0)
        for route in routes:
            ctx.update_dynamic_positions(rest)
            if route == routes[0]:
                ctx.set_dynamic_skin(bone, weight, 64)
                move = [lambda: ctx.update_dynamic_transforms(m1), lambda: ctx.update_dynamic_transforms(mk)]
            elif route == routes[1]:
                move = [lambda: ctx.update_dynamic_positions(numpy_skin(rest, bone, weight, m1)),
                        lambda: ctx.update_dynamic_positions(numpy_skin(rest, bone, weight, mk))]
            else:
                h1, hk = numpy_skin(rest, bone, weight, m1), numpy_skin(rest, bone, weight, mk)
                move = [lambda: ctx.update_dynamic_positions(h1), lambda: ctx.update_dynamic_positions(hk)]
            timed_pass(move[0])
            a = timed_pass(move[1])
            t[route]["ev"].append(a[0]); t[route]["host"].append(a[1]); t[route]["wall"].append(a[2])
            info = ctx.dynamic_info()
            assert not info["left_out"] and info["bricks_used"] > 0, info
            if route == routes[0]:
                ctx.set_dynamic_skin(None, None)
        t0 = time.perf_counter()
        numpy_skin(rest, bone, weight, mk)
        t_numpy.append((time.perf_counter() - t0) * 1e3)
    ctx.set_dynamic_mesh(None)
    first = len(out)
    out.append(f"mover of {ntri} triangles ({ntri * 36} bytes of positions; {ntri * 72} of influences once; 48 per bone and frame):")
    for name, v in kern.items():
        out.append(f"  kernel {name:26s} {stats(v)}")
    for route in routes if not KERNELS_ONLY else ():
        out.append(f"  {route:32s} update + pass: events {stats(t[route]['ev'])}   host {stats(t[route]['host'])}   wall {stats(t[route]['wall'])}")
    if not KERNELS_ONLY:
        out.append(f"  NumPy linear-blend skinning of {3 * ntri} corners alone: {stats(t_numpy)}")
    print("\n".join(out[first:]), flush=True)
ctx.close()
with open(os.path.join(out_dir, os.environ.get("SKIN_FILE", "dynamic_skin_probe.txt")), "w") as f:
    f.write("\n".join(out) + "\n")
