"""ON THE GPU BOX: what a dynamic mesh costs (include/vct.h "dynamic mesh"), and what the only earlier route cost.

The procedural atrium at 256^3 with its 4096^2 shadow map, one context.  A mover -- a tessellated box of about 1 k, 10 k
and 100 k triangles, 6 world units across, crossing the hall above the floor, its positions in device memory as a
renderer has them -- and per mover, medians over ROUNDS rounds:
  * the two times of vct_last_dynamic_ms (slots + fragments kernels of vct_voxelize; the merge of vct_inject_light);
  * update + vct_voxelize + vct_inject_light + vct_build_mips: HIP events on the stream, the host time until the four
    calls have returned, and the wall time until the stream has finished;
  * the same pass detached (static only), alternating with the attached one;
  * the route a caller had before: vct_upload_triangles of static + mover concatenated, then the same pass -- wall time.
    (Only the triangles are uploaded again, not the mesh attributes and textures a renderer would also have to hand
    over: a lower bound of that route.)
  * with an emission table on the mover (vct_set_dynamic_emission), on one of its three materials and on all of them:
    the two kernel times and the attached pass again, alternating with the plain one; and the earlier route of a glowing
    mover, vct_upload_triangles + vct_upload_emission of scene plus mover every frame.  (A library without the entry
    point -- a checkout of the parent commit -- skips these lines; NO_REUPLOAD=1 skips both re-upload routes.)
The chain with the mover differs from the static one (asserted); the detached chain is bit for bit the first one (asserted).
DETACHED_ONLY=1: only the static pass and the resident step, through entry points every earlier version of the library
has -- run from a checkout of the parent commit and from this tree alternately (tools/dynamic_probe.sh does).
PARTS=1: only the routes that move the mover -- positions from host and from device memory against
vct_update_dynamic_transforms with 1 and 64 parts (parts_probe below); a checkout of the parent commit runs the two positions
routes.  Writes dynamic_probe.txt (or dynamic_probe_detached.txt, or with PARTS=1 $PARTS_FILE, default
dynamic_parts_probe.txt) to $OUT (default: tool_out/)."""
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

ROUNDS = int(os.environ.get("ROUNDS", "9"))
STEPS = int(os.environ.get("STEPS", "40"))
DETACHED_ONLY = os.environ.get("DETACHED_ONLY", "0") == "1"
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
ctx = vct.Context(vct.default_config(voxel_dim=V, width=w, height=h, shadow_map_size=S))
ctx.upload_scene(scene)
ctx.set_camera_position(tuple(cam.position))
ctx.set_light_direction(light)
ctx.render_shadow_map(lvp)
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


for _ in range(3):
    timed_pass()
ctx.render_gbuffer(vp)
ctx.trace_resident()
ctx.synchronize()

out_dir = os.environ.get("OUT", os.path.join(ROOT, "tool_out"))
os.makedirs(out_dir, exist_ok=True)
if DETACHED_ONLY:
    p = [timed_pass() for _ in range(ROUNDS)]
    s = [step_ms() for _ in range(ROUNDS)]
    txt = (f"dynamic_probe detached ({os.environ.get('LABEL', 'this tree')}): atrium {V}^3, {w}x{h}: voxelize + inject + mips "
           f"{stats([x[0] for x in p])}, wall {stats([x[2] for x in p])}; resident step {stats(s)}")
    print(txt)
    with open(os.path.join(out_dir, "dynamic_probe_detached.txt"), "a") as f:
        f.write(txt + "\n")
    sys.exit(0)

NPOS = 8


def parts_probe():
    """PARTS=1: the routes that move the mover, alternating on one context -- positions from host memory (what a caller
    without device-side transforms does), positions from device memory, and vct_update_dynamic_transforms with the mover as
    1 part and as 64 parts (each a 64th of the triangles, the same translation).  Per route update + voxelize + inject +
    mips as events, host time and wall time; the transform kernel's device time; with both draw flags on, the PARTS form of
    the prepare kernel against k_dyn_transform (k_dyn_move<DYN_SRC_PARTS> now; the printed label keeps the old name)
    followed by the plain prepare (events around the calls); and what NumPy
    takes to move the vertices on the host.  A library without the entry point (the parent commit) runs the two positions
    routes only.  Writes dynamic_parts_probe.txt."""
    have = hasattr(ctx, "update_dynamic_transforms")
    label = os.environ.get("LABEL", "this tree")
    out = [f"dynamic_parts_probe ({label}): atrium {V}^3 ({scene.pos.shape[0]} static triangles), shadow map {S}^2, "
           f"{ROUNDS} alternating rounds, medians (min max)"]

    def bracket(call):
        ctx.synchronize()
        e = [ev(), ev()]
        with torch.cuda.stream(st):
            e[0].record()
            call()
            e[1].record()
        ctx.synchronize()
        return e[0].elapsed_time(e[1])
    for n in SIDES:
        tris = box(n, 6.0 / MS)
        ntri = tris.shape[0]
        mat = (np.arange(ntri) % 3).astype(np.int32)
        alb = np.array([[0.9, 0.2, 0.2, 1.0], [0.2, 0.9, 0.2, 1.0], [0.2, 0.2, 0.9, 1.0]], np.float32)
        path = [np.array([x, -9.0, 1.0]) / MS for x in np.linspace(-30.0, 30.0, NPOS)]
        rest = np.ascontiguousarray(tris.reshape(-1, 9), np.float32)
        host = [np.ascontiguousarray((tris + c[None, None, :]).reshape(-1, 9), np.float32) for c in path]
        dev = [torch.from_numpy(a).cuda() for a in host]
        torch.cuda.synchronize()
        routes = ["host positions", "device positions"] + (["1 part", "64 parts"] if have else [])
        t = {r: {k: [] for k in ("ev", "host", "wall", "kernel")} for r in routes}
        extra = {k: [] for k in ("numpy", "parts_prepare", "transform_then_prepare", "parts_prepare_timer")}

        def matrices(nparts, k):
            m = np.zeros((nparts, 3, 4), np.float32)
            m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = 1.0
            m[:, :, 3] = path[k].astype(np.float32)
            return m
        ctx.set_dynamic_mesh(host[0], mat, alb)
        for r in range(ROUNDS):
            k = 2 + r % (NPOS - 2)
            for route in routes:
                if route == "host positions":
                    ctx.update_dynamic_positions(rest)
                    move = [lambda: ctx.update_dynamic_positions(host[1]), lambda: ctx.update_dynamic_positions(host[k])]
                elif route == "device positions":
                    move = [lambda: ctx.update_dynamic_positions(dev[1].data_ptr()), lambda: ctx.update_dynamic_positions(dev[k].data_ptr())]
                else:
                    nparts = 1 if route == "1 part" else 64
                    ctx.update_dynamic_positions(rest)
                    ctx.set_dynamic_parts((np.arange(ntri) * nparts // ntri).astype(np.int32), nparts)
                    m1, mk = matrices(nparts, 1), matrices(nparts, k)
                    move = [lambda: ctx.update_dynamic_transforms(m1), lambda: ctx.update_dynamic_transforms(mk)]
                timed_pass(move[0])
                a = timed_pass(move[1])
                t[route]["ev"].append(a[0]); t[route]["host"].append(a[1]); t[route]["wall"].append(a[2])
                info = ctx.dynamic_info()
                assert not info["left_out"] and info["bricks_used"] > 0, info
                if have and route.endswith(("part", "parts")):
                    t[route]["kernel"].append(ctx.last_dynamic_transform_ms())
                    if route == "64 parts":           # drawn: one launch against two
                        ctx.set_dynamic_draw(3)
                        bracket(lambda: ctx.update_dynamic_transforms(m1))
                        extra["parts_prepare"].append(bracket(lambda: ctx.update_dynamic_transforms(mk)))
                        extra["parts_prepare_timer"].append(ctx.last_dynamic_transform_ms())
                        ctx.set_dynamic_draw(0)

                        def two():
                            ctx.update_dynamic_transforms(mk)
                            ctx.set_dynamic_draw(3)
                        bracket(two)
                        ctx.set_dynamic_draw(0)
                        extra["transform_then_prepare"].append(bracket(two))
                        ctx.set_dynamic_draw(0)
                    ctx.set_dynamic_parts(None)
            t0 = time.perf_counter()
            moved = np.ascontiguousarray((rest.reshape(-1, 3) + path[k].astype(np.float32)).reshape(-1, 9))
            extra["numpy"].append((time.perf_counter() - t0) * 1e3)
            assert moved.shape == rest.shape
        ctx.set_dynamic_mesh(None)
        out.append(f"mover of {ntri} triangles ({ntri * 36} bytes of positions, 48 or 3072 of matrices):")
        for route in routes:
            out.append(f"  {route:17s} update + pass: events {stats(t[route]['ev'])}   host {stats(t[route]['host'])}   "
                       f"wall {stats(t[route]['wall'])}" + (f"   transform kernel {stats(t[route]['kernel'])}" if t[route]["kernel"] else ""))
        if have:
            out.append(f"  drawn, 64 parts: PARTS prepare alone, events around the call {stats(extra['parts_prepare'])} "
                       f"(its own timer {stats(extra['parts_prepare_timer'])});   k_dyn_transform + plain prepare, events around "
                       f"both calls {stats(extra['transform_then_prepare'])}")
        out.append(f"  the host's own loop: NumPy adds one translation to {3 * ntri} vertices in {stats(extra['numpy'])}")
        print("\n".join(out[-(len(routes) + 3):]), flush=True)
    with open(os.path.join(out_dir, os.environ.get("PARTS_FILE", "dynamic_parts_probe.txt")), "w") as f:
        f.write("\n".join(out) + "\n")


if os.environ.get("PARTS", "0") == "1":
    parts_probe()
    ctx.close()
    sys.exit(0)

lines = [f"dynamic_probe: atrium {V}^3 ({scene.pos.shape[0]} static triangles), shadow map {S}^2, {ROUNDS} alternating rounds"]
chain0 = ctx.download_chain()
for n in SIDES:
    tris = box(n, 6.0 / MS)
    ntri = tris.shape[0]
    mat = (np.arange(ntri) % 3).astype(np.int32)
    alb = np.array([[0.9, 0.2, 0.2, 1.0], [0.2, 0.9, 0.2, 1.0], [0.2, 0.2, 0.9, 1.0]], np.float32)
    path = [np.array([x, -9.0, 1.0]) / MS for x in np.linspace(-30.0, 30.0, NPOS)]
    host = [np.ascontiguousarray((tris + c[None, None, :]).reshape(-1, 9), np.float32) for c in path]
    dev = [torch.from_numpy(a).cuda() for a in host]
    torch.cuda.synchronize()
    t = {k: [] for k in ("ev0", "host0", "wall0", "ev1", "host1", "wall1", "kvox", "kmerge", "up_wall", "up_ev", "upe_wall", "upe_ev")}
    tables = {"one material": np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.25, 2.0, 0.6]], np.float32),
              "all materials": np.array([[0.9, 0.35, 0.1], [0.5, 0.5, 0.5], [0.25, 2.0, 0.6]], np.float32)}
    if not hasattr(ctx, "set_dynamic_emission"):
        tables = {}
    te = {name: {k: [] for k in ("ev", "wall", "kvox", "kmerge")} for name in tables}
    info = None
    for r in range(ROUNDS):
        ctx.set_dynamic_mesh(None)
        timed_pass()
        a = timed_pass()
        t["ev0"].append(a[0]); t["host0"].append(a[1]); t["wall0"].append(a[2])
        if r == 0:
            assert np.array_equal(ctx.download_chain(), chain0), "detached is not what it was"
        ctx.set_dynamic_mesh(host[0], mat, alb)
        timed_pass(lambda: ctx.update_dynamic_positions(dev[1].data_ptr()))
        k = 2 + r % (NPOS - 2)
        a = timed_pass(lambda: ctx.update_dynamic_positions(dev[k].data_ptr()))
        t["ev1"].append(a[0]); t["host1"].append(a[1]); t["wall1"].append(a[2])
        ms = ctx.last_dynamic_ms()
        t["kvox"].append(ms[0]); t["kmerge"].append(ms[1])
        info = ctx.dynamic_info()
        assert not info["left_out"], info
        if r == 0:
            plain = ctx.download_chain()
            assert not np.array_equal(plain, chain0), "the mover changed nothing in the chain"
        for name, table in tables.items():                # the same positions, the table attached
            ctx.set_dynamic_emission(table)
            timed_pass(lambda: ctx.update_dynamic_positions(dev[1].data_ptr()))
            a = timed_pass(lambda: ctx.update_dynamic_positions(dev[k].data_ptr()))
            ms = ctx.last_dynamic_ms()
            te[name]["ev"].append(a[0]); te[name]["wall"].append(a[2]); te[name]["kvox"].append(ms[0]); te[name]["kmerge"].append(ms[1])
            if r == 0:
                assert not np.array_equal(ctx.download_chain(), plain), "the table changed nothing in the chain"
        if tables:
            ctx.set_dynamic_emission(None)
    ctx.set_dynamic_mesh(None)
    # the earlier route: the whole scene again, mover included
    for r in range(0 if os.environ.get("NO_REUPLOAD", "0") == "1" else ROUNDS):
        k = 2 + r % (NPOS - 2)
        pos = np.concatenate([scene.pos.reshape(-1, 9), host[k]])
        material = np.concatenate([scene.material, mat + scene.albedo.shape[0]]).astype(np.int32)
        albedo = np.concatenate([scene.albedo.reshape(-1, 4), alb])
        a = timed_pass(lambda: ctx.upload_triangles(pos, material, albedo))
        t["up_ev"].append(a[0]); t["up_wall"].append(a[2])
        if tables:                                        # ... and of a glowing mover: the table of scene plus mover too
            em = np.concatenate([np.zeros((scene.albedo.reshape(-1, 4).shape[0], 3), np.float32), tables["all materials"]])

            def upload_both():
                ctx.upload_triangles(pos, material, albedo)
                ctx.upload_emission(em)
            a = timed_pass(upload_both)
            t["upe_ev"].append(a[0]); t["upe_wall"].append(a[2])
    ctx.upload_scene(scene)
    timed_pass()
    if not t["up_wall"]:
        t["up_ev"] = t["up_wall"] = t["upe_ev"] = t["upe_wall"] = [float("nan")]
    lines += [f"mover of {ntri} triangles: bricks {info['bricks_used']} of {info['max_bricks']} slots, {info['fragments']} fragments",
              f"  dynamic kernels (vct_voxelize) {stats(t['kvox'])}   merge (vct_inject_light) {stats(t['kmerge'])}",
              f"  pass detached          events {stats(t['ev0'])}   host {stats(t['host0'])}   wall {stats(t['wall0'])}",
              f"  update + pass attached events {stats(t['ev1'])}   host {stats(t['host1'])}   wall {stats(t['wall1'])}",
              f"  re-upload + pass       events {stats(t['up_ev'])}   wall {stats(t['up_wall'])}",
              f"  attached / re-upload wall: {np.median(t['wall1']) / np.median(t['up_wall']):.3f}"]
    nl = 6
    for name in tables:
        lines += [f"  table on {name}: dynamic kernels {stats(te[name]['kvox'])}   merge {stats(te[name]['kmerge'])}",
                  f"  table on {name}: update + pass attached events {stats(te[name]['ev'])}   wall {stats(te[name]['wall'])}"]
        nl += 2
    if tables and t["upe_wall"]:
        lines += [f"  re-upload with vct_upload_emission + pass events {stats(t['upe_ev'])}   wall {stats(t['upe_wall'])}",
                  f"  attached with a table on all materials / that route, wall: "
                  f"{np.median(te['all materials']['wall']) / np.median(t['upe_wall']):.3f}"]
        nl += 2
    print("\n".join(lines[-nl:]), flush=True)
ctx.close()
txt = "\n".join(lines)
with open(os.path.join(out_dir, "dynamic_probe.txt"), "w") as f:
    f.write(txt + "\n")
