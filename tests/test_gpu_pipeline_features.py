"""Two frame slots and the calls that came after tests/test_gpu_pipeline.py was written: the state setters (lights, sky, gloss
classes and the material gloss map, emission, diffuse rate, lighting components, per-component outputs, footprint records,
the bounce), the per-slot planes and hand-overs (pixel emission, pixel gloss, the G-buffer import, a host-located vct_trace)
and the read-backs (G-buffer, planes, outputs, chain, point queries, voxel view).

The method is that file's test_random_call_orders_give_what_a_synchronised_context_gives: the call list is built first, from
a seeded generator that carries a model of what is attached and what each slot holds (so that it issues only calls
include/vct.h allows, and reads only memory some call has written), then run twice -- as it stands, and with
vct_synchronize after every call -- and every read-back must be the same bytes.  Its sizes too: the atrium at 128^3,
1920 x 1080, because a 1080p trace is still running when the host issues the next call; at the frames of the feature files
the GPU is idle by then and no ordering can show.  Read-backs are held as BLAKE2b digests of their bytes (a 1080p G-buffer
is 190 MB), formed 16 MiB at a time on worker threads so that the host's next call is not held up behind them.

What the library's waits are worth, from scratch builds that lack exactly one wait each (never committed); this file alone
was run on each:
  * vct_set_pixel_emission without its vct_staging_free, and a build with none of the waits that vct_trace's host-linear
    hand-over, vct_download_gbuffer and the chain downloads now take: every test here passes.  Every user of c->gb_linear
    and of c->vol.staging waits for its own stream before it returns, so none of the other slot's work on a staging buffer
    is ever in flight when a call begins.  Those waits are a guarantee, not an observable.
  * vct_inject_light without its vct_pipeline_join, lights attached: test_level_0_rewritten_while_the_other_slot_traces
    fails (the random orders and the staging orders pass: vct_voxelize in front of it, on the same selection, has joined
    already -- the join shows only where the inject is the selection's first producer, which that test arranges).
  * vct_refresh_steps (behind vct_set_cone_apertures) without its vct_pipeline_drain, gloss classes attached:
    test_step_tables_rewritten_while_the_other_slot_traces fails.  (test_gpu_pipeline.py found this drain unobservable with
    the two tables of a context without classes; the class tables make the upload long enough to land in a running trace.)

The dynamic mesh (include/vct.h "dynamic mesh") came after this file: its layer, the two sets of statistics and the one
position buffer are shared by both slots.  Its four calls -- dyn_attach (two meshes to switch between: dyncases' object of
150 triangles and dyncases.crowd(), 200 k small ones, so that k_dyn_tris is still running when the host issues the next
call), dyn_update (host and device positions), dyn_detach, read_dynamic (vct_get_dynamic + vct_download_dynamic_voxels) --
are drawn only by CallList(dynamic=True): DYN_SEEDS; the lists of SEEDS are, draw for draw, what they were (PARENT_LISTS).
The model issues a bounce only detached and an update or a layer download only attached.  The directed orders at the end
of the file are, beyond the comparison of the two runs, held against the CPU oracle: every chain read back is
build_mips(merge(D, S)) for the mesh and positions resolved_states() says that pass used, every layer read back is D.
Scratch builds, this file alone on each:
  * vct_update_dynamic_positions without its vct_pipeline_join: every test passes.  The only readers of the position
    buffer are the kernels of vct_voxelize / vct_gi_pass, and those calls are producers: vct_select_frame_slot puts the
    stream selected next behind a producer (VctSlotOrder::produced), so the copy of an update issued on the other slot at
    once already follows the pass; and a voxelize issued after an update on the other slot joins that slot's stream
    itself.  The join in the update is a guarantee, not an observable.
  * the detaching vct_set_dynamic_mesh without its vct_synchronize: every test passes.  The layer's buffers are released
    with hipFree, which waits for the device itself.  A guarantee, not an observable -- it would become one the day the
    buffers come from a pool.

The dynamic mesh's three switches came after that: vct_set_dynamic_draw, vct_set_dynamic_emission, vct_set_dynamic_bounce.
The draw copy with its face frames (k_dyn_draw_prepare), the shadow map's second raster scratch, the emission table with
its sums and the bounce's brick table are shared by both slots.  CallList(features=True) -- it implies dynamic=True --
draws dyn_draw(flags), dyn_emission(table | none), dyn_bounce(on) mostly with the stage they switch behind them, and reads
back the shadow map (read_shadow) and the pixel-emission planes where the model says they exist: FEAT_SEEDS.  The model: a
bounce is issued attached only while the switch is on (else the mesh is detached first, as before); every
vct_set_dynamic_mesh -- attach, replace, detach -- drops the table and with it the planes no other owner holds; the table is
set on an attached mesh only.  A trace variant is refused while planes are attached: no list sets one.  SEEDS and DYN_SEEDS
generate, draw for draw, what they generated before (PARENT_LISTS holds both).  The directed order at the end of the file
(positions rewritten behind the other slot's draw) is held against the CPU checker's map and planes as well.
Times on an MI355X, one run of this file's dynamic tests: DYN_SEEDS 7 / 8 / 9 take 0.21 / 0.15 / 0.13 s, FEAT_SEEDS
11 / 27 / 42 take 0.17 / 0.27 / 0.24 s -- each within 1.5 times the slowest of the former (0.32 s), so the lists keep ROUNDS.
"""

import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import components_ref as cr
import dyncases as dc
import dynemiscases as de
import gloss_ref as gr
import lights_ref as lr
import sky_ref as sr
import vctpkg
from test_gpu_pipeline import cameras, lights as light_dirs, make

pytestmark = pytest.mark.gpu

W, H, V = 1920, 1080, 128
CAMS, LIGHT_DIRS, ROUNDS = 3, 4, 4
APERTURES = [(0.577, 0.07), (0.577, 0.2), (0.45, 0.105)]
MASKS = [cr.SHOW_ALL, cr.SHOW_ALL & ~cr.SHOW_DIFFUSE, cr.SHOW_DIFFUSE | cr.SHOW_INDIRECT_SPECULAR,
         cr.SHOW_INDIRECT_DIFFUSE | cr.SHOW_AMBIENT_OCCLUSION, cr.SHOW_DIFFUSE | cr.SHOW_SPECULAR]
ALL_AOV = cr.AOV_INDIRECT_DIFFUSE | cr.AOV_INDIRECT_SPECULAR | cr.AOV_DIRECT
# what the setters switch between: index 0 detaches
LIGHT_SETS = [None,
              [lr.point((-40.0, -5.0, 0.0), (400.0, 300.0, 200.0), 60.0, 2.0),
               lr.spot((-20.0, 10.0, 5.0), (900.0, 900.0, 500.0), 80.0, 1.5, (-1.0, -0.5, -0.3), 0.9, 0.3)],
              lr.LIGHTS]
SKIES = [None, sr.SH, np.ascontiguousarray(sr.SH[:, ::-1] * np.float32(0.5))]
GLOSS_TABLES = [None, list(gr.CLASSES[:3]), list(gr.CLASSES[1:3])]
NPOINTS = 64 * 40 + 37
SEEDS = [1, 2, 3, 4, 5, 6]
DYN_SEEDS = [7, 8, 9]               # call lists that also draw the dynamic mesh's calls
DYN_AT = [(0.0, 0.0, 200.0), (500.0, -300.0, 300.0), (-500.0, 200.0, -200.0)]      # where the moving object stands (model units)
DYN_MESHES = 2                      # 0: dyncases' object of 150 triangles, 1: dyncases.crowd(), 200 k small ones
FEAT_SEEDS = [11, 27, 42]           # call lists that also flip the dynamic mesh's draw, emission and bounce switches
DYN_TABLES = [None, de.EM, de.ONE]  # vct_set_dynamic_emission: index 0 detaches (both meshes have dyncases' three materials)
DYN_SPECULAR = (0.3, 0.6, 0.2)
# BLAKE2b-128 of repr(call_list(seed)) for SEEDS as the commit before the dynamic calls gave them: what those seeds run stays
PARENT_LISTS = {1: "7a660e04415f52dafde5dcadd80a686d", 2: "e2f07c84814d189d6ed765f376e623e9", 3: "04d01e65d68d5c8947e75e807342ae87",
                4: "12652795f3b626c8e5a8a69b0e248c50", 5: "0cd29f76f51ef54a9a66068164995224", 6: "8a095071283f9869ad42359f63b4fac5"}
# ... and of repr(call_list(seed, dynamic=True)) for DYN_SEEDS as the commit before the three switches gave them
PARENT_LISTS.update({7: "22af0922d6cd95de84bb62137342ee69", 8: "fd5b1d4b0744b8e89b20d5c4fe4dd197", 9: "5a959b8cee900def11044516f65dfa9d"})


@pytest.fixture(scope="module")
def vct():
    import torch
    assert torch.cuda.is_available()
    return vctpkg.load()


# ---- the call list ------------------------------------------------------------------------------------------------------
class CallList:
    """The calls of one run and the state they leave, as far as legality and defined read-backs need it."""

    def __init__(self, rng, dynamic=False, features=False):
        self.rng, self.ops, self.slot = rng, [], 0
        self.features = features            # draw the dynamic mesh's three switches too (off: SEEDS and DYN_SEEDS, draw for draw)
        self.dynamic = dynamic or features  # draw the dynamic mesh's calls too (off: the lists of SEEDS, draw for draw)
        self.dyn = None                     # the attached dynamic mesh (index), None: detached
        self.dyn_draw_flags = 0             # vct_set_dynamic_draw: context state, outlives the mesh
        self.dyn_bounce_on = False          # vct_set_dynamic_bounce: context state too
        self.dyn_emis = 0                   # index into DYN_TABLES, 0: none; vct_set_dynamic_mesh drops the table
        self.lights = self.sky = self.gloss = 0              # index into LIGHT_SETS / SKIES / GLOSS_TABLES
        self.matgloss = self.emission = self.bounced = False
        self.pending = False                # a voxelize pass waits for its inject_light
        self.rate = 1
        self.aov = 0
        self.deck = []
        self.gb = [False, False]            # the slot has a resident G-buffer
        self.frame = [False, False]         # some launch has written the slot's whole frame
        self.marched = [False, False]       # vct_last_step_count has something to report
        self.emis_user = [False, False]     # the caller's pixel-emission planes
        self.lit = [False, False]           # a composite launch with lights attached has filled the lit planes

    def pick(self, n):
        return int(self.rng.integers(n))

    def chance(self, p):
        return bool(self.rng.random() < p)

    def add(self, *op):
        self.ops.append(op)

    # -- producers and frames (the eight calls of test_gpu_pipeline.py)
    def switch(self, slot):
        self.add("switch", slot)
        self.slot = slot

    def produce(self):
        self.add("produce", self.pick(LIGHT_DIRS))
        self.bounced = self.pending = False

    def revoxelize(self):
        self.add("revoxelize")
        self.bounced = self.pending = False

    def voxelize(self):
        """The first half of a moved light on this selection; inject() on a later one is then the selection's first producer,
        and its join the only thing between the resolve and the other slot's trace."""
        self.add("voxelize", self.pick(LIGHT_DIRS))
        self.pending = True

    def inject(self):
        self.add("inject")
        self.bounced = self.pending = False

    def launched(self):
        s = self.slot
        self.gb[s] = self.frame[s] = self.marched[s] = True
        if self.lights:
            self.lit[s] = True

    def gi(self):
        self.add("gi", self.pick(LIGHT_DIRS), self.pick(CAMS))
        self.bounced = self.pending = False
        self.launched()

    def gbuffer(self):
        self.add("gbuffer", self.pick(CAMS))
        self.gb[self.slot] = True

    def trace(self):
        assert self.gb[self.slot]
        self.add("trace")
        self.launched()

    def remesh(self):
        self.add("remesh", self.pick(2))
        self.matgloss = self.emission = False        # a new mesh detaches both material tables
        self.produce()

    # -- the dynamic mesh: the layer, its statistics and its one position buffer are shared by both slots
    def dyn_attach(self, mesh=None):
        if mesh is None:
            mesh = self.pick(DYN_MESHES) if self.dyn is None else (self.dyn + 1) % DYN_MESHES
        self.dyn = mesh
        self.dyn_emis = 0                   # vct_set_dynamic_mesh drops the emission table (and the planes it attached)
        self.add("dyn_attach", mesh, self.pick(len(DYN_AT)))

    def dyn_update(self):
        assert self.dyn is not None         # refused with nothing attached
        self.add("dyn_update", self.pick(len(DYN_AT)), self.chance(0.5))      # position, device-located

    def dyn_detach(self):
        self.add("dyn_detach")
        self.dyn = None
        self.dyn_emis = 0

    # -- the three switches (CallList(features=True) only): the draw copy with its face frames, the shadow map's second
    #    raster scratch, the emission table with its sums and the bounce's brick table are shared by both slots
    def dyn_draw(self, flags=None):
        if flags is None:
            flags = (self.dyn_draw_flags + 1 + self.pick(3)) % 4
        self.dyn_draw_flags = flags
        self.add("dyn_draw", flags)

    def dyn_emission(self):
        assert self.dyn is not None         # refused with nothing attached
        self.dyn_emis = (self.dyn_emis + 1 + self.pick(2)) % 3
        self.add("dyn_emission", self.dyn_emis)

    def dyn_bounce(self, on):
        self.dyn_bounce_on = on
        self.add("dyn_bounce", on)

    def bounce(self):
        """vct_bounce: refused between voxelize and inject_light, and with a dynamic mesh attached unless the switch is on."""
        if self.pending:
            self.inject()
        if self.dyn is not None:
            if self.features and (self.dyn_bounce_on or self.chance(0.6)):
                if not self.dyn_bounce_on:
                    self.dyn_bounce(True)
            else:
                self.dyn_detach()
        self.add("bounce")
        self.bounced = True
        self.marched[self.slot] = True
        if self.chance(0.5):
            self.add("read_steps")

    def feat_op(self):
        """One of the three switches, at once behind whatever the other slot has in flight, mostly with the stage that reads
        it behind it and a read-back of what that stage wrote."""
        r = self.rng.random()
        if self.dyn is None:
            self.dyn_attach()
        if r < 0.4:
            self.dyn_draw()
            r = self.rng.random()
            if r < 0.35:
                self.gi()
            elif r < 0.85:
                if r < 0.6:
                    self.produce()          # the shadow map with (or without) the mover in it
                self.gbuffer()
                self.trace()
            else:
                return
            what = self.pick(4)
            if what == 0:
                self.add("read_shadow")
            elif what == 1:
                self.add("read_gbuffer")
            elif what == 2 and (self.emission or self.dyn_emis or self.emis_user[self.slot]):
                self.add("read_pixel_emission")
            else:
                self.read_frame()
        elif r < 0.75:
            self.dyn_emission()
            r = self.rng.random()
            if r < 0.4:
                self.revoxelize()
            elif r < 0.7:
                self.gi()
            if self.chance(0.5):
                self.read_dynamic()
            elif self.dyn_emis:
                self.add("read_pixel_emission")
        else:
            self.dyn_bounce(not self.dyn_bounce_on)
            if self.dyn_bounce_on and self.chance(0.7):
                self.bounce()
                self.add("read_chain")

    def read_dynamic(self):
        assert self.dyn is not None         # the download is refused with nothing attached
        self.add("read_dynamic")

    def dyn_op(self):
        """One of the dynamic calls, at once behind whatever the other slot has in flight; a new object or new positions
        mostly with a pass behind them, so that later frames and read-backs see them."""
        r = self.rng.random()
        if self.dyn is None or r < 0.2:
            self.dyn_attach()
        elif r < 0.65:
            self.dyn_update()
        elif r < 0.8:
            self.dyn_detach()
            if self.chance(0.5):
                self.revoxelize()
            return
        else:
            self.read_dynamic()
            return
        r = self.rng.random()
        if r < 0.4:
            self.revoxelize()
        elif r < 0.6:
            self.gi()
        if self.chance(0.4):
            self.read_dynamic()

    # -- hand-overs of a G-buffer other than the raster pass
    def trace_host(self):
        self.add("trace_host", self.pick(2))         # a read-back as well: vct_trace returns the frame
        self.launched()

    def import_gbuffer(self):
        self.add("import", self.pick(2), self.chance(0.5), self.chance(0.5))       # camera, device inputs, shadow + material ids
        self.gb[self.slot] = True

    def some_gbuffer(self):
        r = self.rng.random()
        if r < 0.5:
            self.gbuffer()
        elif r < 0.8:
            self.import_gbuffer()
        else:
            self.trace_host()
            return
        self.trace()

    # -- shared state, rewritten while the other slot's trace is in flight
    def setter(self, r=None):
        """One kind of shared state rewritten; the kinds come off a shuffled deck, so that a run of a few rounds sees many."""
        if r is None:
            if not self.deck:
                self.deck = [int(x) for x in self.rng.permutation(12)]
            r = self.deck.pop()
        if r == 0:
            self.lights = (self.lights + 1 + self.pick(2)) % 3
            self.add("lights", self.lights)
            if not self.lights:
                self.lit = [False, False]
            if self.chance(0.5):
                self.revoxelize()
            else:
                self.gi()
        elif r == 1:
            self.sky = (self.sky + 1 + self.pick(2)) % 3
            self.add("sky", self.sky)
        elif r == 2:
            self.gloss = (self.gloss + 1 + self.pick(2)) % 3
            self.add("gloss", self.gloss)
        elif r == 3:
            self.matgloss = not self.matgloss
            self.add("matgloss", self.matgloss)
        elif r == 4:
            self.emission = not self.emission
            self.add("emission", self.emission)
            self.revoxelize()
        elif r == 5:
            self.rate = 3 - self.rate
            self.add("rate", self.rate)
        elif r == 6:
            self.add("components", MASKS[self.pick(len(MASKS))])
        elif r == 7:
            sets = [0, ALL_AOV, cr.AOV_INDIRECT_SPECULAR, cr.AOV_DIRECT | cr.AOV_INDIRECT_DIFFUSE]
            self.aov = sets[(sets.index(self.aov) + 1 + self.pick(3)) % 4]
            self.add("aov", self.aov)
        elif r == 8:
            self.add("apertures", self.pick(len(APERTURES)))
        elif r == 9:
            self.bounce()
        elif r == 11:
            self.remesh()                  # buffers the other slot's kernels may still read are freed and re-allocated
        else:
            # footprint records are refused beside a sky, gloss classes and rate 2 (and those beside them): whatever bars
            # them goes first; then on, one frame, off
            if self.sky:
                self.sky = 0
                self.add("sky", 0)
            if self.gloss:
                self.gloss = 0
                self.add("gloss", 0)
            if self.rate == 2:
                self.rate = 1
                self.add("rate", 1)
            if self.bounced:
                self.revoxelize()
            if not self.gb[self.slot]:
                self.gbuffer()
            self.add("footprints", True)
            self.trace()
            self.read_frame()
            self.add("footprints", False)

    # -- the slot's own planes
    def planes(self):
        r = self.pick(2 if self.gloss else 1)
        form = ["host", "device", None][self.pick(3)]
        if r == 0:
            self.add("pixel_emission", form)
            self.emis_user[self.slot] = form is not None
        else:
            self.add("pixel_gloss", form)

    # -- read-backs: only what some call has written
    def read_frame(self):
        if self.frame[self.slot]:
            self.add("read_frame", self.marched[self.slot])      # (a voxel view writes a frame and marches no cone)
        else:
            self.reader()

    def reader(self):
        s = self.slot
        can = ["chain", "gather", "gather", "cone", "cone", "voxels"]
        if self.frame[s]:
            can.append("read_frame")
        if self.gb[s]:
            can.append("read_gbuffer")
        if self.emission or self.dyn_emis or self.emis_user[s]:
            can += ["read_pixel_emission"] * 3
        if self.gloss:
            can += ["read_pixel_gloss"] * 3
        if self.lights and self.lit[s]:
            can += ["read_pixel_lights"] * 3
        if self.aov:
            can += ["read_aov"] * 3
        if self.dyn is not None:
            can += ["read_dynamic"] * 2
        if self.features:
            can += ["read_shadow"] * 2      # the one shadow map of the context: every list begins with a pass that renders it
        what = can[self.pick(len(can))]
        if what == "gather":
            self.add("gather", self.chance(0.5), self.chance(0.5))                  # device-located, sorted
        elif what == "cone":
            nap = 2 + (len(GLOSS_TABLES[self.gloss]) if self.gloss else 0)
            self.add("cone", self.chance(0.5), self.chance(0.5), self.pick(nap))
        elif what == "voxels":
            self.add("voxels", self.pick(4), self.pick(CAMS))
            self.frame[s] = True
        elif what == "read_aov":
            for bit in (1, 2, 4):
                if self.aov & bit:
                    self.add("read_aov", bit)
        elif what == "chain":
            self.add("read_chain")
        elif what == "read_frame":
            self.read_frame()
        elif what == "read_dynamic":
            self.read_dynamic()
        else:
            self.add(what)


def call_list(seed, rounds=ROUNDS, dynamic=False, features=False):
    m = CallList(np.random.default_rng(seed), dynamic, features)
    m.add("produce", 0)
    for r in (0, 1, 2, 4, 7):               # most runs begin with something attached: lights, a sky, gloss classes, emission, outputs
        if m.chance(0.6):
            m.setter(r)
    if m.dynamic and m.chance(0.7):
        m.dyn_attach()
        m.revoxelize()
    if m.features:                          # most of these runs begin with the mover drawn
        if m.chance(0.7):
            m.dyn_draw(1 + m.pick(3))
        if m.dyn is not None and m.chance(0.5):
            m.dyn_emission()
    for _ in range(rounds):
        s0 = m.pick(2)
        m.switch(s0)
        # a frame on slot s0, with or without new shared state in front of it ...
        r = m.rng.random()
        if r < 0.15 and m.marched[s0]:
            m.produce()
        elif r < 0.3:
            m.gi()
        else:
            if r < 0.45:
                m.produce()
            elif r < 0.6:
                m.planes()
            m.some_gbuffer()
        if m.chance(0.4):
            m.voxelize()
        # ... and, while its trace is still running, the other slot at once: shared state rewritten, the slot's planes handed
        # over through the staging both slots share, or a read-back
        m.switch(1 - s0)
        if m.dynamic and m.chance(0.7):
            m.dyn_op()                     # the layer or the positions rewritten under the other slot's pass or frame
        if m.features and m.chance(0.8):
            m.feat_op()                    # a switch flipped, and the stage it switches, under the other slot's pass or frame
        m.setter()
        if m.chance(0.5):
            m.planes()
        m.reader()
        m.setter()
        if m.dynamic and m.chance(0.5):
            m.dyn_op()
        if m.features and m.chance(0.5):
            m.feat_op()
        if m.gb[m.slot] and m.chance(0.5):
            m.trace()                      # the resident G-buffer under the new state, at once
            m.reader()
        r = m.rng.random()
        if r < 0.3:
            m.produce()
        elif r < 0.45:
            m.gi()
        if m.chance(0.6):
            m.some_gbuffer()
        if m.chance(0.5):
            m.reader()
        m.switch(s0)
        if m.pending:
            m.inject()                     # level 0 rewritten at once, while the other slot's frame is in flight
        m.read_frame()
        m.reader()
    return m.ops


# ---- inputs, made once for both runs ------------------------------------------------------------------------------------
class Inputs:
    def __init__(self, vct, w, h, v):
        import torch
        from voxel_cone_tracing_amd import scene as sc
        self.torch, self.sc, self.w, self.h, self.v = torch, sc, w, h, v
        npix, tiles = w * h, ((w + 7) // 8) * ((h + 7) // 8)
        self.meshes = [sc.Scene(sc.ATRIUM, 0.15, 1234), sc.Scene(sc.ATRIUM, 0.2, 99)]
        self.cams = cameras(sc, w, h, CAMS)
        self.dirs = light_dirs(LIGHT_DIRS)
        r = np.random.default_rng(77)
        # two host-located linear G-buffers, from the raster pass of a context of its own
        ctx, _ = make(vct, w, h, V=v)
        ctx.render_shadow_map(sc.light_view_proj(self.dirs[0]))
        # the shadow map of light 0 as the oracle takes it: what the directed dynamic orders voxelize under
        self.shadow0 = ctx.download_shadow_map()
        self.lvp0 = np.ascontiguousarray(np.asarray(sc.light_view_proj(self.dirs[0]), np.float32).reshape(4, 4).T)
        self.host_gb = []
        for pos, vp in self.cams[:2]:
            ctx.set_camera_position(pos)
            ctx.render_gbuffer(vp)
            self.host_gb.append(ctx.download_gbuffer())
        ctx.close()
        # the same two as a renderer's buffers, in host memory and as device tensors
        self.imp_host, self.imp_dev, self.keep = [], [], []
        nmat = self.meshes[0].albedo.shape[0]
        for g in self.host_gb:
            spec = np.zeros((npix, 4), np.float32)
            spec[:, :3] = g[19:22].T
            d = dict(position=np.ascontiguousarray(g[0:3].T), normal=np.ascontiguousarray(g[3:6].T),
                     albedo=np.ascontiguousarray(g[15:19].T), specular=spec, shadow=np.ascontiguousarray(g[22]),
                     material=r.integers(0, nmat + 2, npix).astype(np.uint16))
            self.imp_host.append(d)
            t = {k: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda() for k, a in d.items()}
            self.keep.append(t)
            self.imp_dev.append({k: x.data_ptr() for k, x in t.items()})
        # planes of a slot: host linear and device tiled
        self.emis_host = r.uniform(0.0, 2.0, (3, npix)).astype(np.float32)
        self.emis_dev = torch.from_numpy(r.uniform(0.0, 2.0, (tiles, 3, 64)).astype(np.float32)).cuda()
        self.gloss_host = gr.checkerboard(w, h, 3, in_frame_extra=200)
        self.gloss_dev = torch.from_numpy(r.integers(0, 4, (tiles, 64)).astype(np.uint8)).cuda()
        # material tables, per mesh
        self.emission = [(r.uniform(0.0, 1.5, (m.albedo.shape[0], 3)) * (r.random((m.albedo.shape[0], 1)) < 0.5)).astype(np.float32)
                         for m in self.meshes]
        for e in self.emission:
            e[0] = (0.5, 0.25, 1.0)          # never an all-zero table: that would detach
        self.mat_class = [r.integers(0, 4, m.albedo.shape[0]).astype(np.uint8) for m in self.meshes]
        # query points: live pixels of the first G-buffer, in an order that is not spatial
        live = np.flatnonzero(self.host_gb[0][18] >= 0.5)
        idx = r.permutation(live)[:NPOINTS]
        self.gather_pts = np.ascontiguousarray(self.host_gb[0][0:12, idx].T, np.float32)
        dirs = r.normal(size=(idx.size, 3))
        self.cone_pts = np.ascontiguousarray(np.concatenate(
            [self.gather_pts[:, 0:6], dirs / np.linalg.norm(dirs, axis=1, keepdims=True)], axis=1), np.float32)
        n = idx.size
        self.npts = n
        self.d_gather, self.d_cone = torch.from_numpy(self.gather_pts).cuda(), torch.from_numpy(self.cone_pts).cuda()
        self.d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        self.d_cones = torch.zeros((n, 6, 4), dtype=torch.float32, device="cuda")
        self.d_steps = torch.zeros((n, 6), dtype=torch.uint8, device="cuda")
        # the dynamic meshes (material, albedo, positions at each of DYN_AT), and the positions as device tensors
        self.dyn = [(m[1], m[2], [dc.placed(m[0], at) for at in DYN_AT]) for m in ((dc.offsets(),) + dc.materials(), dc.crowd())]
        self.dyn_dev = [[torch.from_numpy(p).cuda() for p in m[2]] for m in self.dyn]
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def inputs(vct):
    return Inputs(vct, W, H, V)


# ---- one run ------------------------------------------------------------------------------------------------------------
CHUNK = 16 << 20


def digest(chunk):
    return hashlib.blake2b(chunk, digest_size=16).digest()


def digests(pool, a):
    """One BLAKE2b digest per 16 MiB of the array's bytes, formed on the pool's threads (hashlib releases the GIL)."""
    b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return [(a.shape, str(a.dtype))] + [pool.submit(digest, b[i:i + CHUNK]) for i in range(0, max(b.size, 1), CHUNK)]


def run(vct, inp, ops, sync):
    """The calls of `ops` on a two-slot context; [(call index, call, digests and values of what it returned)]."""
    sc = inp.sc
    c, _ = make(vct, inp.w, inp.h, V=inp.v, voxel_attributes=1)
    c.set_frames_in_flight(2)
    mesh = 0
    dyn = None
    records = []
    pool = ThreadPoolExecutor(max_workers=8)

    def record(k, op, *values):
        records.append((k, op, [digests(pool, x) if isinstance(x, np.ndarray) else x for x in values]))

    try:
        for k, op in enumerate(ops):
            name = op[0]
            if name == "produce":
                c.set_light_direction(inp.dirs[op[1]])
                c.render_shadow_map(sc.light_view_proj(inp.dirs[op[1]]))
                c.voxelize(); c.inject_light(); c.build_mips()
            elif name == "revoxelize":
                c.voxelize(); c.inject_light(); c.build_mips()
            elif name == "voxelize":
                c.set_light_direction(inp.dirs[op[1]])
                c.render_shadow_map(sc.light_view_proj(inp.dirs[op[1]]))
                c.voxelize()
            elif name == "inject":
                c.inject_light(); c.build_mips()
            elif name == "shadow":
                c.set_light_direction(inp.dirs[op[1]])
                c.render_shadow_map(sc.light_view_proj(inp.dirs[op[1]]))
            elif name == "gi":
                c.set_light_direction(inp.dirs[op[1]]); c.set_camera_position(inp.cams[op[2]][0])
                c.gi_pass(sc.light_view_proj(inp.dirs[op[1]]), inp.cams[op[2]][1])
            elif name == "gbuffer":
                c.set_camera_position(inp.cams[op[1]][0]); c.render_gbuffer(inp.cams[op[1]][1])
            elif name == "trace":
                c.trace_resident()
            elif name == "switch":
                c.select_frame_slot(op[1])
            elif name == "remesh":
                mesh = op[1]
                m = inp.meshes[mesh]
                c.upload_triangles(m.pos, m.material, m.albedo)
                c.upload_mesh_attributes(*m.frames(), m.specular)
            elif name == "apertures":
                c.set_cone_apertures(*APERTURES[op[1]])
            elif name == "trace_host":
                c.set_camera_position(inp.cams[op[1]][0])
                record(k, op, c.trace(inp.host_gb[op[1]]), c.last_step_count())
            elif name == "import":
                cam, device, extras = op[1:]
                src = inp.imp_dev[cam] if device else inp.imp_host[cam]
                kw = dict(shadow=src["shadow"], material=src["material"]) if extras else {}
                if device:
                    kw.update(position_format=vct.IMPORT_POSITION_F32X3, normal_format=vct.IMPORT_NORMAL_F32X3,
                              albedo_format=vct.IMPORT_COLOR_F32X4, specular_format=vct.IMPORT_COLOR_F32X4)
                c.set_camera_position(inp.cams[cam][0])
                c.import_gbuffer(src["position"], src["normal"], src["albedo"], specular=src["specular"], **kw)
            elif name == "lights":
                c.set_lights(LIGHT_SETS[op[1]])
            elif name == "sky":
                c.set_sky(SKIES[op[1]])
            elif name == "gloss":
                c.set_gloss_classes(GLOSS_TABLES[op[1]])
            elif name == "matgloss":
                c.upload_material_gloss(inp.mat_class[mesh] if op[1] else None)
            elif name == "emission":
                c.upload_emission(inp.emission[mesh] if op[1] else None)
            elif name == "rate":
                c.set_diffuse_rate(op[1])
            elif name == "components":
                c.set_lighting_components(op[1])
            elif name == "aov":
                c.set_aov_outputs(op[1])
            elif name == "footprints":
                c.set_footprint_records(op[1])
            elif name == "bounce":
                c.bounce()
            elif name == "pixel_emission":
                if op[1] == "device":
                    c.set_pixel_emission(inp.emis_dev.data_ptr(), layout=vct.GB_TILED)
                else:
                    c.set_pixel_emission(inp.emis_host if op[1] else None)
            elif name == "pixel_gloss":
                if op[1] == "device":
                    c.set_pixel_gloss(inp.gloss_dev.data_ptr(), layout=vct.GB_TILED)
                else:
                    c.set_pixel_gloss(inp.gloss_host if op[1] else None)
            elif name == "read_frame":
                record(k, op, c.download_frame(), c.last_step_count() if len(op) < 2 or op[1] else None)
            elif name == "read_steps":
                record(k, op, c.last_step_count())
            elif name == "read_gbuffer":
                record(k, op, c.download_gbuffer())
            elif name == "read_pixel_emission":
                record(k, op, c.download_pixel_emission())
            elif name == "read_pixel_gloss":
                record(k, op, c.download_pixel_gloss())
            elif name == "read_pixel_lights":
                record(k, op, c.download_pixel_lights())
            elif name == "read_aov":
                record(k, op, c.download_aov(op[1]))
            elif name == "read_chain":
                record(k, op, c.download_chain())
            elif name == "gather":
                device, sort = op[1:]
                if device:
                    c.gather_points(inp.d_gather.data_ptr(), n=inp.npts, out_device_ptr=inp.d_out.data_ptr(),
                                    cones_device_ptr=inp.d_cones.data_ptr(), steps_device_ptr=inp.d_steps.data_ptr(), sort=sort)
                    last = c.last_point_query()             # waits for the slot's stream, and for nothing else
                    got = [t.cpu().numpy() for t in (inp.d_out, inp.d_cones, inp.d_steps)]
                else:
                    got = list(c.gather_points(inp.gather_pts, want_cones=True, want_steps=True, sort=sort))
                    last = c.last_point_query()
                record(k, op, *got, last)
            elif name == "cone":
                device, sort, ap = op[1:]
                if device:
                    c.cone_points(inp.d_cone.data_ptr(), ap, n=inp.npts, out_device_ptr=inp.d_out.data_ptr(),
                                  steps_device_ptr=inp.d_steps.data_ptr(), sort=sort)
                    last = c.last_point_query()
                    got = [inp.d_out.cpu().numpy(), inp.d_steps.cpu().numpy().reshape(-1)[:inp.npts]]
                else:
                    got = list(c.cone_points(inp.cone_pts, ap, want_steps=True, sort=sort))
                    last = c.last_point_query()
                record(k, op, *got, last)
            elif name == "voxels":
                level = 0 if op[1] >= vct.VOXVIEW_ALBEDO else 1
                c.render_voxels(sc.invert_matrix(inp.cams[op[2]][1]), op[1], level)
                record(k, op, c.download_frame())
            elif name == "dyn_attach":
                dyn = op[1]
                mat, alb, at = inp.dyn[dyn]
                c.set_dynamic_mesh(at[op[2]], mat, alb)
            elif name == "dyn_update":
                c.update_dynamic_positions(inp.dyn_dev[dyn][op[1]].data_ptr() if op[2] else inp.dyn[dyn][2][op[1]])
            elif name == "dyn_detach":
                dyn = None
                c.set_dynamic_mesh(None)
            elif name == "read_dynamic":
                record(k, op, c.dynamic_info(), *c.download_dynamic_voxels())
            elif name == "dyn_draw":
                c.set_dynamic_draw(op[1], DYN_SPECULAR)
            elif name == "dyn_emission":
                c.set_dynamic_emission(DYN_TABLES[op[1]])
            elif name == "dyn_bounce":
                c.set_dynamic_bounce(op[1])
            elif name == "read_shadow":
                record(k, op, c.download_shadow_map())
            else:
                raise AssertionError(op)
            if sync:
                c.synchronize()
        c.synchronize()
    finally:
        c.close()
    def settled(v):
        return [x.result() if hasattr(x, "result") else x for x in v] if isinstance(v, list) else v
    out = [(k, op, [settled(v) for v in values]) for k, op, values in records]
    pool.shutdown()
    return out


def assert_same(got, want, ops, what):
    assert len(got) == len(want), what
    for (k, op, a), (_, _, b) in zip(got, want):
        assert a == b, f"{what}: call {k} {op} returned something else without the waits; the calls before it: {ops[max(0, k - 12):k]}"


# ---- the tests ----------------------------------------------------------------------------------------------------------
def test_the_call_lists_reach_every_call():
    """Not a GPU matter, but the generator is this module's: over the seeds below every kind of call is issued."""
    seen = {op[0] for seed in SEEDS for op in call_list(seed)}
    assert seen >= {"produce", "revoxelize", "voxelize", "inject", "gi", "gbuffer", "trace", "switch", "apertures", "trace_host",
                    "import", "lights",
                    "sky", "gloss", "matgloss", "emission", "rate", "components", "aov", "bounce", "pixel_emission",
                    "pixel_gloss", "read_frame", "read_gbuffer", "read_pixel_emission", "read_pixel_gloss", "read_pixel_lights",
                    "read_aov", "read_chain", "gather", "cone", "voxels", "footprints", "remesh"}, sorted(seen)
    assert not seen & {"dyn_attach", "dyn_update", "dyn_detach", "read_dynamic"}
    for seed in DYN_SEEDS:                  # each of the lists with the dynamic mesh issues all four of its calls
        ops = call_list(seed, dynamic=True)
        assert {op[0] for op in ops} >= {"dyn_attach", "dyn_update", "dyn_detach", "read_dynamic", "bounce"}, seed
        attached = False
        for op in ops:                      # ... a bounce only detached, an update and a layer download only attached
            attached = op[0] == "dyn_attach" or (attached and op[0] != "dyn_detach")
            assert not (op[0] == "bounce" and attached) and not (op[0] in ("dyn_update", "read_dynamic") and not attached), (seed, op)
    for seed in FEAT_SEEDS:                 # ... and each of the lists with the switches the three setters and the map read-back
        assert {op[0] for op in call_list(seed, features=True)} >= FEATURE_CALLS, seed


def test_the_call_lists_of_the_earlier_seeds_are_what_they_were():
    """The dynamic draws sit behind CallList's flag: without it the generator draws what it drew before they existed."""
    for seed in SEEDS:
        assert hashlib.blake2b(repr(call_list(seed)).encode(), digest_size=16).hexdigest() == PARENT_LISTS[seed], seed
        assert call_list(seed, dynamic=True) != call_list(seed)


def test_the_call_lists_with_the_dynamic_mesh_are_what_they_were():
    """The three switches sit behind CallList(features=True): without it DYN_SEEDS draw what they drew before."""
    for seed in DYN_SEEDS:
        ops = call_list(seed, dynamic=True)
        assert hashlib.blake2b(repr(ops).encode(), digest_size=16).hexdigest() == PARENT_LISTS[seed], seed
        assert call_list(seed, features=True) != ops
        assert not {op[0] for op in ops} & FEATURE_CALLS


FEATURE_CALLS = {"dyn_draw", "dyn_emission", "dyn_bounce", "read_shadow"}


def test_the_call_lists_with_the_switches_reach_every_new_call_within_the_rules():
    """Each list of FEAT_SEEDS issues the three setters, the four calls of the dynamic mesh, a bounce with the mesh attached,
    G-buffer passes that draw the mover and read-backs of the shadow map and of planes the dynamic table attached; and the
    model holds: a bounce attached only with the switch on, the table only on an attached mesh and gone with every
    vct_set_dynamic_mesh, pixel emission read only where planes exist.  (No list sets a trace variant: the planes a table
    attaches would refuse it.)"""
    for seed in FEAT_SEEDS:
        ops = call_list(seed, features=True)
        names = {op[0] for op in ops}
        assert names >= FEATURE_CALLS | {"dyn_attach", "dyn_update", "dyn_detach", "read_dynamic", "bounce", "read_pixel_emission"}, (seed, sorted(names))
        assert "variant" not in names
        attached = switch = pending = False
        table = static_table = flags = slot = 0
        user = [False, False]
        bounces = drawn = table_reads = 0
        for op in ops:
            name = op[0]
            if name == "switch":
                slot = op[1]
            elif name in ("dyn_attach", "dyn_detach"):
                attached, table = name == "dyn_attach", 0
            elif name == "dyn_bounce":
                switch = op[1]
            elif name == "dyn_draw":
                flags = op[1]
                assert 0 <= flags <= 3
            elif name == "dyn_emission":
                assert attached, (seed, op)
                table = op[1]
            elif name == "emission":
                static_table = op[1]
            elif name == "remesh":
                static_table = False
            elif name == "pixel_emission":
                user[slot] = op[1] is not None
            elif name == "voxelize":
                pending = True
            elif name in ("inject", "produce", "revoxelize", "gi"):
                pending = False
            elif name == "bounce":
                assert not pending and (switch or not attached), (seed, op)
                bounces += attached
            elif name in ("dyn_update", "read_dynamic"):
                assert attached, (seed, op)
            elif name == "read_pixel_emission":
                assert table or static_table or user[slot], (seed, op)
                table_reads += bool(table) and not static_table and not user[slot]
            if name in ("gbuffer", "gi") and attached and flags & 2:
                drawn += 1
        assert bounces >= 1 and drawn >= 3 and table_reads >= 1, (seed, bounces, drawn, table_reads)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_call_orders_give_what_a_synchronised_context_gives(vct, inputs, seed):
    ops = call_list(seed)
    got, want = run(vct, inputs, ops, False), run(vct, inputs, ops, True)
    assert len(want) >= 2 * ROUNDS
    assert_same(got, want, ops, f"seed {seed}")


@pytest.mark.parametrize("seed", DYN_SEEDS)
def test_random_call_orders_with_the_dynamic_mesh(vct, inputs, seed):
    ops = call_list(seed, dynamic=True)
    got, want = run(vct, inputs, ops, False), run(vct, inputs, ops, True)
    assert len(want) >= 2 * ROUNDS
    assert_same(got, want, ops, f"seed {seed}, dynamic mesh")


@pytest.mark.parametrize("seed", FEAT_SEEDS)
def test_random_call_orders_with_the_dynamic_switches(vct, inputs, seed):
    ops = call_list(seed, features=True)
    got, want = run(vct, inputs, ops, False), run(vct, inputs, ops, True)
    assert len(want) >= 2 * ROUNDS
    assert_same(got, want, ops, f"seed {seed}, dynamic mesh with its switches")


# (writer on slot 0, what its effect is read back with): each leaves work on slot 0's stream or has just used the staging
WRITERS = {
    "trace_host": ([("trace_host", 0)], "read_frame"),
    "pixel_emission": ([("pixel_emission", "host"), ("trace",)], "read_frame"),
    "pixel_gloss": ([("pixel_gloss", "host"), ("trace",)], "read_frame"),
    "read_gbuffer": ([("trace",), ("read_gbuffer",)], "read_gbuffer"),
    "read_pixel_emission": ([("trace",), ("read_pixel_emission",)], "read_pixel_emission"),
    "read_pixel_lights": ([("trace",), ("read_pixel_lights",)], "read_pixel_lights"),
}
# what slot 1 does at once; the three downloads start with an untile kernel that writes the staging from the GPU, with no
# host copy in front of it
USERS = {
    "trace_host": [("trace_host", 1)],
    "pixel_emission": [("pixel_emission", "host")],
    "pixel_gloss": [("pixel_gloss", "host")],
    "read_gbuffer": [("read_gbuffer",)],
    "read_pixel_emission": [("read_pixel_emission",)],
    "read_pixel_lights": [("read_pixel_lights",)],
}


@pytest.mark.parametrize("writer", list(WRITERS))
def test_directed_orders_on_the_shared_staging(vct, inputs, writer):
    """For every pair (writer on slot 0, user on slot 1): slot 0's call, the switch, slot 1's call, with nothing in between;
    then slot 0's frame or plane, and slot 1's frame.  Against the same calls with a vct_synchronize between them.  (One
    pair of contexts per writer, the six users one after the other: a 1080p context costs more than the calls.)"""
    first, back = WRITERS[writer]
    ops = [("produce", 0), ("lights", 1), ("gloss", 1), ("revoxelize",)]
    for slot in (0, 1):                      # both slots: a G-buffer, planes of their own, a first frame (lit planes)
        ops += [("switch", slot), ("gbuffer", slot), ("pixel_emission", "device"), ("trace",)]
    for user in USERS:
        ops += [("switch", 0)] + first + [("switch", 1)] + USERS[user] + [("switch", 0), (back,), ("switch", 1), ("read_frame",)]
    got, want = run(vct, inputs, ops, False), run(vct, inputs, ops, True)
    assert_same(got, want, ops, f"{writer} on slot 0")


def two_frames():
    """Both slots with lights and gloss classes attached, a G-buffer and a first frame each."""
    ops = [("produce", 0), ("lights", 1), ("gloss", 1), ("revoxelize",)]
    for slot in (0, 1):
        ops += [("switch", slot), ("gbuffer", slot), ("pixel_gloss", "host"), ("trace",)]
    return ops


def test_level_0_rewritten_while_the_other_slot_traces(vct, inputs):
    """With lights attached: slot 0 voxelizes under a moved light, slot 1 queues frames, slot 0 injects at once -- the
    selection's first producer, so vct_inject_light's own join is all that keeps the resolve and the lights' voxel kernel
    behind slot 1's traces."""
    ops = two_frames()
    for k in (1, 2, 3):
        ops += [("switch", 0), ("voxelize", k), ("switch", 1), ("trace",), ("trace",), ("trace",), ("switch", 0), ("inject",),
                ("switch", 1), ("read_frame",), ("trace",), ("read_frame",), ("switch", 0), ("trace",), ("read_frame",)]
    got, want = run(vct, inputs, ops, False), run(vct, inputs, ops, True)
    assert_same(got, want, ops, "voxelize, the other slot's traces, inject")


def test_step_tables_rewritten_while_the_other_slot_traces(vct, inputs):
    """With gloss classes attached: new apertures and a trace at once on slot 1 while slot 0's frames are in flight -- the
    drain of vct_refresh_steps keeps the upload of the tables behind them."""
    ops = two_frames()
    for k in (1, 2, 0):
        ops += [("switch", 0), ("trace",), ("trace",), ("trace",), ("switch", 1), ("apertures", k), ("trace",),
                ("switch", 0), ("read_frame",), ("switch", 1), ("read_frame",)]
    got, want = run(vct, inputs, ops, False), run(vct, inputs, ops, True)
    assert_same(got, want, ops, "traces, new apertures on the other slot")


def test_step_count_of_a_bounce_while_the_other_slot_bounces(vct, inputs):
    """vct_last_step_count after a bounce reads the context's one bank of counters, which the other slot's bounce rewrites."""
    ops = [("produce", 0), ("bounce",), ("switch", 1), ("bounce",), ("switch", 0), ("read_steps",), ("switch", 1), ("read_steps",)]
    got, want = run(vct, inputs, ops, False), run(vct, inputs, ops, True)
    assert_same(got, want, ops, "bounce, bounce")


# ---- the dynamic mesh: directed orders, held against the oracle as well ---------------------------------------------------
def resolved_states(ops):
    """The model of a directed list (light 0 throughout; no lights, emission or bounce): call index -> what a read_chain
    there holds -- None for the static chain, (mesh, position) for merge(D, S) of the layer the last resolved pass voxelized --
    and what a read_dynamic there downloads -- the same, None for an empty layer.  A pass uses the positions of the last
    dyn_update issued before its voxelize; a layer replaced or detached between voxelize and inject has no pass to resolve."""
    mesh = at = pending = level0 = layer0 = None
    layer, out = 0, {}
    for k, op in enumerate(ops):
        name = op[0]
        if name == "dyn_attach":
            mesh, at, layer, layer0 = op[1], op[2], layer + 1, None
        elif name == "dyn_update":
            at = op[1]
        elif name == "dyn_detach":
            mesh, layer, layer0 = None, layer + 1, None
        elif name in ("produce", "revoxelize", "voxelize", "gi", "inject"):
            if name != "inject":
                assert name == "revoxelize" or op[1] == 0, op
                pending = (layer, None if mesh is None else (mesh, at))
            if name != "voxelize":
                level0 = pending[1] if pending[0] == layer else None
                if pending[0] == layer:
                    layer0 = level0
                pending = None
        elif name == "read_chain":
            out[k] = level0
        elif name == "read_dynamic":
            out[k] = layer0
        else:
            assert name in ("switch", "gbuffer", "trace", "read_frame"), op
    return out


_EXPECTED = {}


def expected(oracle, inp, state):
    """(digests of the chain, digests of the dynamic layer, level 0, the layer) the oracle gives for `state`."""
    def layer(pos, mat, alb):
        return dc.layer_plain(oracle, pos, mat, alb, V=inp.v, depth=inp.shadow0, vp=inp.lvp0)

    def settled(a):
        with ThreadPoolExecutor(max_workers=1) as pool:
            return [x.result() if hasattr(x, "result") else x for x in digests(pool, a)]
    if state not in _EXPECTED:
        m = inp.meshes[0]
        S = _EXPECTED[None][2] if state is not None else layer(m.pos, m.material, m.albedo)
        D = np.zeros_like(S)
        if state is not None:
            mat, alb, at = inp.dyn[state[0]]
            D = layer(at[state[1]], mat, alb)
            dc.assert_non_degenerate(D, S)
        l0 = dc.merge(D, S)
        _EXPECTED[state] = (settled(oracle.build_mips(l0)), settled(D), l0, D)
    return _EXPECTED[state]


def directed_dynamic(vct, oracle, inp, ops, what, states_wanted):
    """ops as they stand against ops with a vct_synchronize after every call, and every chain and layer read back against
    the oracle for the state the model gives; states_wanted: how many different states the chains read back must show."""
    states = resolved_states(ops)
    expected(oracle, inp, None)
    chains = {st: expected(oracle, inp, st)[0] for k, st in states.items() if ops[k][0] == "read_chain"}
    assert len(chains) >= states_wanted and len({repr(v) for v in chains.values()}) == len(chains), sorted(chains, key=repr)
    got, want = run(vct, inp, ops, False), run(vct, inp, ops, True)
    assert_same(got, want, ops, what)
    for k, op, values in want:
        if op[0] == "read_chain":
            assert values[0] == expected(oracle, inp, states[k])[0], f"{what}: call {k}: the chain is not that of {states[k]}"
        elif op[0] == "read_dynamic":
            assert values[1] == expected(oracle, inp, states[k])[1], f"{what}: call {k}: the layer is not that of {states[k]}"
            info = values[0]
            want_bricks = int(dc.bricks(expected(oracle, inp, states[k])[3][..., 3] > 0).sum())
            assert (info["bricks_used"], info["left_out"], info["skipped"]) == (want_bricks, 0, 0), (k, info)


def dynamic_frames(mesh=1):
    """The atrium under light 0, the dynamic mesh attached at position 0, a G-buffer and a first frame on both slots."""
    ops = [("produce", 0), ("dyn_attach", mesh, 0), ("revoxelize",)]
    for slot in (0, 1):
        ops += [("switch", slot), ("gbuffer", slot), ("trace",)]
    return ops


@pytest.mark.parametrize("device", [False, True])
def test_positions_rewritten_while_the_other_slot_voxelizes(vct, oracle, inputs, device):
    """Slot 0 voxelizes the crowd (shadow map, static pass, k_dyn_tris over 200 k triangles); slot 1 at once issues
    vct_update_dynamic_positions -- the one position buffer both slots share; slot 0 injects, builds the mips and reads the
    chain: that of the positions the voxelize was issued under.  Then a whole pass: the new ones."""
    ops = dynamic_frames()
    for at in (1, 2, 0):
        ops += [("switch", 0), ("voxelize", 0), ("switch", 1), ("dyn_update", at, device), ("switch", 0), ("inject",), ("read_chain",),
                ("read_dynamic",), ("revoxelize",), ("read_chain",)]
    directed_dynamic(vct, oracle, inputs, ops, f"voxelize, positions on the other slot (device={device})", 3)


def test_positions_and_a_pass_while_the_other_slot_traces(vct, oracle, inputs):
    """Slot 0 queues three frames; slot 1 at once moves the object, runs a pass and reads chain and layer; slot 0's frame is
    the one traced through the chain before the move."""
    ops = dynamic_frames()
    for at in (1, 2, 0):
        ops += [("switch", 0), ("trace",), ("trace",), ("trace",), ("switch", 1), ("dyn_update", at, at == 2), ("revoxelize",),
                ("read_chain",), ("read_dynamic",), ("switch", 0), ("read_frame",), ("switch", 1), ("trace",), ("read_frame",)]
    directed_dynamic(vct, oracle, inputs, ops, "traces, a move and a pass on the other slot", 3)


def test_layer_replaced_or_detached_while_the_other_slot_s_pass_is_in_flight(vct, oracle, inputs):
    """A pass in flight on slot 0 (its kernels write the layer's accumulators, table and pools); slot 1 at once detaches, or
    attaches the other mesh -- both free the layer -- and runs a pass of its own.  And the same with slot 0's pass only half
    issued: the inject behind the change resolves the static chain."""
    ops = dynamic_frames()
    for change in (("dyn_detach",), ("dyn_attach", 0, 1), ("dyn_attach", 1, 2), ("dyn_detach",), ("dyn_attach", 1, 1)):
        ops += [("switch", 0), ("revoxelize",), ("trace",), ("switch", 1), change, ("revoxelize",), ("read_chain",), ("switch", 0),
                ("read_chain",), ("read_frame",)]
    for change in (("dyn_attach", 0, 2), ("dyn_detach",), ("dyn_attach", 1, 0)):
        ops += [("switch", 0), ("voxelize", 0), ("switch", 1), change, ("switch", 0), ("inject",), ("read_chain",), ("revoxelize",),
                ("read_chain",)]
    directed_dynamic(vct, oracle, inputs, ops, "a pass, the layer replaced on the other slot", 5)


def test_layer_read_back_behind_the_other_slot_s_inject(vct, oracle, inputs):
    """vct_get_dynamic and vct_download_dynamic_voxels from slot 1 directly behind slot 0's vct_inject_light: statistics and
    pools are written by the merge on slot 0's stream."""
    ops = dynamic_frames()
    for at in (1, 2, 0, 1):
        ops += [("switch", 0), ("dyn_update", at, at == 1), ("voxelize", 0), ("inject",), ("switch", 1), ("read_dynamic",), ("read_chain",)]
    directed_dynamic(vct, oracle, inputs, ops, "inject, the layer read on the other slot", 3)


# ---- the drawn dynamic mesh: a directed order, held against the CPU checker as well --------------------------------------------
def test_positions_rewritten_behind_the_other_slot_s_draw(vct, oracle, inputs):
    """Slot 0 renders the shadow map and the G-buffer with both draw flags on (k_dyn_draw_prepare copies the crowd's 200 k
    triangles and forms their face frames; both raster passes read the copy); slot 1 at once issues
    vct_update_dynamic_positions.  Slot 0's map and planes are those of the position they were drawn at; slot 1's next draw
    shows the new one.  Both against the CPU checker's map and planes of the atrium followed by the crowd."""
    import dyndrawcases as ddc
    inp, sc = inputs, inputs.sc
    m = inp.meshes[0]
    static = (m.pos, m.material, m.albedo, m.specular, tuple(m.frames()))
    static_mesh = ddc.mesh_of(oracle, static, 0.05)
    mat, alb, at = inp.dyn[1]
    lvp, vp = sc.light_view_proj(inp.dirs[0]), inp.cams[0][1]
    want = {}

    def settled(a):
        with ThreadPoolExecutor(max_workers=4) as pool:
            return [x.result() if hasattr(x, "result") else x for x in digests(pool, a)][1:]
    depth_static = oracle.render_shadow_map(static_mesh, lvp, 512)
    for k in range(len(DYN_AT)):
        cat = ddc.concatenated(static, (at[k], mat, alb), specular=DYN_SPECULAR, ms=0.05, grid=150.0)
        depth, planes = ddc.reference(oracle, cat, inp.w, inp.h, vp, lvp, S=512, ms=0.05)
        shown = oracle.render_gbuffer(static_mesh, vp, inp.w, inp.h, depth, lvp)
        assert (planes.view(np.uint32) != shown.view(np.uint32)).any(0).sum() >= 100_000, k      # the crowd fills much of the frame
        assert (depth.view(np.uint32) != depth_static.view(np.uint32)).sum() >= 10_000, k
        want[k] = (settled(depth), settled(planes))
    assert len({repr(v) for v in want.values()}) == len(DYN_AT)
    ops = [("produce", 0), ("dyn_attach", 1, 0), ("dyn_draw", 3), ("revoxelize",)]
    for slot in (0, 1):
        ops += [("switch", slot), ("gbuffer", 0), ("trace",)]
    drawn_at, expect = 0, {}
    for new, device in ((1, False), (2, True), (0, False), (2, True)):
        ops += [("switch", 0), ("shadow", 0), ("gbuffer", 0), ("switch", 1), ("dyn_update", new, device), ("switch", 0)]
        expect[len(ops)], expect[len(ops) + 1] = (0, drawn_at), (1, drawn_at)
        ops += [("read_shadow",), ("read_gbuffer",), ("switch", 1), ("shadow", 0), ("gbuffer", 0)]
        expect[len(ops)], expect[len(ops) + 1] = (0, new), (1, new)
        ops += [("read_shadow",), ("read_gbuffer",)]
        drawn_at = new
    got, synced = run(vct, inp, ops, False), run(vct, inp, ops, True)
    assert_same(got, synced, ops, "a draw, new positions on the other slot")
    assert sorted(k for k, _, _ in synced) == sorted(expect)
    for k, op, values in synced:
        which, position = expect[k]
        assert values[0][1:] == want[position][which], f"call {k} {op}: not the {('map', 'planes')[which]} of position {position}"
