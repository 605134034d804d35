"""The expected frame of a screen trace with any set of the newer features attached, stacked from the reference modules of the
features themselves: gloss_ref (per-class oracle runs, selected per pixel), sky_ref (the sky added to each run's cones),
diffuse_rate_ref (the half-rate restatement of the result), components_ref (mask, skipped cone groups, per-component
outputs), lights_ref (the lit planes) and emission_ref (the composite's last add).  No arithmetic of its own: every number
here comes out of one of those modules or of the oracle.  tests/test_frame_ref_restatement.py holds it, with one feature
on, to that feature's module bit for bit.  Test infrastructure: NumPy + the oracle, no GPU.

The order is the composite's: cones (class, then sky), gather (rate), (A + D) + S under the mask, + (E + Lit)."""
import numpy as np

import components_ref as cr
import diffuse_rate_ref as drr
import emission_ref as er
import gloss_ref as gr
import lights_ref as lr
import sky_ref as sr

f32 = np.float32


def attached(classes=None, gloss_plane=None, sky=None, emission=None, lights=None, rate=1, mask=cr.SHOW_ALL, aov=0, rows=None,
             row_stride=1):
    """What is attached to the context when the trace is launched.  classes: [(tan_specular, shininess), ...] with
    gloss_plane uint8 [npix]; sky: float32 [9, 3]; emission: the slot's pixel-emission planes float32 [3, npix]; lights:
    what set_lights took; rate: 1 or 2; mask: SHOW_* bits; aov: AOV_* bits; rows = (tile_row0, tile_row1): the launch covers
    every row_stride-th tile row of that range (None: the whole frame)."""
    assert (classes is None) == (gloss_plane is None) and rate in (1, 2)
    return dict(classes=None if classes is None else [tuple(c) for c in classes], gloss_plane=gloss_plane, sky=sky,
                emission=emission, lights=lights, rate=rate, mask=mask, aov=aov,
                rows=None if rows is None else list(range(rows[0], rows[1], row_stride)),
                row_span=None if rows is None else (rows[0], rows[1], row_stride))


def _class_run(oracle, p, chain, planes, what, cache, nthreads):
    """One oracle parameter set's trace under the mask, with the sky when there is one: dict(rgba32f, rgba16f, steps, cones)."""
    key = bytes(p)
    c = cache.setdefault(key, {})
    sky, mask, aov = what["sky"], what["mask"], what["aov"]
    if sky is not None:
        if "sky" not in c:
            c["sky"] = sr.oracle_runs(oracle, p, chain, planes, nthreads)
            c.setdefault("plain", c["sky"][0])
        return sr.from_runs(oracle, p, planes, c["sky"], sky, mask, aov)
    if "plain" not in c:
        c["plain"] = oracle.trace(p, chain, planes, nthreads=nthreads, want_cones=True)
    ref = c["plain"]
    if mask == cr.SHOW_ALL:                  # both groups marched, the unmasked arithmetic: the oracle's own frame
        return dict(rgba32f=ref["rgba32f"], rgba16f=ref["rgba16f"], steps=ref["steps"], cones=ref["cones"])
    dif, spc = cr.marched_groups(mask, aov)
    steps = np.array(ref["steps"], np.uint8, copy=True)
    if not dif:
        steps[:, :6] = 0
    if not spc:
        steps[:, 6] = 0
    cones = cr.masked_cones(ref["cones"], mask, aov)
    rgba = cr.composite(planes, cones, p.camera_pos[:], p.light_dir[:], p.ambient_factor, p.shininess, mask)["rgba32f"]
    return dict(rgba32f=rgba, rgba16f=cr.to_f16_bits(rgba), steps=steps, cones=cones)


def frame_ref(oracle, p, chain, planes, w, h, what, cache=None, nthreads=4):
    """The trace of `planes` ([23, w*h]) through `chain` under the oracle parameters `p` with `what` (attached()) in force.
    cache: a dict shared between calls on the same (chain, planes): the oracle's runs are kept in it.
    Returns dict(steps [npix, 7], cones [npix, 7, 4], total_steps, rgba32f (the composite before the last add), frame16
    (fp16 bits of the frame), frame32 (fp32 [npix, 4]: rgba32f, or frame16's values where planes are added -- the add is
    emission_ref.frame's, which returns halves), lit (the lit planes [3, npix], the emission planes without lights, or None),
    marched (rate 2: the pixels that march their own diffuse cones; None at rate 1), outputs {AOV bit: fp32 [npix, 4]},
    live, sel [npix] bool (the pixels of the launched rows), shininess (scalar or [npix])).  Outside `sel` nothing is meant."""
    g = np.asarray(planes, f32)
    npix = w * h
    assert g.shape == (23, npix)
    cache = {} if cache is None else cache
    cam, light = [float(v) for v in p.camera_pos], [float(v) for v in p.light_dir]
    mask, aov = what["mask"], what["aov"]
    live = ~(g[18] < f32(0.5))
    # 1. cones: per gloss class an oracle run (with the sky), per pixel the run of its class
    if what["classes"] is not None:
        runs = [_class_run(oracle, gr.class_params(p, c), chain, g, what, cache, nthreads) for c in what["classes"]]
        ref = gr.select(runs, what["gloss_plane"], what["classes"])
        shin = lr.class_shininess(what["gloss_plane"], what["classes"])
    else:
        ref = _class_run(oracle, p, chain, g, what, cache, nthreads)
        shin = p.shininess
    # 2. the gather and the composite under the mask
    marched = None
    if what["rate"] == 2:
        assert what["rows"] is None, "diffuse rate 2 traces whole frames only"
        r2 = drr.restate(g, w, h, f32(p.G) / f32(p.V), ref, cam, light, p.ambient_factor, shin, mask, aov)
        steps, cones, rgba32f, marched = r2["steps"], r2["cones"], r2["rgba32f"], r2["marched"]
        parts = r2
    else:
        steps, cones, rgba32f = np.asarray(ref["steps"]), np.asarray(ref["cones"], f32), np.asarray(ref["rgba32f"], f32)
        parts = cr.composite(g, cones, cam, light, p.ambient_factor, shin, mask) if aov else None
    outputs = {}
    if aov & cr.AOV_INDIRECT_DIFFUSE:
        outputs[cr.AOV_INDIRECT_DIFFUSE] = parts["ind"]
    if aov & cr.AOV_INDIRECT_SPECULAR:
        outputs[cr.AOV_INDIRECT_SPECULAR] = parts["spec_cone"]
    if aov & cr.AOV_DIRECT:
        outputs[cr.AOV_DIRECT] = parts["direct"]
    # 3. the planes of the last add: E, or E + Lit with lights attached
    lit = what["emission"]
    if what["lights"]:
        lit = lr.lit_planes(g, what["lights"], cam, shin, mask=mask, E=what["emission"])
    if lit is not None:
        frame16 = er.frame(rgba32f, g, lit)
        frame32 = frame16.view(np.float16).astype(f32)
    else:
        frame16, frame32 = cr.to_f16_bits(rgba32f), rgba32f
    sel = np.ones(npix, bool)
    if what["rows"] is not None:
        y = np.arange(npix) // w
        sel = np.isin(y // 8, what["rows"])
    total = int(np.asarray(steps)[sel].astype(np.int64).sum())
    return dict(steps=steps, cones=cones, total_steps=total, rgba32f=rgba32f, frame16=frame16, frame32=frame32, lit=lit,
                marched=marched, outputs=outputs, live=live, sel=sel, shininess=shin)
