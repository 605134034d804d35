#!/usr/bin/env python3
"""Issue-cycle model of the trace kernel's march loop (no GPU needed).

    tools/valu_model.py  [--write]

Compiles csrc/vct_trace.hip to gfx950 assembly, takes the specular march loop of
k_trace_tile_split<true, 1, SF_PRIO | SF_CHAIN> (csrc/vct_trace_forms.h; the whole-frame instantiation of a chain whose
levels start below 4 GiB: one texel buffer per wave; the diffuse loop has the
same body), splits it at its labels into basic blocks, tells the blocks of a level sample apart by what they hold
(coordinates, fit test against the held block, reuse, fresh anchor, fetch, LDS write, gather, zero result, per-lane
gather: see main) and prices every VALU instruction with the issue cost MEASURED for its class on this GPU
(tools/valu_bench.hip at 8 waves per SIMD, gpurun_out/valu_bench.txt; classes it does not cover are priced as
4-cycle ops).  Each block is weighted with the frequency at which the instrumented build executes it
(profiles/r07_reuse_stats.json: tools/trace_stats.py on the default workload).

Round 18 adds the scalar table: scalar-ALU instructions and branches of every segment and of every route of a level
sample (held block filled / all zero, fresh block filled / all zero, per lane) x the same frequencies, so that the
scalar stream per wave-step can be set against SQ_INSTS_SALU per launch route by route.  `--source FILE` prices another
copy of vct_trace.hip (the parent's, for the predicted difference); nothing is written then.

Output: VALU instructions and issue cycles per wave-step and the mean issue cycles per instruction -- the factor
bench.py uses for `roofline.valu_pipe_busy_model` (profiles/valu_model.json, keyed by the kernel-source sha).
The segmentation relies on the block layout the compiler currently emits; the script checks the instruction
counts it finds (plus the tile's work outside the march) against the per-wave-step count of the PMC profile and refuses
to write on a mismatch > 8 %.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# tools/valu_bench.hip at 8 waves per SIMD (the march runs at 7), x 0.96: the bench prints cycles for an assumed
# 2.4 GHz and its scalar-ALU lines (one instruction per 4 cycles per SIMD by construction) read 4.17
COST = {"fma": 2.42, "mul": 2.20, "add": 2.18, "logic2": 2.25, "cvt": 3.95, "floor": 3.95, "int3": 4.0, "max": 3.96,
        "cndmask": 2.4, "readlane": 4.0, "cmp": 2.4, "mov": 2.3, "mul_lo": 4.0, "other": 4.0}
SALU_CYCLES = 4.0       # s_add / s_and / s_mul / s_lshl: 4.17 "cycles @2.4 GHz" at 1, 4 and 8 waves per SIMD


def classify(op):
    if op.startswith(("v_fma", "v_fmac")): return "fma"
    if op.startswith("v_mul_f32"): return "mul"
    if op.startswith(("v_mul_lo", "v_mad")): return "mul_lo"
    if op.startswith(("v_add_f32", "v_sub_f32", "v_subrev_f32")): return "add"
    if op.startswith(("v_add_u32", "v_sub_u32", "v_subrev_u32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_lshlrev_b32",
                      "v_lshrrev_b32", "v_not")): return "logic2"
    if op.startswith("v_cvt"): return "cvt"
    if op.startswith(("v_floor", "v_fract")): return "floor"
    if op.startswith(("v_or3", "v_add3", "v_lshl_add", "v_lshl_or", "v_and_or", "v_bitop3", "v_bfe", "v_add_lshl", "v_perm")): return "int3"
    if op.startswith(("v_max", "v_min", "v_med3")): return "max"
    if op.startswith("v_cndmask"): return "cndmask"
    if op.startswith(("v_readlane", "v_readfirstlane")): return "readlane"
    if op.startswith("v_cmp"): return "cmp"
    if op.startswith("v_mov"): return "mov"
    return "other"


def price(lines):
    ops = [ln.split()[0] for ln in lines if re.match(r"\s+v_", ln)]
    return len(ops), sum(COST[classify(o)] for o in ops)


NOT_SALU = ("s_waitcnt", "s_nop", "s_setprio", "s_load", "s_buffer_load", "s_barrier", "s_endpgm", "s_sleep")


def scalars(lines):
    """(scalar-ALU instructions, branches) of a block: what the scalar pipe issues, without waits, loads and priority."""
    ops = [ln.split()[0] for ln in lines if re.match(r"\s+s_", ln)]
    br = sum(1 for o in ops if o.startswith(("s_cbranch", "s_branch")))
    return sum(1 for o in ops if not o.startswith(NOT_SALU)) - br, br


def split_kernel_label(asm, wrap, fastdiv, flags):
    """The assembly label of k_trace_tile_split<wrap, fastdiv, FORM>, FORM = the OR of the named bits of
    csrc/vct_trace_forms.h (read from the header): found by the demangled name, not by a mangled string."""
    hdr = open(os.path.join(ROOT, "voxel-cone-tracing_amd", "csrc", "vct_trace_forms.h")).read()
    bits = {name: 1 << int(sh) for name, sh in re.findall(r"\b(SF_[A-Z]+) = 1u << (\d+)", hdr)}
    word = sum(bits[f] for f in flags)
    labels = sorted(set(re.findall(r"^(_Z\w*k_trace_tile_split\w*):", asm, re.M)))
    names = subprocess.run(["c++filt"], input="\n".join(labels), capture_output=True, text=True, check=True).stdout.split("\n")
    want = "k_trace_tile_split<%s, %d, (VctSplitForm)%d>(" % ("true" if wrap else "false", fastdiv, word)
    found = [lb for lb, name in zip(labels, names) if want in name]
    assert len(found) == 1, (want, found)
    return found[0]


def kernel_text(asm, label):
    return re.search(r"^" + re.escape(label) + r":.*?\.end_amdhsa_kernel", asm, re.S | re.M).group(0)


def main():
    src = os.path.join(ROOT, "voxel-cone-tracing_amd", "csrc", "vct_trace.hip")
    other = "--source" in sys.argv
    if other:
        src = sys.argv[sys.argv.index("--source") + 1]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "t.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-slp-vectorize", "-fPIC", "-Wno-unused-function", "-S", "--cuda-device-only",
                        "-I", os.path.join(ROOT, "voxel-cone-tracing_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", out, src],
                       check=True, capture_output=True)
        text = open(out).read()
    body = kernel_text(text, split_kernel_label(text, True, 1, ("SF_PRIO", "SF_CHAIN"))).split("\n")
    # the specular march = the largest depth-1 inner loop (the diffuse march, inside the cone loop, is depth 2 and has the
    # same body; small depth-1 loops, if any, are prologue code)
    loops = [i for i, ln in enumerate(body) if "Inner Loop Header: Depth=1" in ln]

    def loop_at(start):
        end = next(i for i in range(start + 1, len(body)) if re.match(r"\.LBB\d+_\d+:\s*$", body[i]))   # first label outside the loop
        return body[start:end]
    loop = max((loop_at(i) for i in loops), key=len)
    # blocks of the loop, split at labels
    blocks, cur = [], []
    for ln in loop:
        if (re.match(r"\.LBB\d+_\d+:", ln) or re.match(r";\s*%bb\.\d+:", ln)) and cur:
            blocks.append(cur); cur = []
        cur.append(ln)
    blocks.append(cur)
    # Round 7 (block reuse): a level sample is a chain of small blocks, told apart by what they hold, each executed
    # with the frequency the instrumented build measured for it (profiles/r07_reuse_stats.json, default apertures):
    #   coords   level coordinates (the first level's block also holds the step's position and constant divisions)
    #   cand     fit test against the held block            -- samples with a candidate
    #   hit      LDS offset of a reused block               -- samples served from the held block
    #   anchor   anchor + fit test of a fresh block         -- samples not served from the held block
    #   fetch    dilated index, typed load, zero ballot     -- cooperative samples that fetch
    #   write    ds_write of the block, LDS offset          -- ... whose block is not all zero
    #   gather   8 ds_read_b128 + the trilinear fold        -- reused or fetched, block not all zero
    #   zero     the four v_mov of a sample that is +0      -- priced as executed whenever the gather is not
    #   lane     per-lane gather (8 typed loads) and its preamble
    # Everything else (blend, composite, loop control) is executed once per step.
    stats = json.load(open(os.path.join(ROOT, "profiles", "r07_reuse_stats.json")))["launches"][0]
    n_s = float(stats["level_samples"])
    reused = sum(stats[f"reuse_hits_{w}_{l}"] for w in ("diffuse", "specular") for l in ("first", "second"))
    reused_zero = sum(stats[f"reuse_hits_zero_{w}_{l}"] for w in ("diffuse", "specular") for l in ("first", "second"))
    cands = sum(stats[f"reuse_candidates_{w}_{l}"] for w in ("diffuse", "specular") for l in ("first", "second"))
    f_hit, f_cand, f_lane = reused / n_s, cands / n_s, stats["fallback"] / n_s
    f_fetch, f_write = (stats["coop_zero"] + stats["coop_hit"]) / n_s, stats["coop_hit"] / n_s
    f_gather = f_write + (reused - reused_zero) / n_s
    freq = {"coords": 1.0, "cand": f_cand, "hit": f_hit, "anchor": 1.0 - f_hit, "fetch": f_fetch, "write": f_write,
            "gather": f_gather, "zero": 1.0 - f_gather, "lane": f_lane, "route": 1.0, "step": 1.0}
    second = n_s / stats["wave_steps"] - 1.0          # level samples per wave-step: the second level only where two_levels

    def kind(b):
        t = "\n".join(b)
        loads = sum(1 for ln in b if "buffer_load_format_xyzw" in ln)
        nv = price(b)[0]
        if loads >= 6: return "lane"
        if t.count("ds_read_b128") >= 8: return "gather"
        if "ds_write_b128" in t: return "write"
        if loads == 1: return "fetch"
        if "v_readlane" in t: return "anchor"
        if "v_max3_u32" in t: return "cand"
        if "v_floor" in t: return "coords"
        if "s_setprio 0" in t: return "hit"
        if "s_setprio 1" in t and nv <= 6: return "lane"      # (the per-lane path's preamble)
        if nv == 4 and all("v_mov_b32" in ln for ln in b if re.match(r"\s+v_", ln)): return "zero"
        # round 18: a block that only compares and branches on the sampler's routing word (priced per sample in the scalar table)
        if nv == 0 and "s_cmp" in t and sum(scalars(b)) <= 6 and "s_load" not in t and "s_add" not in t: return "route"
        return "step"
    kinds = [kind(b) for b in blocks]
    # the march is unrolled by two (cone_march): two identical steps per loop body -- model the first
    heads = [i for i, (k, b) in enumerate(zip(kinds, blocks)) if k == "coords" and price(b)[0] >= 20]
    assert len(heads) == 2 and kinds.count("lane") >= 4 and kinds.count("gather") == 4, kinds
    first_step = range(heads[0] - 1 if heads[0] > 0 else 0, heads[1] - 1)
    seg = {}
    sseg = {1: {}, 2: {}}       # scalar table: level of the step -> segment -> [scalar-ALU instructions, branches]
    n_step = c_step = s_step = b_step = 0.0
    level = 0
    for i in first_step:
        k = kinds[i]
        if k == "coords": level += 1
        wgt = freq[k] * (second if (level == 2 and k != "step") else 1.0)
        n, c = price(blocks[i])
        n_step += wgt * n; c_step += wgt * c
        e = seg.setdefault(k, [0, 0.0]); e[0] += n; e[1] = round(e[1] + c, 1)
        sa, sb = scalars(blocks[i])
        s_step += wgt * sa; b_step += wgt * sb
        e = sseg[max(level, 1)].setdefault(k, [0, 0]); e[0] += sa; e[1] += sb
    # routes of a level sample: the segments a route passes (static counts: every block of a segment, so a route's count
    # is an upper bound where a segment holds blocks of more than one route -- `route`, the compare-and-branch blocks, is
    # charged whole to every route) x the route's share of the level samples
    ROUTES = {"held_filled": ("coords", "cand", "hit", "route", "gather"), "held_zero": ("coords", "cand", "hit", "route", "zero"),
              "fresh_filled": ("coords", "anchor", "fetch", "write", "route", "gather"),
              "fresh_zero": ("coords", "anchor", "fetch", "route", "zero"), "per_lane": ("coords", "anchor", "route", "zero", "lane")}
    f_route = {"held_filled": (reused - reused_zero) / n_s, "held_zero": reused_zero / n_s, "fresh_filled": f_write,
               "fresh_zero": stats["coop_zero"] / n_s, "per_lane": f_lane}
    routes = {}
    for lvl in (1, 2):
        for r, ks in ROUTES.items():
            routes[f"level{lvl}_{r}"] = {"scalar_alu": sum(sseg[lvl].get(k, [0, 0])[0] for k in ks),
                                         "branches": sum(sseg[lvl].get(k, [0, 0])[1] for k in ks),
                                         "share_of_level_samples": round(f_route[r], 4)}
    res = {"segments": seg, "segment_frequencies": {k: round(v, 4) for k, v in freq.items()},
           "second_level_samples_per_wave_step": round(second, 4),
           "valu_per_wave_step_model": round(n_step, 1), "issue_cycles_per_wave_step_model": round(c_step, 1),
           "model_issue_cycles_per_valu_instr": round(c_step / n_step, 3),
           "cost_table_cycles": COST,
           "scalar_segments": {f"level{l}": v for l, v in sseg.items()}, "scalar_routes": routes,
           "salu_per_wave_step_model": round(s_step, 1), "branches_per_wave_step_model": round(b_step, 1),
           "kernel_static": {"scalar": sum(sum(scalars([ln])) for ln in body), "v_readlane_writelane": sum(
               1 for ln in body if re.match(r"\s+v_(readlane|writelane)", ln))}}
    if other:
        print(json.dumps(res, indent=1))
        return
    import bench
    res["kernel_source_sha16"] = bench.kernel_source_sha()
    tt = os.path.join(ROOT, "profiles", "trace_traffic.json")
    if os.path.exists(tt):
        t = json.load(open(tt))
        measured = t["wave_instructions_per_launch"]["valu"] / stats["wave_steps"]      # (the r07 statistics' wave steps)
        res["valu_per_wave_step_pmc"] = round(measured, 1)
        res["salu_per_wave_step_pmc"] = round(t["wave_instructions_per_launch"]["salu"] / stats["wave_steps"], 1)
        res["pipe_busy_model"] = round(t["wave_instructions_per_launch"]["valu"] * res["model_issue_cycles_per_valu_instr"]
                                       / 1024.0 / t["gpu_cycles_per_launch"], 3)
        # the scalar pipe: one instruction per 4 cycles per SIMD (measured), SALU + SMEM instructions of the launch
        res["salu_issue_cycles_per_instr"] = SALU_CYCLES
        res["salu_pipe_busy_model"] = round(t["wave_instructions_per_launch"]["salu"] * SALU_CYCLES
                                            / 1024.0 / t["gpu_cycles_per_launch"], 3)
        # the PMC count also holds what a tile executes outside the march -- prologue, per-cone set-up, composite: about
        # 1,530 VALU wave-instructions per tile (1,700 before the tile's divisions, the light vector and
        # the second E left the waves: -170 per tile by SQ_INSTS_VALU) of the default 1080p frame's 240 x 135 tiles
        outside = 1530.0 * 240 * 135 / stats["wave_steps"]
        res["valu_per_wave_step_outside_march"] = round(outside, 1)
        ok = abs(measured - (n_step + outside)) / measured < 0.08
    else:
        ok = False
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        if not ok:
            sys.exit("model and PMC instruction counts per wave-step differ by more than 8 %: not written")
        with open(os.path.join(ROOT, "profiles", "valu_model.json"), "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
