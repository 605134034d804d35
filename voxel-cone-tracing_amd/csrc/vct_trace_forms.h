// vct_trace_forms.h -- the forms of the trace kernels as named bits, the table of the forms that exist, and the one rule
// that maps a launch to its kernel (no HIP calls: host and device code, and a plain g++ program -- tests/
// trace_forms_check_main.cpp -- include it).  Tables and rules only: the kernels are vct_trace.hip's.
//
// A FORM is what used to be a list of positional template flags: one word, every flag a named bit, so a call site says
// which flags it sets and a flag more is a bit more, not a position more in every list.  Three kinds of form, three
// enum types (a form of one kind does not convert to another's):
//   VctSplitForm   k_trace_tile_split<WRAP, FASTDIV, FORM>                          SF_*   split_form(bits)
//   VctMarchForm   cone_march<WRAP, FASTDIV, MARCH, SKY>                            MF_*   march_form(bits)
//   VctLevelForm   sample_level, sample_level_reuse, sample_step_level<WRAP, LEVEL> LF_*   level_form(bits)
// The kernel derives its march form from its own form in one place (split_march_form), the march the form of its level
// samples in one place (march_level_form).
//
// To add a form: one bit below, one row in kVctSplitForms, one line in vct_plan_launch, and one line in the restatement
// of tests/trace_forms_check_main.cpp (DESIGN.md "Kernel forms and the launch plan").
#ifndef VCT_TRACE_FORMS_H_
#define VCT_TRACE_FORMS_H_

// ---- build-time bounds the form rules read (A/B builds override them: tools/build_ab.sh) ---------------------------------
#ifndef VCT_TRACE_MIN_WAVES
#define VCT_TRACE_MIN_WAVES 7     // waves per SIMD the register allocator must leave room for (<= 72 VGPRs).  A/B on the
                                  // final round-2 kernel (ms at 256^3/1080p): 4: 0.776, 5: 0.775, 6: 0.7235, 7: 0.695, 8: 0.719
                                  // (spills); with the two-plane gather 7: 0.683 (69 VGPRs, no scratch), 8: 0.689; gathering texel pairs: 7: 0.685, 8: 0.684
#endif
#ifndef VCT_ANISO_MIN_WAVES
#define VCT_ANISO_MIN_WAVES 5     // A/B (ms, 256^3 1080p): 4: 1.61, 5: 1.47, 6: 1.88 (spills), 7: 1.60
#endif
#ifndef VCT_SPLIT_MAX_WAVES
#define VCT_SPLIT_MAX_WAVES 8
#endif
// -DVCT_REUSE=0 builds the kernels without block reuse (vct_trace.hip BlockDesc): kept for A/B builds, like VCT_STATS.
#ifndef VCT_REUSE
#define VCT_REUSE 1
#endif

// ---- k_trace_tile_split ---------------------------------------------------------------------------------------------------
// (the anisotropic instantiation carries three samples' worth of state: it gets 128 VGPRs instead of
// spilling under the 80 of the default kernel)
// CELLS: the per-lane sampler reads footprint records (p.cells_biased != null; vct_set_footprint_records) -- an
// instantiation of its own, because the same code behind a run-time test cost the default kernel 2 % (0.608 -> 0.620 ms)
// COMPACT: the live-pixel compaction experiment (trace_variant 4): the wave's pixels come from the compaction list
// COMP: lighting components (p.comp; vct_set_lighting_components, vct_set_aov_outputs) -- a wave whose cone group
// nothing reads marches nothing, the composite applies the VCT_SHOW_* mask, and the per-component outputs are stored
// beside the frame.  An instantiation of its own for the same reason as CELLS: the default kernels carry none of it.
// HALF: the last launch of a half-rate pass (vct_set_diffuse_rate(ctx, 2); "Half-rate diffuse gather" in vct_trace.hip):
// the diffuse waves march nothing and leave the debug outputs to the launches in front of this one, and the composite
// takes the pixel's gather from p.dr_ind instead of the cones in LDS.  Instantiated with COMP and PRIO only (whole frames).
// GLOSS: gloss classes (include/vct.h "per-material gloss"; p.pix_gloss, p.gloss): the specular wave marches once per class
// present among its live lanes, each time with that class's step table and the other lanes masked off, and the composite
// takes the lane's Phong exponent from the class headers.  Instantiated with COMP, for the plain, PRIO and HALF forms.
// SKY: sky light (include/vct.h "sky light"; p.sky): every marched cone adds what its open remainder gathers from the
// sky -- cone_march<.., VCT_SKY_INSIDE>, or, with GLOSS, one sky_epilogue per lane behind the class loop.  Instantiated
// with COMP, for the plain, PRIO and HALF forms, each with and without GLOSS.
// PRIO: issue priority raised around every sample's loads (sample_level): the launches of whole frames.
// CHAIN: one texel buffer per wave, a level's byte offset in the load's scalar operand (vct_trace.hip ChainRef).
enum VctSplitForm : unsigned {
    SF_PLAIN = 0u,
    SF_ANISO = 1u << 0,
    SF_COMPACT = 1u << 1,
    SF_CELLS = 1u << 2,
    SF_PRIO = 1u << 3,
    SF_COMP = 1u << 4,
    SF_HALF = 1u << 5,
    SF_GLOSS = 1u << 6,
    SF_SKY = 1u << 7,
    SF_CHAIN = 1u << 8,
};
constexpr VctSplitForm split_form(unsigned bits) { return (VctSplitForm)bits; }

// The split forms that exist.  Each is built for FASTDIV 0 and 1 under GL_REPEAT and -- but for the CELLS and CHAIN forms,
// which need WRAP (split_form_exists) -- in clamp mode; the loose kernel of variant 3 (FASTDIV 2, SF_PLAIN) comes on top.
constexpr VctSplitForm kVctSplitForms[] = {
    // plain x {PRIO} x {COMP} x {CHAIN}
    split_form(SF_PLAIN), split_form(SF_PRIO), split_form(SF_COMP), split_form(SF_PRIO | SF_COMP),
    split_form(SF_CHAIN), split_form(SF_PRIO | SF_CHAIN), split_form(SF_COMP | SF_CHAIN), split_form(SF_PRIO | SF_COMP | SF_CHAIN),
    // anisotropic chains, footprint records: x {COMP}; the compaction experiment
    split_form(SF_ANISO), split_form(SF_ANISO | SF_COMP),
    split_form(SF_CELLS), split_form(SF_CELLS | SF_COMP),
    split_form(SF_COMPACT),
    // gloss classes x {PRIO}; sky light x {GLOSS} x {PRIO}
    split_form(SF_COMP | SF_GLOSS), split_form(SF_COMP | SF_GLOSS | SF_PRIO),
    split_form(SF_COMP | SF_SKY), split_form(SF_COMP | SF_SKY | SF_PRIO),
    split_form(SF_COMP | SF_SKY | SF_GLOSS), split_form(SF_COMP | SF_SKY | SF_GLOSS | SF_PRIO),
    // the last launch of a half-rate pass x {SKY} x {GLOSS}
    split_form(SF_HALF | SF_PRIO | SF_COMP), split_form(SF_HALF | SF_PRIO | SF_COMP | SF_SKY),
    split_form(SF_HALF | SF_PRIO | SF_COMP | SF_GLOSS), split_form(SF_HALF | SF_PRIO | SF_COMP | SF_SKY | SF_GLOSS),
};
constexpr int kVctSplitFormCount = (int)(sizeof(kVctSplitForms) / sizeof(kVctSplitForms[0]));
// the sampler reads footprint records under GL_REPEAT only, and a byte offset per level serves GL_REPEAT chains only
constexpr bool split_form_exists(bool wrap, VctSplitForm f) { return wrap || !(f & (SF_CELLS | SF_CHAIN)); }
// k_trace_tile_split kernels in the code object: the table under both wrap modes and both exact divisions + the two loose ones
constexpr int split_kernel_count() {
    int n = 2;
    for (int i = 0; i < kVctSplitFormCount; ++i)
        n += 2 * ((split_form_exists(true, kVctSplitForms[i]) ? 1 : 0) + (split_form_exists(false, kVctSplitForms[i]) ? 1 : 0));
    return n;
}

// what a form must come with (checked where the kernel is instantiated)
template <bool WRAP, VctSplitForm F>
struct VctSplitFormChecked {
    static constexpr bool kDefaultComp = (F & SF_COMP) && !(F & (SF_ANISO | SF_COMPACT | SF_CELLS));
    static_assert(!(F & SF_GLOSS) || kDefaultComp, "gloss classes: the default kernel's COMP forms only");
    static_assert(!(F & SF_SKY) || kDefaultComp, "sky light: the default kernel's COMP forms only");
    static_assert(!(F & SF_CHAIN) || (WRAP && !(F & (SF_ANISO | SF_COMPACT | SF_CELLS))),
                  "one texel buffer per wave (ChainRef): the plain GL_REPEAT forms only");
    static constexpr bool value = true;
};

// Waves per SIMD of an instantiation (its launch bound): 8, with the two-texel gathers (NARROW), for the whole-frame
// forms (PRIO) under GL_REPEAT, which fit 64 registers without scratch -- and for the footprint-record forms (CELLS), which
// ran 8 waves in 64 registers under the bound of 7 until the hand-over took a 65th.  Everything else keeps the bound of 7
// and the four-texel gathers: clamp mode (66-72 registers), the HALF forms (56-64 registers: 8 waves without being asked),
// the compaction experiment, and the forms without PRIO -- launches of at most half the frame, the slabs of a multi-GPU
// frame: an eighth of a frame is 16 tiles per CU, too few for residency to bind, and the 8-wave form's 1.6 % more
// vector instructions made those launches 0.2 - 1.5 % slower.  Both forms give the same bits.
// (A cap on the vector registers alone -- amdgpu_num_vgpr(64) under the bound of 7, which keeps six more scalar
// registers and 30 scalars out of the spill lanes -- does not get the eighth wave: +2.9 % against the parent where the
// bound of 8 measures -2 %.)  -DVCT_SPLIT_MAX_WAVES=7 builds every form with the bound of 7: kept for A/B builds
// (tools/build_ab.sh), like VCT_REUSE.  Resource lines: profiles/experiments/r16_occupancy_kernels.txt.
constexpr int split_min_waves(bool wrap, VctSplitForm f) {
    if (f & SF_ANISO) return VCT_ANISO_MIN_WAVES;
    const bool fits = wrap && !(f & (SF_COMPACT | SF_HALF)) && (f & (SF_CELLS | SF_PRIO));
    return fits && VCT_SPLIT_MAX_WAVES >= 8 ? 8 : VCT_TRACE_MIN_WAVES;
}
// NARROW: two texels in flight where there are four (gather_block, sample_level): the forms under the bound of 8
constexpr bool split_narrow(bool wrap, VctSplitForm f) { return !(f & SF_ANISO) && split_min_waves(wrap, f) >= 8; }
// block reuse (vct_trace.hip BlockDesc): the plain, PRIO, COMP, HALF and loose instantiations under GL_REPEAT; the others
// -- and clamp mode, where the descriptor costs the kernel 12 B of scratch per lane -- sample as before
constexpr bool split_reuse(bool wrap, VctSplitForm f) { return VCT_REUSE && wrap && !(f & (SF_ANISO | SF_CELLS | SF_COMPACT)); }

// ---- cone_march -------------------------------------------------------------------------------------------------------------
// COOP: the cooperative 4x4x4 block where the wave's footprints fit one (else every sample is a per-lane gather).
// REUSE: `held` describes the block in the wave's second slab; the caller keeps it across the cones of a wave.
// ANISO, CELLS, PRIO, NARROW, CHAIN: as the kernel's.  (The sky mode of a march -- VCT_SKY_NONE / INSIDE / ALPHA, three
// values -- is a template parameter of its own.)
enum VctMarchForm : unsigned {
    MF_NONE = 0u,
    MF_COOP = 1u << 0,
    MF_ANISO = 1u << 1,
    MF_CELLS = 1u << 2,
    MF_PRIO = 1u << 3,
    MF_REUSE = 1u << 4,
    MF_NARROW = 1u << 5,
    MF_CHAIN = 1u << 6,
};
constexpr VctMarchForm march_form(unsigned bits) { return (VctMarchForm)bits; }
// the march of a split kernel's waves
constexpr VctMarchForm split_march_form(bool wrap, VctSplitForm f) {
    return march_form(MF_COOP | ((f & SF_ANISO) ? MF_ANISO : 0u) | ((f & SF_CELLS) ? MF_CELLS : 0u) | ((f & SF_PRIO) ? MF_PRIO : 0u) |
                      (split_reuse(wrap, f) ? MF_REUSE : 0u) | (split_narrow(wrap, f) ? MF_NARROW : 0u) |
                      ((f & SF_CHAIN) ? MF_CHAIN : 0u));
}

// ---- sample_level, sample_level_reuse, sample_step_level ---------------------------------------------------------------------
// LOOSE: the one-multiply unorm8 decode of variant 3's kernel (FASTDIV 2), not exact.  REUSE: sample_step_level goes
// through sample_level_reuse.  The others: as the march's.
enum VctLevelForm : unsigned {
    LF_NONE = 0u,
    LF_COOP = 1u << 0,
    LF_LOOSE = 1u << 1,
    LF_CELLS = 1u << 2,
    LF_PRIO = 1u << 3,
    LF_REUSE = 1u << 4,
    LF_NARROW = 1u << 5,
    LF_CHAIN = 1u << 6,
};
constexpr VctLevelForm level_form(unsigned bits) { return (VctLevelForm)bits; }
constexpr VctLevelForm level_form_without(VctLevelForm f, unsigned bits) { return level_form(f & ~bits); }
// the level samples of a march (its isotropic ones: sample_aniso has no form)
constexpr VctLevelForm march_level_form(VctMarchForm m, int fastdiv) {
    return level_form(((m & MF_COOP) ? LF_COOP : 0u) | (fastdiv == 2 ? LF_LOOSE : 0u) | ((m & MF_CELLS) ? LF_CELLS : 0u) |
                      ((m & MF_PRIO) ? LF_PRIO : 0u) | ((m & MF_REUSE) ? LF_REUSE : 0u) | ((m & MF_NARROW) ? LF_NARROW : 0u) |
                      ((m & MF_CHAIN) ? LF_CHAIN : 0u));
}

// ---- the launch plan --------------------------------------------------------------------------------------------------------
// strided (row_stride > 1) and packed tile rows are read by k_trace_tile_split's own tiles only: not by the one-wave
// kernel (variants 1, 2) nor by the compaction's virtual tiles (4)
static inline bool vct_variant_takes_row_subsets(int variant) { return variant == 0 || variant == 3; }

// What vct_launch_trace knows about a launch before it picks a kernel (from config.trace_variant and VctTraceParams).
struct VctLaunchFacts {
    int variant;            // config.trace_variant 0 .. 4 (include/vct.h)
    bool wrap;              // GL_REPEAT (p.wrap_repeat), else clamp
    bool fast_div;          // the step tables were built for the verified two-term product (p.fast_div)
    bool aniso;             // anisotropic chains (p.aniso)
    bool cells;             // footprint records (p.cells_biased)
    bool comp;              // lighting components on (p.comp != 0)
    bool sky;               // sky light (p.sky)
    bool gloss_plane;       // gloss classes: the pixel-gloss plane (p.pix_gloss) ...
    bool gloss_table;       // ... and the class tables (p.gloss)
    bool half_rate;         // the buffers of a half-rate pass (p.dr_ind)
    bool compact_list;      // the compaction list (p.vt_pix)
    bool spec_prio;         // a launch of at most half the frame: the priority goes to the specular waves (p.spec_prio)
    bool chain_form;        // the context's chain admits byte offsets per level (p.chain_form)
    bool strided;           // p.row_stride > 1
    bool packed;            // p.pack_rows
    bool whole_frame;       // tile rows [0, tiles_y)
};
enum VctKernelFamily { VCT_FAMILY_TILE, VCT_FAMILY_SPLIT, VCT_FAMILY_HALF_RATE };
struct VctLaunchPlan {
    bool refused;               // no kernel serves these facts together: the launch is hipErrorInvalidValue
    VctKernelFamily family;     // k_trace_tile | k_trace_tile_split | the four launches of a half-rate pass
    bool coop;                  // k_trace_tile<.., COOP>
    VctSplitForm form;          // k_trace_tile_split's form (of a half-rate pass: its last launch's)
    int fastdiv;                // div_const's MODE: 0 IEEE, 1 the verified product, 2 variant 3's x * r
    // what vct_get_stage_counts reports: bits 0-7 the division (1 IEEE, 2 the verified product, 3 x * r), bits 8-9 how the
    // typed loads reach a level (2 one resource per wave: a CHAIN form of variant 0; 1 one per level).  Also of a refused
    // or an empty launch.
    int reported_form;
};

// The rule "which kernel does this launch take": here and nowhere else.
// variant 0 (default) the cooperative sampler with each tile split over 3 waves; 1 the per-lane sampler only and 2 the
// cooperative sampler, one wave per tile (with anisotropic chains both run the default kernel); 3 the default kernel with
// reciprocal-multiply divisions and the one-multiply decode -- never the default, not bit-exact: it exists to price the
// exactness (bench.py exactness_tax) -- and with anisotropic chains the default kernel; 4 the default kernel
// over the live-pixel compaction (the caller sets the list).
constexpr VctLaunchPlan vct_plan_launch(const VctLaunchFacts& f) {
    VctLaunchPlan pl = {false, VCT_FAMILY_SPLIT, false, split_form(SF_PLAIN), f.fast_div ? 1 : 0, 0};
    const bool loose = f.variant == 3 && !f.aniso;
    // lighting components: the COMP form of the same branch; whole frames (or most of one) take issue priority around
    // the samples' loads, launches of at most half the frame give it to the specular waves
    const unsigned comp = f.comp ? SF_COMP : 0u, prio = f.spec_prio ? 0u : SF_PRIO;
    if (!f.aniso && (f.variant == 1 || f.variant == 2)) {       // the anisotropic option exists in the default kernel only
        pl.family = VCT_FAMILY_TILE;
        pl.coop = f.variant == 2;
    } else if (loose) {
        pl.fastdiv = 2;
    } else if (f.compact_list) {
        pl.form = split_form(SF_COMPACT);
    } else if (f.half_rate) {                                   // whole frames only, so PRIO always
        pl.family = VCT_FAMILY_HALF_RATE;
        pl.form = split_form(SF_HALF | SF_PRIO | SF_COMP | (f.sky ? SF_SKY : 0u) | (f.gloss_plane ? SF_GLOSS : 0u));
    } else if (f.comp && f.sky) {
        pl.form = split_form(comp | SF_SKY | (f.gloss_plane ? SF_GLOSS : 0u) | prio);
    } else if (f.comp && f.gloss_plane) {
        pl.form = split_form(comp | SF_GLOSS | prio);
    } else if (f.aniso) {
        pl.form = split_form(SF_ANISO | comp);
    } else if (f.wrap && f.cells) {
        pl.form = split_form(SF_CELLS | comp);
    } else {        // the plain forms; under GL_REPEAT with one texel buffer per wave where the chain admits it
        pl.form = split_form(comp | prio | (f.chain_form && f.wrap && !f.sky && !f.gloss_plane ? SF_CHAIN : 0u));
    }
    pl.reported_form = (loose ? 3 : (f.fast_div ? 2 : 1)) | ((f.variant == 0 && (pl.form & SF_CHAIN) ? 2 : 1) << 8);
    // sky light, gloss classes and the half-rate pass have kernels in the default variant's COMP forms only, and none
    // beside anisotropic chains or footprint records; a half-rate pass traces whole frames
    const bool default_comp = f.variant == 0 && !f.aniso && !f.cells && f.comp;
    pl.refused = ((f.strided || f.packed) && !vct_variant_takes_row_subsets(f.variant)) ||
                 (f.gloss_plane && !(default_comp && f.gloss_table)) ||
                 (f.sky && !default_comp) ||
                 (f.half_rate && !(default_comp && !f.strided && !f.packed && f.whole_frame));
    return pl;
}

#endif
