// Stand-alone check of csrc/vct_trace_forms.h (built with ASan + UBSan by tests/test_trace_forms_host.py): the launch
// plan over every combination of the facts of a launch, against the dispatch of csrc/vct_trace.hip as it stood before the
// header existed (commit 43f2dc4).  That dispatch is restated below literally -- launch_v, launch_split, launch_half_rate,
// takes_chain_form and the refusals and march_form of vct_launch_trace, with the kernels' positional template lists as
// they were written there -- and is NOT computed from the header's table or rule.
// A new form gets one line here, in the branch of the restatement that launches it.
#include <stdio.h>
#include <string.h>

#include "../voxel-cone-tracing_amd/csrc/vct_trace_forms.h"

// ---- the restatement --------------------------------------------------------------------------------------------------------
struct Params {         // the fields of VctTraceParams the dispatch read; pointers as "set or not"
    bool chain_form, wrap_repeat, fast_div, sky, pix_gloss, gloss, aniso, cells_biased, dr_ind, vt_pix, spec_prio, comp;
    int row_stride, pack_rows, tile_row0, tile_row1, tiles_y;
};
struct Kernel {         // what a launch ran: the template arguments, by position
    enum Name { NONE, TILE, SPLIT } name;
    bool half_rate_pass;        // the three launches of a half-rate pass in front of it
    int WRAP, FASTDIV, COOP;    // k_trace_tile<WRAP, FASTDIV, COOP>
    // k_trace_tile_split<WRAP, FASTDIV, ANISO, COMPACT, CELLS, PRIO, COMP, HALF, GLOSS, SKY, CHAIN>
    bool ANISO, COMPACT, CELLS, PRIO, COMP, HALF, GLOSS, SKY, CHAIN;
};
static Kernel k_trace_tile(bool WRAP, int FASTDIV, bool COOP) {
    Kernel k;
    memset(&k, 0, sizeof(k));
    k.name = Kernel::TILE; k.WRAP = WRAP; k.FASTDIV = FASTDIV; k.COOP = COOP;
    return k;
}
static Kernel k_trace_tile_split(bool WRAP, int FASTDIV, bool ANISO, bool COMPACT = false, bool CELLS = false, bool PRIO = false,
                                 bool COMP = false, bool HALF = false, bool GLOSS = false, bool SKY = false, bool CHAIN = false) {
    Kernel k;
    memset(&k, 0, sizeof(k));
    k.name = Kernel::SPLIT; k.WRAP = WRAP; k.FASTDIV = FASTDIV;
    k.ANISO = ANISO; k.COMPACT = COMPACT; k.CELLS = CELLS; k.PRIO = PRIO; k.COMP = COMP; k.HALF = HALF; k.GLOSS = GLOSS; k.SKY = SKY;
    k.CHAIN = CHAIN;
    return k;
}

static bool takes_chain_form(const Params& p) {
    return p.chain_form && p.wrap_repeat && !p.sky && !p.pix_gloss && !p.aniso && !p.cells_biased;
}

static Kernel launch_split(bool WRAP, int FASTDIV, bool COMP, const Params& p) {
    if (COMP) {
        if (p.sky) {
            const bool gloss = p.pix_gloss, prio = !p.spec_prio;
            return k_trace_tile_split(WRAP, FASTDIV, false, false, false, prio, true, false, gloss, true);
        }
        if (p.pix_gloss) {
            if (!p.spec_prio) return k_trace_tile_split(WRAP, FASTDIV, false, false, false, true, true, false, true);
            else return k_trace_tile_split(WRAP, FASTDIV, false, false, false, false, true, false, true);
        }
    }
    if (p.aniso) return k_trace_tile_split(WRAP, FASTDIV, true, false, false, false, COMP);
    if (WRAP) {
        if (p.cells_biased) return k_trace_tile_split(WRAP, FASTDIV, false, false, true, false, COMP);
    }
    const bool CHAIN = WRAP && (WRAP && takes_chain_form(p));
    if (!p.spec_prio) return k_trace_tile_split(WRAP, FASTDIV, false, false, false, true, COMP, false, false, false, CHAIN);
    else return k_trace_tile_split(WRAP, FASTDIV, false, false, false, false, COMP, false, false, false, CHAIN);
}

static Kernel launch_half_rate(bool WRAP, int FASTDIV, const Params& p) {
    Kernel k;
    if (p.sky) {
        const bool gloss = p.pix_gloss;
        k = k_trace_tile_split(WRAP, FASTDIV, false, false, false, true, true, true, gloss, true);
    } else if (p.pix_gloss)
        k = k_trace_tile_split(WRAP, FASTDIV, false, false, false, true, true, true, true);
    else k = k_trace_tile_split(WRAP, FASTDIV, false, false, false, true, true, true);
    k.half_rate_pass = true;
    return k;
}

static Kernel launch_v(bool WRAP, int FASTDIV, const Params& p, int variant, bool loose) {
    if (!p.aniso && (variant == 1 || variant == 2))
        return variant == 1 ? k_trace_tile(WRAP, FASTDIV, false) : k_trace_tile(WRAP, FASTDIV, true);
    if (loose) return k_trace_tile_split(WRAP, 2, false);
    if (p.vt_pix) return k_trace_tile_split(WRAP, FASTDIV, false, true);
    if (p.dr_ind) return launch_half_rate(WRAP, FASTDIV, p);
    return launch_split(WRAP, FASTDIV, p.comp != 0, p);
}

struct Launch { bool refused; int march_form; Kernel kernel; };
static Launch vct_launch_trace(const Params& p, int variant) {
    Launch r;
    memset(&r, 0, sizeof(r));
    const int rstride = p.row_stride > 1 ? p.row_stride : 1;
    const bool loose = variant == 3 && !p.aniso;
    const bool chain = variant == 0 && !loose && !p.vt_pix && !p.dr_ind && takes_chain_form(p);
    r.march_form = (loose ? 3 : (p.fast_div ? 2 : 1)) | ((chain ? 2 : 1) << 8);
    r.refused = true;
    if ((rstride > 1 || p.pack_rows) && !(variant == 0 || variant == 3)) return r;
    if (p.pix_gloss && (variant != 0 || p.aniso || p.cells_biased || !p.comp || !p.gloss)) return r;
    if (p.sky && (variant != 0 || p.aniso || p.cells_biased || !p.comp)) return r;
    if (p.dr_ind && (variant != 0 || p.aniso || p.cells_biased || !p.comp || rstride > 1 || p.pack_rows || p.tile_row0 != 0 ||
                     p.tile_row1 != p.tiles_y))
        return r;
    r.refused = false;
    r.kernel = launch_v(p.wrap_repeat != 0, p.fast_div != 0 ? 1 : 0, p, variant, loose);
    return r;
}

// ---- the plan against it ----------------------------------------------------------------------------------------------------
static int table_index(VctSplitForm f) {
    for (int i = 0; i < kVctSplitFormCount; ++i)
        if (kVctSplitForms[i] == f) return i;
    return -1;
}

int main() {
    static_assert(kVctSplitFormCount == 23, "23 forms under GL_REPEAT");
    static_assert(split_kernel_count() == 82, "82 k_trace_tile_split kernels in the code object");
    int clamp_forms = 0;
    for (int i = 0; i < kVctSplitFormCount; ++i) {
        if (!split_form_exists(true, kVctSplitForms[i])) { printf("entry %d does not exist under GL_REPEAT\n", i); return 1; }
        if (split_form_exists(false, kVctSplitForms[i])) ++clamp_forms;
        if (table_index(kVctSplitForms[i]) != i) { printf("entry %d is in the table twice\n", i); return 1; }
    }
    if (clamp_forms != 17) { printf("%d forms in clamp mode\n", clamp_forms); return 1; }

    static const char* const kShapes[4] = {"whole frame", "slab", "strided", "packed"};
    bool planned[2][32] = {};          // [wrap][table entry]: some case that is not refused launches it
    bool loose_planned[2] = {false, false};
    long cases = 0, refused = 0;
    for (int variant = 0; variant <= 4; ++variant)
        for (int shape = 0; shape < 4; ++shape)
            for (unsigned bits = 0; bits < (1u << 12); ++bits) {
                VctLaunchFacts f;
                memset(&f, 0, sizeof(f));
                f.variant = variant;
                f.wrap = bits & 1u; f.fast_div = bits & 2u; f.aniso = bits & 4u; f.cells = bits & 8u; f.comp = bits & 16u;
                f.sky = bits & 32u; f.gloss_plane = bits & 64u; f.gloss_table = bits & 128u; f.half_rate = bits & 256u;
                f.compact_list = bits & 512u; f.spec_prio = bits & 1024u; f.chain_form = bits & 2048u;
                // tile rows of a frame of 8: all of them; a slab of at most half of them; every second row; a packed slab
                Params p;
                memset(&p, 0, sizeof(p));
                p.tiles_y = 8; p.tile_row0 = 0; p.tile_row1 = 8; p.row_stride = 1;
                if (shape == 1) { p.tile_row0 = 2; p.tile_row1 = 5; }
                if (shape == 2) p.row_stride = 2;
                if (shape == 3) { p.tile_row0 = 4; p.pack_rows = 1; }
                f.strided = p.row_stride > 1; f.packed = p.pack_rows != 0;
                f.whole_frame = p.tile_row0 == 0 && p.tile_row1 == p.tiles_y;
                p.chain_form = f.chain_form; p.wrap_repeat = f.wrap; p.fast_div = f.fast_div; p.sky = f.sky;
                p.pix_gloss = f.gloss_plane; p.gloss = f.gloss_table; p.aniso = f.aniso; p.cells_biased = f.cells;
                p.dr_ind = f.half_rate; p.vt_pix = f.compact_list; p.spec_prio = f.spec_prio; p.comp = f.comp;

                const Launch want = vct_launch_trace(p, variant);
                const VctLaunchPlan got = vct_plan_launch(f);
                ++cases;
#define FAIL(what) { printf("variant %d, %s, facts %03x: %s\n", variant, kShapes[shape], bits, what); return 1; }
                if (got.reported_form != want.march_form) FAIL("march_form differs")
                if (got.refused != want.refused) FAIL("refusal differs")
                if (got.refused) { ++refused; continue; }
                const Kernel& k = want.kernel;
                if (k.name == Kernel::TILE) {
                    if (got.family != VCT_FAMILY_TILE || (int)got.coop != k.COOP || got.fastdiv != k.FASTDIV) FAIL("k_trace_tile: another kernel")
                    continue;
                }
                if (got.family != (k.half_rate_pass ? VCT_FAMILY_HALF_RATE : VCT_FAMILY_SPLIT)) FAIL("family differs")
                if (got.fastdiv != k.FASTDIV) FAIL("FASTDIV differs")
                const VctSplitForm g = got.form;
                if (((g & SF_ANISO) != 0) != k.ANISO || ((g & SF_COMPACT) != 0) != k.COMPACT || ((g & SF_CELLS) != 0) != k.CELLS ||
                    ((g & SF_PRIO) != 0) != k.PRIO || ((g & SF_COMP) != 0) != k.COMP || ((g & SF_HALF) != 0) != k.HALF ||
                    ((g & SF_GLOSS) != 0) != k.GLOSS || ((g & SF_SKY) != 0) != k.SKY || ((g & SF_CHAIN) != 0) != k.CHAIN ||
                    (g & ~(SF_ANISO | SF_COMPACT | SF_CELLS | SF_PRIO | SF_COMP | SF_HALF | SF_GLOSS | SF_SKY | SF_CHAIN)))
                    FAIL("form differs")
                if (got.fastdiv == 2) {         // the loose kernel: on top of the table
                    if (g != SF_PLAIN) FAIL("the loose kernel has no flags")
                    loose_planned[f.wrap] = true;
                    continue;
                }
                const int at = table_index(g);
                if (at < 0) FAIL("planned form is not in the table")
                if (!split_form_exists(f.wrap, g)) FAIL("a GL_REPEAT-only form planned in clamp mode")
                planned[f.wrap][at] = true;
            }
    for (int wrap = 0; wrap < 2; ++wrap) {
        if (!loose_planned[wrap]) { printf("wrap %d: the loose kernel is never planned\n", wrap); return 1; }
        for (int i = 0; i < kVctSplitFormCount; ++i)
            if (planned[wrap][i] != split_form_exists(wrap != 0, kVctSplitForms[i])) {
                printf("wrap %d, table entry %d (form %03x): instantiated %d, planned %d\n", wrap, i, (unsigned)kVctSplitForms[i],
                       (int)split_form_exists(wrap != 0, kVctSplitForms[i]), (int)planned[wrap][i]);
                return 1;
            }
    }
    printf("trace_forms_check ok: %ld cases, %ld refused, %d forms (%d in clamp mode), %d kernels\n", cases, refused,
           kVctSplitFormCount, clamp_forms, split_kernel_count());
    return 0;
}
