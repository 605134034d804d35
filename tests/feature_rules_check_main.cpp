// Stand-alone check of csrc/vct_feature_rules.h (built with ASan + UBSan by tests/test_feature_rules_host.py): every
// subset of the features against every subset of the modes.  The matrix below is written out by hand from the setters
// as they were before the header existed -- it is NOT computed from the header's table.
#include <stdio.h>

#include "../voxel-cone-tracing_amd/csrc/vct_feature_rules.h"

struct Pair { unsigned feature, mode; };
static const Pair kMatrix[] = {
    // a lighting-component mask other than VCT_SHOW_ALL
    {VCT_FEAT_MASK, VCT_MODE_VARIANT},
    // per-component outputs
    {VCT_FEAT_AOV, VCT_MODE_VARIANT}, {VCT_FEAT_AOV, VCT_MODE_COMM},
    // diffuse rate 2
    {VCT_FEAT_RATE2, VCT_MODE_VARIANT}, {VCT_FEAT_RATE2, VCT_MODE_ANISO}, {VCT_FEAT_RATE2, VCT_MODE_CELLS}, {VCT_FEAT_RATE2, VCT_MODE_COMM},
    // pixel-emission planes
    {VCT_FEAT_EMISSION, VCT_MODE_VARIANT},
    // gloss classes
    {VCT_FEAT_GLOSS, VCT_MODE_VARIANT}, {VCT_FEAT_GLOSS, VCT_MODE_ANISO}, {VCT_FEAT_GLOSS, VCT_MODE_CELLS},
    // sky
    {VCT_FEAT_SKY, VCT_MODE_VARIANT}, {VCT_FEAT_SKY, VCT_MODE_ANISO}, {VCT_FEAT_SKY, VCT_MODE_CELLS},
    // local lights
    {VCT_FEAT_LIGHTS, VCT_MODE_VARIANT},
    // two frames in flight
    {VCT_FEAT_TWO_FRAMES, VCT_MODE_DEBUG}, {VCT_FEAT_TWO_FRAMES, VCT_MODE_VARIANT4}, {VCT_FEAT_TWO_FRAMES, VCT_MODE_STATS},
};

static bool listed(unsigned feature, unsigned mode) {
    for (const Pair& p : kMatrix)
        if (p.feature == feature && p.mode == mode) return true;
    return false;
}

int main() {
    static_assert(sizeof(kMatrix) / sizeof(kMatrix[0]) == 18, "18 pairs");
    // the bits are what the header's comments say: distinct single bits, as many as the counts
    unsigned all_f = 0, all_m = 0;
    for (const Pair& p : kMatrix) { all_f |= p.feature; all_m |= p.mode; }
    if (all_f != (1u << VCT_FEAT_COUNT) - 1u || all_m != (1u << VCT_MODE_COUNT) - 1u) { printf("bits: %x %x\n", all_f, all_m); return 1; }
    long cases = 0, refused = 0;
    for (unsigned f = 0; f < (1u << VCT_FEAT_COUNT); ++f)
        for (unsigned m = 0; m < (1u << VCT_MODE_COUNT); ++m) {
            bool want = false;
            for (const Pair& p : kMatrix) want = want || ((f & p.feature) && (m & p.mode));
            const VctConflict got = vct_rule_conflict(f, m);
            ++cases;
            if ((bool)got != want) { printf("features %02x modes %02x: conflict %d, the matrix says %d\n", f, m, (int)(bool)got, (int)want); return 1; }
            if (!got) {
                if (got.feature || got.mode) { printf("features %02x modes %02x: no conflict but a pair\n", f, m); return 1; }
                continue;
            }
            ++refused;
            // the reported pair: one bit each, both present, and a pair of the matrix
            const bool one_bit = !(got.feature & (got.feature - 1u)) && got.mode && !(got.mode & (got.mode - 1u));
            if (!one_bit || !(f & got.feature) || !(m & got.mode) || !listed(got.feature, got.mode)) {
                printf("features %02x modes %02x: reported pair %x / %x\n", f, m, got.feature, got.mode);
                return 1;
            }
            // ... and it has words: a name on both sides, a lifting call at least on the feature's
            const VctRuleText& ft = kVctFeatureText[vct_rule_bit_index(got.feature)];
            const VctRuleText& mt = kVctModeText[vct_rule_bit_index(got.mode)];
            if (!ft.name || !ft.name[0] || !ft.lift || !ft.lift[0] || !mt.name || !mt.name[0]) { printf("pair %x / %x: no words\n", got.feature, got.mode); return 1; }
        }
    printf("feature_rules_check ok: %ld cases, %ld refused\n", cases, refused);
    return 0;
}
