// vct_feature_rules.h -- which feature of a context goes with which mode: the matrix, as data (host only, no HIP).
//
// A FEATURE is something a caller attaches to a context; a MODE is a way the context traces that some features have no
// kernels for.  A pair of the matrix is refused wherever it could come about: by the feature's setter while the mode is
// in force, by the mode's setter while the feature is attached, and by the trace launch (vct_capi.hip vct_rules_in_force,
// vct_refuse_conflict).  Requirements that are no conflicts (lights need voxel attributes, ...) stay with their setters.
#ifndef VCT_FEATURE_RULES_H_
#define VCT_FEATURE_RULES_H_

enum VctFeature : unsigned {
    VCT_FEAT_MASK = 1u << 0,          // a lighting-component mask other than VCT_SHOW_ALL
    VCT_FEAT_AOV = 1u << 1,           // per-component outputs
    VCT_FEAT_RATE2 = 1u << 2,         // the half-rate diffuse gather
    VCT_FEAT_EMISSION = 1u << 3,      // pixel-emission planes on a frame slot (the material table's or the caller's)
    VCT_FEAT_GLOSS = 1u << 4,         // gloss classes
    VCT_FEAT_SKY = 1u << 5,           // sky light
    VCT_FEAT_LIGHTS = 1u << 6,        // local lights
    VCT_FEAT_TWO_FRAMES = 1u << 7,    // two frames in flight
    VCT_FEAT_COUNT = 8
};

enum VctMode : unsigned {
    VCT_MODE_VARIANT = 1u << 0,       // config.trace_variant != 0
    VCT_MODE_ANISO = 1u << 1,         // config.anisotropic_mips
    VCT_MODE_CELLS = 1u << 2,         // footprint records
    VCT_MODE_COMM = 1u << 3,          // an attached communicator: a rank of a multi-GPU frame
    VCT_MODE_DEBUG = 1u << 4,         // config.debug_outputs
    VCT_MODE_VARIANT4 = 1u << 5,      // config.trace_variant == 4 (per-context compaction scratch)
    VCT_MODE_STATS = 1u << 6,         // a VCT_STATS build (per-context statistics words)
    VCT_MODE_COUNT = 7
};

// the matrix: one row per feature, the modes it is refused with
struct VctFeatureRule { unsigned feature, modes; };
static const VctFeatureRule kVctFeatureRules[VCT_FEAT_COUNT] = {
    {VCT_FEAT_MASK, VCT_MODE_VARIANT},
    {VCT_FEAT_AOV, VCT_MODE_VARIANT | VCT_MODE_COMM},
    {VCT_FEAT_RATE2, VCT_MODE_VARIANT | VCT_MODE_ANISO | VCT_MODE_CELLS | VCT_MODE_COMM},
    {VCT_FEAT_EMISSION, VCT_MODE_VARIANT},
    {VCT_FEAT_GLOSS, VCT_MODE_VARIANT | VCT_MODE_ANISO | VCT_MODE_CELLS},
    {VCT_FEAT_SKY, VCT_MODE_VARIANT | VCT_MODE_ANISO | VCT_MODE_CELLS},
    {VCT_FEAT_LIGHTS, VCT_MODE_VARIANT},
    {VCT_FEAT_TWO_FRAMES, VCT_MODE_DEBUG | VCT_MODE_VARIANT4 | VCT_MODE_STATS},
};

// what a message calls a feature or a mode, and the call that lifts it (null: fixed when the context or the library is made)
struct VctRuleText { const char* name; const char* lift; };
static const VctRuleText kVctFeatureText[VCT_FEAT_COUNT] = {
    {"a lighting-component mask", "vct_set_lighting_components(ctx, VCT_SHOW_ALL)"},
    {"per-component outputs", "vct_set_aov_outputs(ctx, 0)"},
    {"the half-rate diffuse gather", "vct_set_diffuse_rate(ctx, 1)"},
    {"pixel-emission planes", "vct_upload_emission(ctx, NULL) and vct_set_pixel_emission(ctx, NULL, ...)"},
    {"gloss classes", "vct_set_gloss_classes(ctx, NULL, 0)"},
    {"sky light", "vct_set_sky(ctx, NULL)"},
    {"local lights", "vct_set_lights(ctx, NULL, 0)"},
    {"two frames in flight", "vct_set_frames_in_flight(ctx, 1)"},
};
static const VctRuleText kVctModeText[VCT_MODE_COUNT] = {
    {"config.trace_variant 1 .. 4", "vct_set_trace_variant(ctx, 0)"},
    {"config.anisotropic_mips", nullptr},
    {"footprint records", "vct_set_footprint_records(ctx, 0)"},
    {"a rank of a multi-GPU frame", "vct_comm_destroy(ctx)"},
    {"config.debug_outputs (per-context scratch)", nullptr},
    {"config.trace_variant 4 (per-context scratch)", "vct_set_trace_variant"},
    {"an instrumented build (VCT_STATS: per-context scratch)", nullptr},
};

// The first pair of the matrix among `features` x `modes`, as one bit each; {0, 0}: they go together.
struct VctConflict {
    unsigned feature, mode;
    explicit operator bool() const { return feature != 0u; }
};
static inline VctConflict vct_rule_conflict(unsigned features, unsigned modes) {
    for (const VctFeatureRule& r : kVctFeatureRules) {
        const unsigned hit = (features & r.feature) ? (modes & r.modes) : 0u;
        if (hit) return VctConflict{r.feature, hit & (0u - hit)};
    }
    return VctConflict{0u, 0u};
}
static inline int vct_rule_bit_index(unsigned bit) { return __builtin_ctz(bit); }

// The MOVERS of the dynamic mesh (include/vct.h "dynamic mesh", Parts and Skin): what turns the matrices of
// vct_update_dynamic_transforms into positions.  They share the matrix table and the call, so a mesh has at most one:
// the setter of one is refused while the other is attached.  (Outside the matrix above: no mode is involved.)
enum VctMover : unsigned { VCT_MOVER_NONE = 0, VCT_MOVER_PARTS = 1, VCT_MOVER_SKIN = 2, VCT_MOVER_COUNT = 3 };
static const VctRuleText kVctMoverText[VCT_MOVER_COUNT] = {
    {"no mover", nullptr},
    {"parts", "vct_set_dynamic_parts(ctx, NULL, 0)"},
    {"a skin", "vct_set_dynamic_skin(ctx, NULL, NULL, 0)"},
};
// The attached mover that refuses attaching `wanted`, or VCT_MOVER_NONE: they go together (nothing attached, or the same
// kind, which the attach replaces).
static inline VctMover vct_mover_conflict(VctMover attached, VctMover wanted) {
    return attached != VCT_MOVER_NONE && wanted != VCT_MOVER_NONE && attached != wanted ? attached : VCT_MOVER_NONE;
}

#endif
