// vct_dynamic_check.h -- argument checks, the default-capacity rule and the buffer-size arithmetic of the dynamic mesh
// (vct_api_dynamic.hip), free of any HIP call so that a host program can run them under the sanitizers
// (tests/dynamic_check_main.cpp).
#ifndef VCT_DYNAMIC_CHECK_H_
#define VCT_DYNAMIC_CHECK_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/vct.h"
#include "vct_emission_check.h"

#define VCT_DYNAMIC_MIN_BRICKS 64

// What is wrong with the arguments of an attaching vct_set_dynamic_mesh (pos != NULL and ntri != 0), or null.
static inline const char* vct_dynamic_check_args(const float* pos, const int32_t* material, int32_t ntri, const float* albedo,
                                                 int32_t nmat, int32_t max_bricks) {
    if (!pos) return "null positions";
    if (ntri < 1 || ntri > VCT_DYNAMIC_TRIS_MAX) return "ntri outside 1 .. VCT_DYNAMIC_TRIS_MAX";
    if (!material) return "null material indices";
    if (!albedo) return "null albedo table";
    if (nmat < 1) return "nmat < 1";
    if (max_bricks < 0) return "max_bricks < 0";
    for (int32_t i = 0; i < ntri; ++i)
        if (material[i] < 0 || material[i] >= nmat) return "material index out of range";
    return nullptr;
}

// What is wrong with the arguments of vct_update_dynamic_positions, or null.
static inline const char* vct_dynamic_check_update(bool attached, const float* pos, int32_t location) {
    if (!attached) return "no dynamic mesh attached";
    if (!pos) return "null positions";
    if (location != VCT_MEM_HOST && location != VCT_MEM_DEVICE) return "location is neither VCT_MEM_HOST nor VCT_MEM_DEVICE";
    if ((uintptr_t)pos & 3u) return "positions need 4-byte alignment";
    return nullptr;
}

// What is wrong with the arguments of an attaching vct_set_dynamic_parts (the detaching form is part == NULL with
// nparts == 0), or null.  A part index outside 0 .. nparts-1: *bad_tri is its triangle, else -1.
static inline const char* vct_dynamic_check_parts(bool attached, const int32_t* part, int32_t ntri, int32_t nparts, int32_t* bad_tri) {
    *bad_tri = -1;
    if (!attached || ntri < 1) return "no dynamic mesh attached";
    if (nparts < 1 || nparts > VCT_DYNAMIC_PARTS_MAX) return "nparts outside 1 .. VCT_DYNAMIC_PARTS_MAX";
    if (!part) return "null part indices";
    for (int32_t i = 0; i < ntri; ++i)
        if (part[i] < 0 || part[i] >= nparts) { *bad_tri = i; return "part index out of range"; }
    return nullptr;
}

// What is wrong with the arguments of vct_update_dynamic_transforms, or null; nparts is the count of matrices the attached
// mover takes, its parts or its bones.  The matrices themselves are not looked at: a device pointer cannot be, and the
// rule is the same for both locations.
static inline const char* vct_dynamic_check_transforms(bool attached, int32_t nparts, const float* m, int32_t location) {
    if (!attached) return "no dynamic mesh attached";
    if (nparts < 1) return "no parts and no skin attached (vct_set_dynamic_parts, vct_set_dynamic_skin)";
    if (!m) return "null matrices";
    if (location != VCT_MEM_HOST && location != VCT_MEM_DEVICE) return "location is neither VCT_MEM_HOST nor VCT_MEM_DEVICE";
    if ((uintptr_t)m & 3u) return "matrices need 4-byte alignment";
    return nullptr;
}

// Byte counts of what the parts add to the layer: the rest copy [ntri][9] fp32, the part indices [ntri] int32 and the
// matrix table [nparts][12] fp32.  ok == false: an argument out of range, or a count does not fit size_t.
struct VctDynamicPartsSizes {
    bool ok;
    size_t rest, part, table;
};
static inline VctDynamicPartsSizes vct_dynamic_parts_sizes(int32_t ntri, int32_t nparts) {
    VctDynamicPartsSizes s = {};
    if (ntri < 1 || ntri > VCT_DYNAMIC_TRIS_MAX || nparts < 1 || nparts > VCT_DYNAMIC_PARTS_MAX) return s;
    bool ok = !__builtin_mul_overflow((size_t)ntri, 9 * sizeof(float), &s.rest);
    ok = ok && !__builtin_mul_overflow((size_t)ntri, sizeof(int32_t), &s.part);
    ok = ok && !__builtin_mul_overflow((size_t)nparts, 12 * sizeof(float), &s.table);
    s.ok = ok;
    if (!ok) { const VctDynamicPartsSizes none = {}; return none; }
    return s;
}

static inline bool vct_dynamic_finite(float v) { return v == v && v - v == 0.0f; }

// What is wrong with the arguments of an attaching vct_set_dynamic_skin (the detaching form is bone == NULL and weight ==
// NULL with nbones == 0), or null.  bone and weight are [ntri][3][4]: per triangle corner four bone indices in 0 ..
// nbones-1 and four finite weights.  A bone index out of range or a weight that is NaN or infinite: *bad is its index in
// the array (triangle = index / 12, corner = index / 4 % 3, slot = index % 4), else (size_t)-1.
static inline const char* vct_dynamic_check_skin(bool attached, const int32_t* bone, const float* weight, int32_t ntri, int32_t nbones,
                                                 size_t* bad) {
    *bad = (size_t)-1;
    if (!attached || ntri < 1) return "no dynamic mesh attached";
    if (nbones < 1 || nbones > VCT_DYNAMIC_BONES_MAX) return "nbones outside 1 .. VCT_DYNAMIC_BONES_MAX";
    if (!bone) return "null bone indices";
    if (!weight) return "null weights";
    const size_t n = (size_t)ntri * 12;       // ntri <= 2^20 wherever `attached` is true: no overflow
    for (size_t i = 0; i < n; ++i)
        if (bone[i] < 0 || bone[i] >= nbones) { *bad = i; return "bone index out of range"; }
    for (size_t i = 0; i < n; ++i)
        if (!vct_dynamic_finite(weight[i])) { *bad = i; return "weight not finite"; }
    return nullptr;
}

// Byte counts of what a skin adds to the layer: the rest copy [ntri][9] fp32, the bone indices [ntri][12] packed as
// uint16 (nbones <= 2^16), the weights [ntri][12] fp32 and the matrix table [nbones][12] fp32.  ok == false: an argument
// out of range, or a count does not fit size_t.
struct VctDynamicSkinSizes {
    bool ok;
    size_t rest, bone, weight, table;
};
static inline VctDynamicSkinSizes vct_dynamic_skin_sizes(int32_t ntri, int32_t nbones) {
    VctDynamicSkinSizes s = {};
    if (ntri < 1 || ntri > VCT_DYNAMIC_TRIS_MAX || nbones < 1 || nbones > VCT_DYNAMIC_BONES_MAX) return s;
    bool ok = !__builtin_mul_overflow((size_t)ntri, 9 * sizeof(float), &s.rest);
    ok = ok && !__builtin_mul_overflow((size_t)ntri, 12 * sizeof(uint16_t), &s.bone);
    ok = ok && !__builtin_mul_overflow((size_t)ntri, 12 * sizeof(float), &s.weight);
    ok = ok && !__builtin_mul_overflow((size_t)nbones, 12 * sizeof(float), &s.table);
    s.ok = ok;
    if (!ok) { const VctDynamicSkinSizes none = {}; return none; }
    return s;
}

// What is wrong with the arguments of an attaching vct_set_dynamic_normals (nrm == NULL detaches), or null.  The values
// are not looked at: any fp32 value is accepted, and the accept test on the device decides corner by corner.
static inline const char* vct_dynamic_check_normals(bool attached, int32_t ntri) {
    if (!attached || ntri < 1) return "no dynamic mesh attached";
    return nullptr;
}

// What is wrong with the arguments of vct_update_dynamic_normals, or null.
static inline const char* vct_dynamic_check_normals_update(bool attached, bool normals, const float* nrm, int32_t location) {
    if (!attached) return "no dynamic mesh attached";
    if (!normals) return "no normals attached (vct_set_dynamic_normals)";
    if (!nrm) return "null normals";
    if (location != VCT_MEM_HOST && location != VCT_MEM_DEVICE) return "location is neither VCT_MEM_HOST nor VCT_MEM_DEVICE";
    if ((uintptr_t)nrm & 3u) return "normals need 4-byte alignment";
    return nullptr;
}

// What is wrong with a vct_download_dynamic_frames, or null: the frame arrays exist while a draw flag is on for an
// attached mesh.
static inline const char* vct_dynamic_check_frames(bool attached, int32_t draw_flags, bool arrays) {
    if (!attached) return "no dynamic mesh attached";
    if (!draw_flags || !arrays) return "no draw flag is on (vct_set_dynamic_draw): the frame arrays do not exist";
    return nullptr;
}

// Bytes of the corner normals [ntri][3][3] fp32; 0: ntri out of range (ntri <= 2^20: no overflow).
static inline size_t vct_dynamic_normals_bytes(int32_t ntri) {
    return ntri < 1 || ntri > VCT_DYNAMIC_TRIS_MAX ? 0 : (size_t)ntri * 9 * sizeof(float);
}

// What is wrong with the arguments of vct_set_dynamic_draw, or null.  specular null: the constant is 0, 0, 0.
#define VCT_DYNAMIC_DRAW_ALL (VCT_DYNAMIC_DRAW_SHADOW | VCT_DYNAMIC_DRAW_GBUFFER)
static inline const char* vct_dynamic_check_draw(int32_t flags, const float* specular) {
    if (flags & ~(int32_t)VCT_DYNAMIC_DRAW_ALL) return "unknown flag bits";
    if (specular)
        for (int k = 0; k < 3; ++k)
            if (!vct_dynamic_finite(specular[k])) return "non-finite specular value";
    return nullptr;
}

// 8^3 bricks of a grid of V^3 voxels (V a power of two, 8 .. 1024: at most 2^21)
static inline uint32_t vct_dynamic_grid_bricks(int32_t V) {
    if (V < 8) return 0u;
    const uint64_t b = (uint64_t)(V / 8);
    return (uint32_t)(b * b * b);
}

// What is wrong with the argument of vct_set_dynamic_bounce, or null.
static inline const char* vct_dynamic_check_bounce(int32_t on) { return on == 0 || on == 1 ? nullptr : "the switch is 0 or 1"; }

// Bytes of the bounce's brick -> resolved-slot table, [grid bricks] uint32; 0: no grid, or the count does not fit size_t.
static inline size_t vct_dynamic_bounce_map_bytes(int32_t V) {
    size_t bytes = 0;
    if (__builtin_mul_overflow((size_t)vct_dynamic_grid_bricks(V), sizeof(uint32_t), &bytes)) return 0;
    return bytes;
}

// Slots the bounce's list kernel is sized for: the static slots and, behind them, the layer's.  Both are at most the
// grid's bricks (2^21); the sum saturates all the same.
static inline uint32_t vct_dynamic_bounce_list_slots(uint32_t static_slots, uint32_t max_bricks) {
    const uint64_t n = (uint64_t)static_slots + (uint64_t)max_bricks;
    return n > 0xffffffffull ? 0xffffffffu : (uint32_t)n;
}

// What vct_set_dynamic_emission does with a table [nmat][3] for the attached mesh: VCT_EMISSION_OK attaches it,
// VCT_EMISSION_ZERO (null, or every value zero) detaches, VCT_EMISSION_BAD refuses -- *why says what is wrong, and for a
// value that is NaN, infinite or below 0 *bad_index is its index (material = index / 3, channel = index % 3), else
// (size_t)-1.  The table check itself is vct_upload_emission's (vct_emission_check.h).
static inline int vct_dynamic_check_emission(bool attached, const float* emission, int32_t nmat, size_t* bad_index, const char** why) {
    *bad_index = (size_t)-1;
    *why = nullptr;
    if (!attached || nmat < 1) { *why = "no dynamic mesh attached"; return VCT_EMISSION_BAD; }
    if (!emission) return VCT_EMISSION_ZERO;
    const int verdict = vct_emission_check(emission, nmat, bad_index);
    if (verdict == VCT_EMISSION_BAD) *why = "a value is not finite or below 0";
    return verdict;
}

// Byte counts of what the table adds to the layer: the padded table [nmat][4] fp32 and the emission sums
// [slots][512][2] uint64 -- 8 KiB per brick slot.  ok == false: a count does not fit size_t (nothing is allocated).
struct VctDynamicEmissionSizes {
    bool ok;
    size_t table, sums;
};
static inline VctDynamicEmissionSizes vct_dynamic_emission_sizes(int32_t nmat, uint32_t slots) {
    VctDynamicEmissionSizes s = {};
    if (nmat < 1) return s;
    bool ok = !__builtin_mul_overflow((size_t)nmat, 4 * sizeof(float), &s.table);
    ok = ok && !__builtin_mul_overflow((size_t)slots, (size_t)512 * 2 * sizeof(uint64_t), &s.sums);
    s.ok = ok;
    if (!ok) { const VctDynamicEmissionSizes none = {}; return none; }
    return s;
}

// Brick slots of the dynamic layer.  asked > 0: as asked; asked == 0: twice the bricks the attached positions touch, at
// least VCT_DYNAMIC_MIN_BRICKS.  Either way no more than the grid has: more can never be used.
static inline uint32_t vct_dynamic_capacity(int32_t asked, uint32_t touched, uint32_t grid_bricks) {
    uint64_t want;
    if (asked > 0) want = (uint64_t)asked;
    else {
        want = 2ull * (uint64_t)touched;
        if (want < VCT_DYNAMIC_MIN_BRICKS) want = VCT_DYNAMIC_MIN_BRICKS;
    }
    if (want > grid_bricks) want = grid_bricks;
    return (uint32_t)want;
}

// Byte counts of every buffer of the dynamic layer.  ok == false: a count does not fit size_t (nothing is allocated).
struct VctDynamicSizes {
    bool ok;
    size_t pos, material, albedo;       // [ntri][9] fp32, [ntri] int32, [nmat][4] fp32
    size_t big_list;                    // [ntri] int32
    size_t brick_slot;                  // [grid_bricks] uint32
    size_t slot_list;                   // [slots] uint32 (two of them: claimed, resolved)
    size_t acc, acc_attr;               // [slots][512][2] / [slots][512][3] uint64 (acc_attr 0 without voxel attributes)
    size_t pool;                        // [slots][512] uint32 (radiance; with attributes also albedo and normal)
    size_t words;                       // the counters and the two sets of statistics
    size_t volume;                      // V^3 * 4: the dense staging of a download
};
static inline bool vct_dynamic_mul(size_t a, size_t b, size_t* out) { return !__builtin_mul_overflow(a, b, out); }
static inline VctDynamicSizes vct_dynamic_sizes(int32_t ntri, int32_t nmat, uint32_t slots, int32_t V, bool attributes) {
    VctDynamicSizes s = {};
    if (ntri < 1 || ntri > VCT_DYNAMIC_TRIS_MAX || nmat < 1 || V < 8) return s;
    const size_t nt = (size_t)ntri, nm = (size_t)nmat, ns = (size_t)slots, nb = (size_t)vct_dynamic_grid_bricks(V);
    size_t vox = 0;
    bool ok = vct_dynamic_mul(nt, 9 * sizeof(float), &s.pos);
    ok = ok && vct_dynamic_mul(nt, sizeof(int32_t), &s.material);
    ok = ok && vct_dynamic_mul(nm, 4 * sizeof(float), &s.albedo);
    ok = ok && vct_dynamic_mul(nt, sizeof(int32_t), &s.big_list);
    ok = ok && vct_dynamic_mul(nb, sizeof(uint32_t), &s.brick_slot);
    ok = ok && vct_dynamic_mul(ns, sizeof(uint32_t), &s.slot_list);
    ok = ok && vct_dynamic_mul(ns, (size_t)512 * 2 * sizeof(uint64_t), &s.acc);
    if (attributes) ok = ok && vct_dynamic_mul(ns, (size_t)512 * 3 * sizeof(uint64_t), &s.acc_attr);
    ok = ok && vct_dynamic_mul(ns, (size_t)512 * sizeof(uint32_t), &s.pool);
    ok = ok && vct_dynamic_mul(nb, 512, &vox) && vct_dynamic_mul(vox, sizeof(uint32_t), &s.volume);
    s.words = 32 * sizeof(uint32_t);
    s.ok = ok;
    if (!ok) { const VctDynamicSizes none = {}; return none; }
    return s;
}

// floats of the draw copy and of each of the three frame arrays of a drawn layer, [ntri][9] (ntri <= 2^20: no overflow)
static inline size_t vct_dynamic_draw_floats(int32_t ntri) { return ntri < 1 ? 0 : (size_t)ntri * 9; }

// Byte counts of what drawing the layer adds: the four [ntri][9] arrays, and per raster target of w x h pixels (a frame
// slot, or the shadow map with w = h = its size) the direct form's scratch sized by the layer's triangles -- the two
// lists, the set-up records and the tile work items -- and, for a frame slot, the second visibility buffer.
struct VctDynamicDrawSizes {
    bool ok;
    size_t arrays;                      // draw copy + three frame arrays
    size_t lists, recs, items;          // [4 * ntri] int32, [2 * ntri] 96-byte records, [pixels / 16 + 4096] 8-byte items
    size_t vis;                         // [pixels] uint64 (frame slots only)
};
static inline VctDynamicDrawSizes vct_dynamic_draw_sizes(int32_t ntri, int32_t w, int32_t h) {
    VctDynamicDrawSizes s = {};
    if (ntri < 1 || ntri > VCT_DYNAMIC_TRIS_MAX || w < 1 || h < 1) return s;
    const size_t nt = (size_t)ntri;
    size_t pixels = 0, items = 0;
    bool ok = vct_dynamic_mul((size_t)w, (size_t)h, &pixels);
    ok = ok && vct_dynamic_mul(vct_dynamic_draw_floats(ntri), 4 * sizeof(float), &s.arrays);
    ok = ok && vct_dynamic_mul(nt, 4 * sizeof(int32_t), &s.lists);
    ok = ok && vct_dynamic_mul(nt, (size_t)2 * 96, &s.recs);
    ok = ok && !__builtin_add_overflow(pixels / 16, (size_t)4096, &items) && vct_dynamic_mul(items, 8, &s.items);
    ok = ok && vct_dynamic_mul(pixels, sizeof(uint64_t), &s.vis);
    s.ok = ok;
    if (!ok) { const VctDynamicDrawSizes none = {}; return none; }
    return s;
}

#endif
