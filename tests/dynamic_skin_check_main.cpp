// Host-only driver of what the dynamic mesh's skin adds to csrc/vct_dynamic_check.h -- the argument check of
// vct_set_dynamic_skin and the size arithmetic of the rest copy, the packed bone indices, the weights and the matrix
// table -- and of the movers' rule of csrc/vct_feature_rules.h, for a run under -fsanitize=address,undefined
// (tests/test_dynamic_skin_host.py).  No GPU call.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_dynamic_check.h"
#include "../voxel-cone-tracing_amd/csrc/vct_feature_rules.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    size_t bad = 7;
    const size_t none = (size_t)-1;
    EXPECT(VCT_DYNAMIC_BONES_MAX == (1 << 16));
    const int32_t* dangling_i = reinterpret_cast<const int32_t*>(8);
    const float* dangling_f = reinterpret_cast<const float*>(8);
    // accepted: exactly ntri * 12 values of each array are read (ASan would see one more); weights are taken as given --
    // negative, zero, sums other than 1, denormals, the largest finite value
    {
        const int32_t ntri = 3;
        std::vector<int32_t> bone((size_t)ntri * 12, 0);
        std::vector<float> weight((size_t)ntri * 12, 0.25f);
        for (size_t i = 0; i < bone.size(); ++i) bone[i] = (int32_t)(i % 5);
        weight[0] = -0.5f; weight[1] = 0.0f; weight[2] = -0.0f; weight[3] = 3.0f; weight[4] = 1e-45f; weight[5] = 3.4028234e38f;
        weight[6] = -3.4028234e38f;
        EXPECT(!vct_dynamic_check_skin(true, bone.data(), weight.data(), ntri, 5, &bad) && bad == none);
        EXPECT(!vct_dynamic_check_skin(true, bone.data(), weight.data(), ntri, VCT_DYNAMIC_BONES_MAX, &bad) && bad == none);
        std::vector<int32_t> top(12, VCT_DYNAMIC_BONES_MAX - 1);                           // the last admissible index: 65535
        EXPECT(!vct_dynamic_check_skin(true, top.data(), weight.data(), 1, VCT_DYNAMIC_BONES_MAX, &bad) && bad == none);
        EXPECT((uint16_t)top[0] == 65535u && (int32_t)(uint16_t)top[0] == top[0]);         // ... and it survives the packing
        std::vector<int32_t> zero(12, 0);
        EXPECT(!vct_dynamic_check_skin(true, zero.data(), weight.data(), 1, 1, &bad));
    }
    // no mesh: refused whatever else is given, and the arrays are not read (a dangling pointer would trip ASan)
    {
        const char* why = vct_dynamic_check_skin(false, dangling_i, dangling_f, 1000, 5, &bad);
        EXPECT(why && strstr(why, "no dynamic mesh") && bad == none);
        why = vct_dynamic_check_skin(false, nullptr, nullptr, 0, 0, &bad);
        EXPECT(why && strstr(why, "no dynamic mesh"));
        why = vct_dynamic_check_skin(true, dangling_i, dangling_f, 0, 5, &bad);           // (attached means ntri >= 1)
        EXPECT(why && strstr(why, "no dynamic mesh"));
    }
    // nbones outside 1 .. VCT_DYNAMIC_BONES_MAX: refused before a value is read; a NULL array
    {
        for (int32_t n : {0, -1, INT32_MIN, VCT_DYNAMIC_BONES_MAX + 1, INT32_MAX}) {
            const char* why = vct_dynamic_check_skin(true, dangling_i, dangling_f, 1000, n, &bad);
            EXPECT(why && strstr(why, "nbones") && bad == none);
        }
        std::vector<int32_t> bone(12, 0);
        std::vector<float> weight(12, 0.25f);
        const char* why = vct_dynamic_check_skin(true, nullptr, weight.data(), 1, 5, &bad);
        EXPECT(why && strstr(why, "null bone") && bad == none);
        why = vct_dynamic_check_skin(true, bone.data(), nullptr, 1, 5, &bad);
        EXPECT(why && strstr(why, "null weights") && bad == none);
        why = vct_dynamic_check_skin(true, nullptr, nullptr, 1, 5, &bad);
        EXPECT(why && strstr(why, "null") && bad == none);
    }
    // a bone index outside 0 .. nbones-1 at every place: refused, and the place named as triangle, corner and slot
    for (int32_t ntri : {1, 7, 30})
        for (size_t at = 0; at < (size_t)ntri * 12; ++at)
            for (int32_t v : {5, -1, INT32_MIN, INT32_MAX, VCT_DYNAMIC_BONES_MAX}) {
                std::vector<int32_t> bone((size_t)ntri * 12, 4);
                std::vector<float> weight((size_t)ntri * 12, 0.25f);
                bone[at] = v;
                bad = none;
                const char* why = vct_dynamic_check_skin(true, bone.data(), weight.data(), ntri, 5, &bad);
                EXPECT(why && strstr(why, "bone index out of range") && bad == at);
                EXPECT(bad / 12 < (size_t)ntri && bad / 4 % 3 < 3 && (bad / 12) * 12 + (bad / 4 % 3) * 4 + bad % 4 == at);
            }
    // a weight that is NaN or infinite at every place: the same
    for (int32_t ntri : {1, 7, 30})
        for (size_t at = 0; at < (size_t)ntri * 12; ++at)
            for (float v : {NAN, -NAN, INFINITY, -INFINITY}) {
                std::vector<int32_t> bone((size_t)ntri * 12, 4);
                std::vector<float> weight((size_t)ntri * 12, 0.25f);
                weight[at] = v;
                bad = none;
                const char* why = vct_dynamic_check_skin(true, bone.data(), weight.data(), ntri, 5, &bad);
                EXPECT(why && strstr(why, "weight not finite") && bad == at);
            }
    {   // the first offender is the one named; a bad index is named before a bad weight
        std::vector<int32_t> bone(24, 0);
        std::vector<float> weight(24, 0.5f);
        bone[17] = 9; bone[20] = -3; weight[2] = NAN;
        EXPECT(vct_dynamic_check_skin(true, bone.data(), weight.data(), 2, 2, &bad) && bad == 17);
        bone[17] = 1; bone[20] = 1;
        EXPECT(vct_dynamic_check_skin(true, bone.data(), weight.data(), 2, 2, &bad) && bad == 2);
    }

    // sizes: 36 bytes per triangle of rest positions, 24 of packed indices, 48 of weights; 48 per matrix
    {
        const VctDynamicSkinSizes s = vct_dynamic_skin_sizes(150, 6);
        EXPECT(s.ok && s.rest == 150u * 36u && s.bone == 150u * 24u && s.weight == 150u * 48u && s.table == 6u * 48u);
        EXPECT(s.bone % 8u == 0u && s.weight % 16u == 0u && s.table % 16u == 0u);      // what the kernel's 8- and 16-byte loads need
        const VctDynamicPartsSizes p = vct_dynamic_parts_sizes(150, 6);
        EXPECT(p.ok && p.rest == s.rest && p.table == s.table);
        std::vector<uint16_t> packed(s.bone / sizeof(uint16_t));
        packed[149 * 12 + 11] = 65535u;                                                 // the last index of the last triangle
        EXPECT(packed.size() == 1800u);
        const VctDynamicSkinSizes top = vct_dynamic_skin_sizes(VCT_DYNAMIC_TRIS_MAX, VCT_DYNAMIC_BONES_MAX);
        EXPECT(top.ok && top.rest == ((size_t)36 << 20) && top.bone == ((size_t)24 << 20) && top.weight == ((size_t)48 << 20) &&
               top.table == ((size_t)48 << 16));
        const VctDynamicSkinSizes least = vct_dynamic_skin_sizes(1, 1);
        EXPECT(least.ok && least.rest == 36u && least.bone == 24u && least.weight == 48u && least.table == 48u);
    }
    // the overflow paths: an argument out of range gives nothing, whatever the other is
    for (const VctDynamicSkinSizes& s : {vct_dynamic_skin_sizes(0, 5), vct_dynamic_skin_sizes(-1, 5), vct_dynamic_skin_sizes(INT32_MIN, 5),
                                         vct_dynamic_skin_sizes((1 << 20) + 1, 5), vct_dynamic_skin_sizes(INT32_MAX, 5),
                                         vct_dynamic_skin_sizes(150, 0), vct_dynamic_skin_sizes(150, -1), vct_dynamic_skin_sizes(150, INT32_MIN),
                                         vct_dynamic_skin_sizes(150, (1 << 16) + 1), vct_dynamic_skin_sizes(150, INT32_MAX),
                                         vct_dynamic_skin_sizes(INT32_MAX, INT32_MAX)})
        EXPECT(!s.ok && s.rest == 0u && s.bone == 0u && s.weight == 0u && s.table == 0u);

    // vct_update_dynamic_transforms counts bones as it counts parts
    {
        alignas(16) float m[16] = {};
        EXPECT(!vct_dynamic_check_transforms(true, VCT_DYNAMIC_BONES_MAX, m + 1, VCT_MEM_HOST));
        const char* why = vct_dynamic_check_transforms(true, 0, m, VCT_MEM_HOST);
        EXPECT(why && strstr(why, "no skin"));
    }
    // the movers' rule: parts and a skin refuse each other, both ways; the same kind replaces itself; none refuses nothing
    EXPECT(vct_mover_conflict(VCT_MOVER_PARTS, VCT_MOVER_SKIN) == VCT_MOVER_PARTS);
    EXPECT(vct_mover_conflict(VCT_MOVER_SKIN, VCT_MOVER_PARTS) == VCT_MOVER_SKIN);
    for (VctMover m : {VCT_MOVER_NONE, VCT_MOVER_PARTS, VCT_MOVER_SKIN}) {
        EXPECT(vct_mover_conflict(m, m) == VCT_MOVER_NONE);
        EXPECT(vct_mover_conflict(VCT_MOVER_NONE, m) == VCT_MOVER_NONE && vct_mover_conflict(m, VCT_MOVER_NONE) == VCT_MOVER_NONE);
        EXPECT(kVctMoverText[m].name && (m == VCT_MOVER_NONE) == !kVctMoverText[m].lift);
    }
    if (failures) { printf("dynamic_skin_check: %d failures\n", failures); return 1; }
    printf("dynamic_skin_check ok\n");
    return 0;
}
