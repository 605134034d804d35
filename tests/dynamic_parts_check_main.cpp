// Host-only driver of what the dynamic mesh's parts add to csrc/vct_dynamic_check.h -- the argument checks of
// vct_set_dynamic_parts and vct_update_dynamic_transforms and the size arithmetic of the rest copy, the part indices and
// the matrix table -- for a run under -fsanitize=address,undefined (tests/test_dynamic_parts_host.py).  No GPU call.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_dynamic_check.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    int32_t bad = 7;
    EXPECT(VCT_DYNAMIC_PARTS_MAX == (1 << 16));
    // accepted: exactly ntri indices are read (ASan would see one more); parts need not be contiguous, a part may be empty
    {
        std::vector<int32_t> part = {3, 0, 2, 0, 1, 2, 0};
        EXPECT(!vct_dynamic_check_parts(true, part.data(), (int32_t)part.size(), 5, &bad) && bad == -1);
        EXPECT(!vct_dynamic_check_parts(true, part.data(), (int32_t)part.size(), 4, &bad) && bad == -1);
        EXPECT(!vct_dynamic_check_parts(true, part.data(), (int32_t)part.size(), VCT_DYNAMIC_PARTS_MAX, &bad));
        std::vector<int32_t> one = {0};
        EXPECT(!vct_dynamic_check_parts(true, one.data(), 1, 1, &bad));
        std::vector<int32_t> top(1000, VCT_DYNAMIC_PARTS_MAX - 1);
        EXPECT(!vct_dynamic_check_parts(true, top.data(), 1000, VCT_DYNAMIC_PARTS_MAX, &bad));
    }
    // no mesh: refused whatever else is given, and the indices are not read (a dangling pointer would trip ASan)
    {
        const char* why = vct_dynamic_check_parts(false, reinterpret_cast<const int32_t*>(8), 1000, 5, &bad);
        EXPECT(why && strstr(why, "no dynamic mesh") && bad == -1);
        why = vct_dynamic_check_parts(false, nullptr, 0, 0, &bad);
        EXPECT(why && strstr(why, "no dynamic mesh"));
        why = vct_dynamic_check_parts(true, reinterpret_cast<const int32_t*>(8), 0, 5, &bad);       // (attached means ntri >= 1)
        EXPECT(why && strstr(why, "no dynamic mesh"));
    }
    // nparts outside 1 .. VCT_DYNAMIC_PARTS_MAX: refused before an index is read; a NULL array with nparts > 0
    {
        for (int32_t n : {0, -1, INT32_MIN, VCT_DYNAMIC_PARTS_MAX + 1, INT32_MAX}) {
            const char* why = vct_dynamic_check_parts(true, reinterpret_cast<const int32_t*>(8), 1000, n, &bad);
            EXPECT(why && strstr(why, "nparts") && bad == -1);
        }
        const char* why = vct_dynamic_check_parts(true, nullptr, 1000, 5, &bad);
        EXPECT(why && strstr(why, "null") && bad == -1);
    }
    // an index outside 0 .. nparts-1 at every place: refused, and the triangle named; the first of two is the one named
    for (int32_t ntri : {1, 7, 300})
        for (int32_t at = 0; at < ntri; ++at)
            for (int32_t v : {5, -1, INT32_MIN, INT32_MAX, VCT_DYNAMIC_PARTS_MAX}) {
                std::vector<int32_t> part((size_t)ntri, 4);
                part[(size_t)at] = v;
                bad = -1;
                const char* why = vct_dynamic_check_parts(true, part.data(), ntri, 5, &bad);
                EXPECT(why && strstr(why, "out of range") && bad == at);
            }
    {
        std::vector<int32_t> part = {0, 1, 9, 0, -3};
        EXPECT(vct_dynamic_check_parts(true, part.data(), 5, 2, &bad) && bad == 2);
    }

    // vct_update_dynamic_transforms: the matrices themselves are never read
    {
        alignas(16) float m[16] = {};
        EXPECT(!vct_dynamic_check_transforms(true, 1, m, VCT_MEM_HOST));
        EXPECT(!vct_dynamic_check_transforms(true, VCT_DYNAMIC_PARTS_MAX, m, VCT_MEM_DEVICE));
        EXPECT(!vct_dynamic_check_transforms(true, 5, m + 1, VCT_MEM_HOST));                   // 4 bytes off a 16-byte boundary
        EXPECT(!vct_dynamic_check_transforms(true, 5, reinterpret_cast<const float*>(0x1004), VCT_MEM_DEVICE));
        const char* why = vct_dynamic_check_transforms(false, 5, m, VCT_MEM_HOST);
        EXPECT(why && strstr(why, "no dynamic mesh"));
        why = vct_dynamic_check_transforms(true, 0, m, VCT_MEM_HOST);
        EXPECT(why && strstr(why, "no parts"));
        why = vct_dynamic_check_transforms(true, 5, nullptr, VCT_MEM_HOST);
        EXPECT(why && strstr(why, "null"));
        for (int32_t loc : {-1, 2, 7, INT32_MAX, INT32_MIN}) {
            why = vct_dynamic_check_transforms(true, 5, m, loc);
            EXPECT(why && strstr(why, "location"));
        }
        for (uintptr_t off : {1u, 2u, 3u}) {
            why = vct_dynamic_check_transforms(true, 5, reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(m) + off), VCT_MEM_HOST);
            EXPECT(why && strstr(why, "alignment"));
        }
    }

    // sizes: 36 bytes per triangle of rest positions, 4 per index, 48 per matrix
    {
        const VctDynamicPartsSizes s = vct_dynamic_parts_sizes(150, 5);
        EXPECT(s.ok && s.rest == 150u * 36u && s.part == 150u * 4u && s.table == 5u * 48u);
        const VctDynamicSizes l = vct_dynamic_sizes(150, 3, 64, 64, true);
        EXPECT(l.ok && s.rest == l.pos && s.part == l.material);
        std::vector<float> table(s.table / sizeof(float));
        table[12 * 4 + 11] = 1.0f;                                                       // the last float of the last matrix
        EXPECT(table.size() == 60u && s.table % 16u == 0u);
        const VctDynamicPartsSizes top = vct_dynamic_parts_sizes(1 << 20, 1 << 16);      // the largest mesh, the most parts
        EXPECT(top.ok && top.rest == ((size_t)36 << 20) && top.part == ((size_t)4 << 20) && top.table == ((size_t)48 << 16));
        EXPECT(VCT_DYNAMIC_TRIS_MAX == (1 << 20) && vct_dynamic_parts_sizes(VCT_DYNAMIC_TRIS_MAX, VCT_DYNAMIC_PARTS_MAX).ok);
        const VctDynamicPartsSizes least = vct_dynamic_parts_sizes(1, 1);
        EXPECT(least.ok && least.rest == 36u && least.part == 4u && least.table == 48u);
    }
    // the overflow paths: an argument out of range gives nothing, whatever the other is
    for (const VctDynamicPartsSizes& s : {vct_dynamic_parts_sizes(0, 5), vct_dynamic_parts_sizes(-1, 5), vct_dynamic_parts_sizes(INT32_MIN, 5),
                                          vct_dynamic_parts_sizes((1 << 20) + 1, 5), vct_dynamic_parts_sizes(INT32_MAX, 5),
                                          vct_dynamic_parts_sizes(150, 0), vct_dynamic_parts_sizes(150, -1), vct_dynamic_parts_sizes(150, INT32_MIN),
                                          vct_dynamic_parts_sizes(150, (1 << 16) + 1), vct_dynamic_parts_sizes(150, INT32_MAX),
                                          vct_dynamic_parts_sizes(INT32_MAX, INT32_MAX)})
        EXPECT(!s.ok && s.rest == 0u && s.part == 0u && s.table == 0u);
    if (failures) { printf("dynamic_parts_check: %d failures\n", failures); return 1; }
    printf("dynamic_parts_check ok\n");
    return 0;
}
