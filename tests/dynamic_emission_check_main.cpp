// Host-only driver of what the dynamic mesh's emission adds to csrc/vct_dynamic_check.h -- the verdict of
// vct_set_dynamic_emission on a table and the size arithmetic of the table and the emission sums -- for a run under
// -fsanitize=address,undefined (tests/test_dynamic_emission_host.py).  No GPU call.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_dynamic_check.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const size_t none = (size_t)-1;
    size_t bad = 0;
    const char* why = nullptr;
    // exactly nmat * 3 floats are read (ASan would see one more)
    {
        std::vector<float> t = {0.9f, 0.35f, 0.1f, 0.0f, 0.0f, 0.0f, 0.25f, 2.0f, 0.6f};
        EXPECT(vct_dynamic_check_emission(true, t.data(), 3, &bad, &why) == VCT_EMISSION_OK && !why && bad == none);
        std::vector<float> one = {0.0f, 0.0f, 1.0e30f};
        EXPECT(vct_dynamic_check_emission(true, one.data(), 1, &bad, &why) == VCT_EMISSION_OK && !why);
        one[2] = std::numeric_limits<float>::denorm_min();
        EXPECT(vct_dynamic_check_emission(true, one.data(), 1, &bad, &why) == VCT_EMISSION_OK);
    }
    // NULL and all zero (either sign) detach
    {
        EXPECT(vct_dynamic_check_emission(true, nullptr, 3, &bad, &why) == VCT_EMISSION_ZERO && !why && bad == none);
        std::vector<float> z(9, 0.0f);
        z[4] = -0.0f;
        EXPECT(vct_dynamic_check_emission(true, z.data(), 3, &bad, &why) == VCT_EMISSION_ZERO && !why && bad == none);
    }
    // no mesh: refused whatever the table is, and the table is not read (a dangling pointer would trip ASan)
    {
        std::vector<float> t = {1.0f, 1.0f, 1.0f};
        bad = 7;
        EXPECT(vct_dynamic_check_emission(false, t.data(), 1, &bad, &why) == VCT_EMISSION_BAD && why && strstr(why, "no dynamic mesh") && bad == none);
        EXPECT(vct_dynamic_check_emission(false, nullptr, 0, &bad, &why) == VCT_EMISSION_BAD && why && bad == none);
        EXPECT(vct_dynamic_check_emission(false, reinterpret_cast<const float*>(8), 3, &bad, &why) == VCT_EMISSION_BAD && bad == none);
        EXPECT(vct_dynamic_check_emission(true, t.data(), 0, &bad, &why) == VCT_EMISSION_BAD && why && bad == none);
        EXPECT(vct_dynamic_check_emission(true, t.data(), INT32_MIN, &bad, &why) == VCT_EMISSION_BAD && why);
    }
    // a NaN, an infinity or a negative value at every place of the table: refused, and named
    for (int32_t nmat : {1, 3, 17})
        for (size_t at = 0; at < (size_t)nmat * 3; ++at)
            for (float v : {nan, -nan, inf, -inf, -1.0f, -std::numeric_limits<float>::denorm_min()}) {
                std::vector<float> t((size_t)nmat * 3, 0.5f);
                t[at] = v;
                bad = none; why = nullptr;
                EXPECT(vct_dynamic_check_emission(true, t.data(), nmat, &bad, &why) == VCT_EMISSION_BAD);
                EXPECT(bad == at && why && bad / 3 == at / 3 && bad % 3 == at % 3);
            }
    {   // the first of two bad values is the one named
        std::vector<float> t = {0.0f, 0.0f, 0.0f, 0.0f, nan, 0.0f, -1.0f, 0.0f, 0.0f};
        EXPECT(vct_dynamic_check_emission(true, t.data(), 3, &bad, &why) == VCT_EMISSION_BAD && bad == 4u);
    }

    // sizes: the padded table and 8 KiB of sums per brick slot
    {
        const VctDynamicEmissionSizes s = vct_dynamic_emission_sizes(3, 64);
        EXPECT(s.ok && s.table == 3u * 16u && s.sums == 64u * 8192u);
        std::vector<float> table(s.table / sizeof(float));
        const float em[9] = {0.9f, 0.35f, 0.1f, 0.0f, 0.0f, 0.0f, 0.25f, 2.0f, 0.6f};
        vct_emission_pad(em, 3, table.data());
        EXPECT(table[4 * 2 + 1] == 2.0f && table[4 * 2 + 3] == 0.0f && table[3] == 0.0f);
        std::vector<unsigned long long> sums(s.sums / sizeof(unsigned long long));
        sums[((size_t)63 * 512 + 511) * 2 + 1] = 1ull;             // the second word of the last voxel of the last slot
        EXPECT(sums.size() == (size_t)64 * 1024);
    }
    {
        const VctDynamicEmissionSizes s = vct_dynamic_emission_sizes(1, 0);      // (a layer always has slots; the arithmetic holds)
        EXPECT(s.ok && s.table == 16u && s.sums == 0u);
        const VctDynamicEmissionSizes g = vct_dynamic_emission_sizes(1, 1u << 21);      // every brick of a 1024^3 grid
        if (sizeof(size_t) >= 8) EXPECT(g.ok && g.sums == ((size_t)1 << 34));
        const VctDynamicEmissionSizes m = vct_dynamic_emission_sizes(INT32_MAX, 0xffffffffu);
        if (sizeof(size_t) >= 8) EXPECT(m.ok && m.table == (size_t)INT32_MAX * 16u && m.sums == (size_t)0xffffffffu * 8192u);
        // what the sums add to a slot: 8 KiB beside acc's 8 KiB
        const VctDynamicSizes l = vct_dynamic_sizes(150, 3, 64, 64, true);
        EXPECT(l.ok && vct_dynamic_emission_sizes(3, 64).sums == l.acc);
    }
    for (const VctDynamicEmissionSizes& s : {vct_dynamic_emission_sizes(0, 64), vct_dynamic_emission_sizes(-1, 64),
                                             vct_dynamic_emission_sizes(INT32_MIN, 0)})
        EXPECT(!s.ok && s.table == 0u && s.sums == 0u);
    // the bound that lets a channel's sum share a 64-bit word: 255 * 2^20 fragments stay below 2^32
    EXPECT(255ull * (1ull << 20) < (1ull << 32) && 255ull * (uint64_t)VCT_DYNAMIC_TRIS_MAX < (1ull << 32));
    if (failures) { printf("dynamic_emission_check: %d failures\n", failures); return 1; }
    printf("dynamic_emission_check ok\n");
    return 0;
}
