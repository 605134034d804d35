// Host-only driver of csrc/vct_emission_check.h -- the table check of vct_upload_emission and the padding to the
// voxelizer's colour-table stride -- for a run under -fsanitize=address,undefined (tests/test_emission_restatement.py).
// No GPU call.
#include <limits.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_emission_check.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float denorm = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
    size_t bad = 99;
    // exactly-sized heap tables: a read past nmat * 3 floats is an ASan report
    for (int32_t nmat : {1, 2, 5, 64}) {
        std::vector<float> t((size_t)nmat * 3, 0.0f);
        EXPECT(vct_emission_check(t.data(), nmat, &bad) == VCT_EMISSION_ZERO);
        t[(size_t)nmat * 3 - 1] = -0.0f;
        EXPECT(vct_emission_check(t.data(), nmat, &bad) == VCT_EMISSION_ZERO);      // -0 is not below 0
        t[(size_t)nmat * 3 - 1] = denorm;
        EXPECT(vct_emission_check(t.data(), nmat, &bad) == VCT_EMISSION_OK);
        t[0] = big;
        EXPECT(vct_emission_check(t.data(), nmat, nullptr) == VCT_EMISSION_OK);
        for (float v : {nan, -nan, inf, -inf, -denorm, -1.0f}) {
            for (size_t at : {(size_t)0, (size_t)nmat * 3 - 1}) {
                std::vector<float> u = t;
                u[at] = v;
                bad = 99;
                EXPECT(vct_emission_check(u.data(), nmat, &bad) == VCT_EMISSION_BAD);
                EXPECT(bad == at);
                EXPECT(vct_emission_check(u.data(), nmat, nullptr) == VCT_EMISSION_BAD);
            }
        }
        std::vector<float> src((size_t)nmat * 3), out((size_t)nmat * 4, -7.0f);
        for (size_t i = 0; i < src.size(); ++i) src[i] = (float)(i + 1);
        vct_emission_pad(src.data(), nmat, out.data());
        for (int32_t m = 0; m < nmat; ++m) {
            for (int k = 0; k < 3; ++k) EXPECT(out[(size_t)m * 4 + k] == src[(size_t)m * 3 + k]);
            EXPECT(out[(size_t)m * 4 + 3] == 0.0f);
        }
    }
    EXPECT(vct_emission_check(nullptr, 0, &bad) == VCT_EMISSION_ZERO);
    EXPECT(vct_emission_check(nullptr, -3, &bad) == VCT_EMISSION_ZERO);
    EXPECT(vct_emission_check(nullptr, INT32_MIN, &bad) == VCT_EMISSION_ZERO);
    if (failures) return 1;
    printf("emission_check ok\n");
    return 0;
}
