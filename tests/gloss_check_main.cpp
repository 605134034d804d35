// Host-only driver of csrc/vct_gloss_check.h -- the table check of vct_set_gloss_classes and the copy of
// vct_upload_material_gloss's map -- for a run under -fsanitize=address,undefined
// (tests/test_gloss_restatement.py).  No GPU call.
#include <limits.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_gloss_check.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float denorm = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
    int32_t bad = 99;
    // exactly-sized heap tables: a read past nclasses entries is an ASan report
    for (int32_t n = 1; n <= VCT_GLOSS_CLASSES_MAX; ++n) {
        std::vector<vct_gloss_class> t((size_t)n, vct_gloss_class{0.07f, 20.0f});
        EXPECT(vct_gloss_check_classes(t.data(), n, &bad) == VCT_GLOSS_OK);
        EXPECT(vct_gloss_check_classes(t.data(), n, nullptr) == VCT_GLOSS_OK);
        t[(size_t)n - 1] = vct_gloss_class{denorm, 0.0f};          // the smallest aperture above 0, shininess +0
        EXPECT(vct_gloss_check_classes(t.data(), n, &bad) == VCT_GLOSS_OK);
        t[(size_t)n - 1] = vct_gloss_class{big, -0.0f};            // -0 is not below 0
        EXPECT(vct_gloss_check_classes(t.data(), n, &bad) == VCT_GLOSS_OK);
        t[0] = vct_gloss_class{1.0f, big};
        EXPECT(vct_gloss_check_classes(t.data(), n, &bad) == VCT_GLOSS_OK);
        for (size_t at : {(size_t)0, (size_t)n - 1}) {
            for (float v : {nan, -nan, inf, -inf, -denorm, -1.0f, 0.0f, -0.0f}) {       // tan_specular: finite and > 0
                std::vector<vct_gloss_class> u = t;
                u[at].tan_specular = v;
                bad = 99;
                EXPECT(vct_gloss_check_classes(u.data(), n, &bad) == VCT_GLOSS_BAD_VALUE);
                EXPECT(bad == (int32_t)at);
                EXPECT(vct_gloss_check_classes(u.data(), n, nullptr) == VCT_GLOSS_BAD_VALUE);
            }
            for (float v : {nan, -nan, inf, -inf, -denorm, -1.0f}) {                    // shininess: finite and >= 0
                std::vector<vct_gloss_class> u = t;
                u[at].shininess = v;
                bad = 99;
                EXPECT(vct_gloss_check_classes(u.data(), n, &bad) == VCT_GLOSS_BAD_VALUE);
                EXPECT(bad == (int32_t)at);
            }
        }
    }
    // counts outside [1, 8]: nothing of the table is read (a one-entry table stands behind every count)
    std::vector<vct_gloss_class> one(1, vct_gloss_class{nan, nan});
    EXPECT(vct_gloss_check_classes(one.data(), 0, &bad) == VCT_GLOSS_DETACH);
    EXPECT(vct_gloss_check_classes(nullptr, 3, &bad) == VCT_GLOSS_DETACH);
    EXPECT(vct_gloss_check_classes(nullptr, 0, nullptr) == VCT_GLOSS_DETACH);
    for (int32_t n : {9, 10, 255, INT32_MAX, -1, -8, INT32_MIN})
        EXPECT(vct_gloss_check_classes(one.data(), n, &bad) == VCT_GLOSS_BAD_COUNT);
    // the material map: exactly nmat bytes in, exactly nmat bytes out
    for (int32_t nmat : {1, 2, 5, 64, 300}) {
        std::vector<uint8_t> src((size_t)nmat), out((size_t)nmat, 0xee);
        for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(i * 37u + 3u);
        vct_gloss_map_copy(src.data(), nmat, out.data());
        EXPECT(out == src);                                        // stored as given, the clamp is the reader's
        EXPECT(vct_gloss_map_bytes(nmat) == (size_t)nmat);
    }
    EXPECT(vct_gloss_map_bytes(0) == 0 && vct_gloss_map_bytes(-3) == 0 && vct_gloss_map_bytes(INT32_MIN) == 0);
    vct_gloss_map_copy(nullptr, 0, nullptr);                       // a map without values: nothing is touched
    vct_gloss_map_copy(nullptr, INT32_MIN, nullptr);
    if (failures) return 1;
    printf("gloss_check ok\n");
    return 0;
}
