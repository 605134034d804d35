// Host-only driver of what drawing the dynamic mesh adds to csrc/vct_dynamic_check.h -- the argument check of
// vct_set_dynamic_draw and the size arithmetic of the draw copy, the frames, the dynamic pass's raster scratch and the
// second visibility buffer -- for a run under -fsanitize=address,undefined (tests/test_dynamic_draw_host.py).  No GPU call.
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
    // the flags: the two bits in any combination, nothing else -- the sign bit and bit 2 included
    EXPECT(VCT_DYNAMIC_DRAW_SHADOW == 1 && VCT_DYNAMIC_DRAW_GBUFFER == 2 && VCT_DYNAMIC_DRAW_ALL == 3);
    for (int32_t f = 0; f <= 3; ++f) EXPECT(!vct_dynamic_check_draw(f, nullptr));
    EXPECT(vct_dynamic_check_draw(4, nullptr));
    EXPECT(vct_dynamic_check_draw(7, nullptr));
    EXPECT(vct_dynamic_check_draw(-1, nullptr));
    EXPECT(vct_dynamic_check_draw(INT32_MIN, nullptr));
    EXPECT(vct_dynamic_check_draw(INT32_MAX, nullptr));
    EXPECT(vct_dynamic_check_draw(INT32_MIN | 1, nullptr));
    // the constant: exactly three floats are read (ASan would see a fourth), every one finite
    {
        std::vector<float> sp = {0.25f, 0.0f, 1.0e30f};
        EXPECT(!vct_dynamic_check_draw(3, sp.data()));
        EXPECT(!vct_dynamic_check_draw(0, sp.data()));
        sp[2] = -0.0f;
        EXPECT(!vct_dynamic_check_draw(2, sp.data()));
        sp[1] = std::numeric_limits<float>::denorm_min();
        EXPECT(!vct_dynamic_check_draw(1, sp.data()));
        for (int k = 0; k < 3; ++k)
            for (float bad : {inf, -inf, nan, -nan}) {
                std::vector<float> q = {0.5f, 0.5f, 0.5f};
                q[k] = bad;
                EXPECT(vct_dynamic_check_draw(3, q.data()));
                EXPECT(vct_dynamic_check_draw(0, q.data()));      // refused even where nothing would be drawn
            }
        sp = {nan, 0.0f, 0.0f};
        EXPECT(vct_dynamic_check_draw(8, sp.data()));             // either reason refuses
    }
    EXPECT(vct_dynamic_finite(0.0f) && vct_dynamic_finite(-3.0e38f) && !vct_dynamic_finite(inf) && !vct_dynamic_finite(nan));

    // the four [ntri][9] arrays
    EXPECT(vct_dynamic_draw_floats(1) == 9u && vct_dynamic_draw_floats(150) == 1350u);
    EXPECT(vct_dynamic_draw_floats(0) == 0u && vct_dynamic_draw_floats(-5) == 0u && vct_dynamic_draw_floats(INT32_MIN) == 0u);
    EXPECT(vct_dynamic_draw_floats(VCT_DYNAMIC_TRIS_MAX) == (size_t)VCT_DYNAMIC_TRIS_MAX * 9u);
    {
        std::vector<float> arr(vct_dynamic_draw_floats(150));
        arr[(size_t)149 * 9 + 8] = 1.0f;                          // the last float of the last triangle
    }
    // the scratch of the dynamic pass per raster target, and the second visibility buffer
    {
        const VctDynamicDrawSizes s = vct_dynamic_draw_sizes(150, 203, 117);
        EXPECT(s.ok && s.arrays == 4u * 150u * 36u && s.lists == 150u * 16u && s.recs == 150u * 192u);
        EXPECT(s.items == ((size_t)203 * 117 / 16 + 4096) * 8u && s.vis == (size_t)203 * 117 * 8u);
        std::vector<unsigned char> vis(s.vis), lists(s.lists), recs(s.recs);
        vis[((size_t)116 * 203 + 202) * 8 + 7] = 1;               // the last byte of the last pixel's word
        lists[((size_t)150 * 2 + 150 * 2 - 1) * 4 + 3] = 1;       // the last entry of the group list behind the wave list
        recs[((size_t)2 * 150 - 1) * 96 + 95] = 1;                // the record of wave entry 0
    }
    {
        const VctDynamicDrawSizes s = vct_dynamic_draw_sizes(1, 1, 1);
        EXPECT(s.ok && s.arrays == 144u && s.lists == 16u && s.recs == 192u && s.items == 4096u * 8u && s.vis == 8u);
    }
    {
        // the largest legal layer on the largest frame and the largest shadow map the config admits
        const VctDynamicDrawSizes f = vct_dynamic_draw_sizes(VCT_DYNAMIC_TRIS_MAX, 32768, 32768);
        if (sizeof(size_t) >= 8) {
            EXPECT(f.ok && f.arrays == (size_t)VCT_DYNAMIC_TRIS_MAX * 144u && f.recs == (size_t)VCT_DYNAMIC_TRIS_MAX * 192u);
            EXPECT(f.vis == ((size_t)1 << 33) && f.items == (((size_t)1 << 26) + 4096) * 8u);
        }
        // 2^62 pixels fit size_t, their 8-byte words do not: refused, not wrapped
        const VctDynamicDrawSizes g = vct_dynamic_draw_sizes(VCT_DYNAMIC_TRIS_MAX, INT32_MAX, INT32_MAX);
        EXPECT(!g.ok && g.vis == 0u && g.arrays == 0u);
        const VctDynamicDrawSizes e = vct_dynamic_draw_sizes(1, INT32_MAX, 1 << 29);
        EXPECT(e.ok == (sizeof(size_t) >= 8));
        if (e.ok) EXPECT(e.vis == (size_t)INT32_MAX * ((size_t)1 << 32));
    }
    for (const VctDynamicDrawSizes& s : {vct_dynamic_draw_sizes(0, 8, 8), vct_dynamic_draw_sizes(-1, 8, 8),
                                         vct_dynamic_draw_sizes(VCT_DYNAMIC_TRIS_MAX + 1, 8, 8), vct_dynamic_draw_sizes(5, 0, 8),
                                         vct_dynamic_draw_sizes(5, 8, -3), vct_dynamic_draw_sizes(INT32_MIN, INT32_MIN, INT32_MIN)})
        EXPECT(!s.ok && s.arrays == 0u && s.lists == 0u && s.recs == 0u && s.items == 0u && s.vis == 0u);
    if (failures) { printf("dynamic_draw_check: %d failures\n", failures); return 1; }
    printf("dynamic_draw_check ok\n");
    return 0;
}
