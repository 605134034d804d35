// Host-only driver of csrc/vct_dynamic_check.h -- the argument checks, the default-capacity rule and the buffer-size
// arithmetic of the dynamic mesh (vct_api_dynamic.hip) -- for a run under -fsanitize=address,undefined
// (tests/test_dynamic_host.py).  No GPU call.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_dynamic_check.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    std::vector<float> pos(9 * 5, 1.0f), alb(4 * 3, 0.5f);
    std::vector<int32_t> mat = {0, 1, 2, 2, 0};
    // arguments of an attach
    EXPECT(!vct_dynamic_check_args(pos.data(), mat.data(), 5, alb.data(), 3, 0));
    EXPECT(!vct_dynamic_check_args(pos.data(), mat.data(), 1, alb.data(), 1, INT32_MAX));
    EXPECT(vct_dynamic_check_args(nullptr, mat.data(), 5, alb.data(), 3, 0));
    EXPECT(vct_dynamic_check_args(pos.data(), nullptr, 5, alb.data(), 3, 0));
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), 5, nullptr, 3, 0));
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), 0, alb.data(), 3, 0));
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), -1, alb.data(), 3, 0));
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), INT32_MIN, alb.data(), 3, 0));
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), VCT_DYNAMIC_TRIS_MAX + 1, alb.data(), 3, 0));      // refused before a read
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), INT32_MAX, alb.data(), 3, 0));
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), 5, alb.data(), 0, 0));
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), 5, alb.data(), -2, 0));
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), 5, alb.data(), 3, -1));
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), 5, alb.data(), 2, 0));       // material 2 of a table of 2
    mat[3] = -1;
    EXPECT(vct_dynamic_check_args(pos.data(), mat.data(), 5, alb.data(), 3, 0));
    EXPECT(!vct_dynamic_check_args(pos.data(), mat.data(), 3, alb.data(), 3, 0));      // the bad index lies behind the mesh
    {
        std::vector<int32_t> many((size_t)VCT_DYNAMIC_TRIS_MAX, 2);
        std::vector<float> one(9, 0.0f);
        EXPECT(!vct_dynamic_check_args(one.data(), many.data(), VCT_DYNAMIC_TRIS_MAX, alb.data(), 3, 7));    // only `material` is read
        many.back() = 3;
        EXPECT(vct_dynamic_check_args(one.data(), many.data(), VCT_DYNAMIC_TRIS_MAX, alb.data(), 3, 7));
    }
    // arguments of an update
    EXPECT(!vct_dynamic_check_update(true, pos.data(), VCT_MEM_HOST));
    EXPECT(!vct_dynamic_check_update(true, pos.data(), VCT_MEM_DEVICE));
    EXPECT(vct_dynamic_check_update(false, pos.data(), VCT_MEM_HOST));
    EXPECT(vct_dynamic_check_update(true, nullptr, VCT_MEM_HOST));
    EXPECT(vct_dynamic_check_update(true, pos.data(), 2));
    EXPECT(vct_dynamic_check_update(true, pos.data(), -1));
    EXPECT(vct_dynamic_check_update(true, (const float*)((const char*)pos.data() + 2), VCT_MEM_DEVICE));

    // bricks of a grid
    EXPECT(vct_dynamic_grid_bricks(8) == 1u && vct_dynamic_grid_bricks(32) == 64u && vct_dynamic_grid_bricks(64) == 512u);
    EXPECT(vct_dynamic_grid_bricks(1024) == 2097152u && vct_dynamic_grid_bricks(4) == 0u && vct_dynamic_grid_bricks(-8) == 0u);

    // the capacity rule: as asked, or twice the touched bricks and at least 64; never more than the grid has
    EXPECT(vct_dynamic_capacity(0, 0u, 512u) == 64u);
    EXPECT(vct_dynamic_capacity(0, 12u, 512u) == 64u);
    EXPECT(vct_dynamic_capacity(0, 32u, 512u) == 64u);
    EXPECT(vct_dynamic_capacity(0, 33u, 512u) == 66u);
    EXPECT(vct_dynamic_capacity(0, 300u, 512u) == 512u);
    EXPECT(vct_dynamic_capacity(0, 5u, 1u) == 1u);
    EXPECT(vct_dynamic_capacity(0, 0xffffffffu, 2097152u) == 2097152u);      // 2 * touched does not wrap
    EXPECT(vct_dynamic_capacity(11, 12u, 512u) == 11u);
    EXPECT(vct_dynamic_capacity(1, 500u, 512u) == 1u);
    EXPECT(vct_dynamic_capacity(INT32_MAX, 0u, 2097152u) == 2097152u);
    EXPECT(vct_dynamic_capacity(600, 0u, 512u) == 512u);

    // sizes: every product checked, the largest legal layer fits, and a buffer of exactly that size takes its last byte
    {
        const VctDynamicSizes s = vct_dynamic_sizes(150, 3, 64u, 64, true);
        EXPECT(s.ok && s.pos == 150u * 36u && s.material == 600u && s.albedo == 48u && s.big_list == 600u);
        EXPECT(s.brick_slot == 2048u && s.slot_list == 256u && s.acc == 64u * 8192u && s.acc_attr == 64u * 12288u);
        EXPECT(s.pool == 64u * 2048u && s.volume == 64u * 64u * 64u * 4u && s.words >= 24u * 4u);
        std::vector<unsigned char> buf(s.acc);
        buf[s.acc - 1] = 1;                                   // (ASan would see a short allocation)
        std::vector<unsigned char> pool(s.pool);
        pool[(size_t)63 * 512 * 4 + 511 * 4 + 3] = 1;         // the last texel of the last slot
        const VctDynamicSizes n = vct_dynamic_sizes(150, 3, 64u, 64, false);
        EXPECT(n.ok && n.acc_attr == 0u && n.acc == s.acc);
    }
    {
        const VctDynamicSizes s = vct_dynamic_sizes(VCT_DYNAMIC_TRIS_MAX, INT32_MAX, 2097152u, 1024, true);
        if (sizeof(size_t) >= 8) {
            EXPECT(s.ok && s.pos == (size_t)VCT_DYNAMIC_TRIS_MAX * 36u && s.acc == (size_t)2097152u * 8192u);
            EXPECT(s.acc_attr == (size_t)2097152u * 12288u && s.volume == ((size_t)1 << 32));
            EXPECT(s.albedo == (size_t)INT32_MAX * 16u);
        }
        EXPECT(vct_dynamic_sizes(5, 3, 0xffffffffu, 1024, true).ok == (sizeof(size_t) >= 8));
    }
    EXPECT(!vct_dynamic_sizes(0, 3, 64u, 64, true).ok);
    EXPECT(!vct_dynamic_sizes(-1, 3, 64u, 64, true).ok);
    EXPECT(!vct_dynamic_sizes(VCT_DYNAMIC_TRIS_MAX + 1, 3, 64u, 64, true).ok);
    EXPECT(!vct_dynamic_sizes(5, 0, 64u, 64, true).ok);
    EXPECT(!vct_dynamic_sizes(5, 3, 64u, 4, true).ok);
    {
        const VctDynamicSizes none = vct_dynamic_sizes(0, 3, 64u, 64, true);
        EXPECT(none.pos == 0u && none.acc == 0u && none.volume == 0u);
        size_t r = 7;
        EXPECT(!vct_dynamic_mul((size_t)-1, 2, &r));
        EXPECT(vct_dynamic_mul((size_t)-1, 1, &r) && r == (size_t)-1);
    }
    if (failures) { printf("dynamic_check: %d failures\n", failures); return 1; }
    printf("dynamic_check ok\n");
    return 0;
}
