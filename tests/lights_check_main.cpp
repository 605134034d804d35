// Host-only driver of csrc/vct_lights_check.h -- the table check of vct_set_lights and the folding of a light into the
// device's form -- for a run under -fsanitize=address,undefined (tests/test_lights_restatement.py).  No GPU call.
// With two arguments it also folds the vct_light records of the first file into the second (VctLightDev records), so
// that the test can hold the host's folding against the numpy restatement bit for bit.
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_lights_check.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static vct_light good_point() {
    vct_light l;
    memset(&l, 0, sizeof l);
    l.position[0] = 1.0f; l.position[1] = -2.0f; l.position[2] = 3.0f;
    l.radius = 10.0f; l.source_radius = 0.5f;
    l.color[0] = 1.0f; l.color[1] = 0.0f; l.color[2] = 2.0f;
    return l;
}
static vct_light good_spot() {
    vct_light l = good_point();
    l.flags = VCT_LIGHT_SPOT;
    l.direction[0] = 0.0f; l.direction[1] = -3.0f; l.direction[2] = 4.0f;
    l.cos_outer = 0.5f; l.cos_inner = 0.75f;
    return l;
}

int main(int argc, char** argv) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    static_assert(sizeof(vct_light) == 56, "vct_light is 56 bytes");
    static_assert(sizeof(VctLightDev) == 64, "one scalar load of sixteen dwords");
    int32_t bad = 99;
    const char* why = nullptr;
    // exactly-sized heap tables: a read past n lights is an ASan report
    for (int32_t n : {1, 2, 63, 64}) {
        std::vector<vct_light> t((size_t)n);
        for (int32_t i = 0; i < n; ++i) t[(size_t)i] = (i & 1) ? good_spot() : good_point();
        EXPECT(vct_lights_check(t.data(), n, &bad, &why) == VCT_LIGHTS_OK);
        EXPECT(vct_lights_check(t.data(), n, nullptr, nullptr) == VCT_LIGHTS_OK);
        // every float field of the last light, with every non-finite value: refused, also for a point light's spot fields
        for (int field = 0; field < 13; ++field)
            for (float v : {nan, inf, -inf}) {
                std::vector<vct_light> u = t;
                float* f = reinterpret_cast<float*>(&u[(size_t)n - 1]);
                f[field] = v;
                bad = 99;
                EXPECT(vct_lights_check(u.data(), n, &bad, &why) == VCT_LIGHTS_BAD);
                EXPECT(bad == n - 1 && why != nullptr);
            }
    }
    EXPECT(vct_lights_check(nullptr, 0, &bad, &why) == VCT_LIGHTS_OK);      // nothing is read
    struct { void (*edit)(vct_light&); bool spot; bool ok; } cases[] = {
        {[](vct_light& l) { l.radius = 0.0f; }, false, false},
        {[](vct_light& l) { l.radius = -1.0f; }, false, false},
        {[](vct_light& l) { l.source_radius = 0.0f; }, false, false},
        {[](vct_light& l) { l.source_radius = -0.5f; }, true, false},
        {[](vct_light& l) { l.color[1] = -1e-30f; }, false, false},
        {[](vct_light& l) { l.color[0] = l.color[1] = l.color[2] = 0.0f; }, false, true},      // a black light is a light
        {[](vct_light& l) { l.color[2] = -0.0f; }, false, true},                               // -0 is not below 0
        {[](vct_light& l) { l.flags = 2u; }, false, false},
        {[](vct_light& l) { l.flags = 3u; }, true, false},
        {[](vct_light& l) { l.flags = 0x80000001u; }, true, false},
        {[](vct_light& l) { l.direction[0] = l.direction[1] = l.direction[2] = 0.0f; }, true, false},
        {[](vct_light& l) { l.direction[0] = l.direction[1] = l.direction[2] = 0.0f; }, false, true},      // unused by a point light
        {[](vct_light& l) { l.direction[0] = 3e38f; l.direction[1] = 3e38f; }, true, false},               // the length overflows
        {[](vct_light& l) { l.direction[0] = 0.0f; l.direction[1] = 1e-30f; l.direction[2] = 0.0f; }, true, false},   // ... underflows
        {[](vct_light& l) { l.cos_outer = l.cos_inner; }, true, false},
        {[](vct_light& l) { l.cos_outer = 0.8f; }, true, false},
        {[](vct_light& l) { l.cos_outer = -1.0f; l.cos_inner = 1.0f; }, true, true},
        {[](vct_light& l) { l.cos_outer = -1.0001f; }, true, false},
        {[](vct_light& l) { l.cos_inner = 1.0001f; }, true, false},
        {[](vct_light& l) { l.cos_outer = 2.0f; l.cos_inner = 1.0f; }, false, true},           // unused by a point light
    };
    for (const auto& c : cases) {
        vct_light l = c.spot ? good_spot() : good_point();
        c.edit(l);
        EXPECT((vct_light_fault(&l) == nullptr) == c.ok);
    }
    // folding
    {
        const vct_light s = good_spot();
        VctLightDev d;
        vct_light_fold(&s, &d);
        EXPECT(d.R2 == 100.0f && d.S2 == 0.25f && d.flags == VCT_LIGHT_SPOT);
        EXPECT(d.axis[0] == 0.0f && d.axis[1] == -3.0f * (1.0f / 5.0f) && d.axis[2] == 4.0f * (1.0f / 5.0f));
        EXPECT(d.cos_outer == 0.5f && d.inv_cone == 4.0f);
        const vct_light p = good_point();
        vct_light_fold(&p, &d);
        EXPECT(d.axis[0] == 0.0f && d.axis[1] == 0.0f && d.axis[2] == 0.0f && d.inv_cone == 0.0f && d.flags == 0u);
        EXPECT(d.pos[0] == 1.0f && d.pos[1] == -2.0f && d.pos[2] == 3.0f && d.color[2] == 2.0f);
    }
    if (argc == 3) {
        FILE* in = fopen(argv[1], "rb");
        FILE* out = in ? fopen(argv[2], "wb") : nullptr;
        if (!in || !out) { printf("cannot open the files\n"); return 2; }
        vct_light l;
        while (fread(&l, sizeof l, 1, in) == 1) {
            if (vct_light_fault(&l)) { printf("a light of the file is outside the contract: %s\n", vct_light_fault(&l)); ++failures; break; }
            VctLightDev d;
            vct_light_fold(&l, &d);
            fwrite(&d, sizeof d, 1, out);
        }
        fclose(in);
        fclose(out);
    }
    if (failures) return 1;
    printf("lights_check ok\n");
    return 0;
}
