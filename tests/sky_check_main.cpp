// Host-only driver of csrc/vct_sky_check.h -- the table check of vct_set_sky, the folding of the basis constants and the
// evaluation chain -- for a run with and without -fsanitize=address,undefined (tests/test_sky_restatement.py).  No GPU call.
//   sky_check_main                       the checks; prints "sky_check ok"
//   sky_check_main SH DIRS OUT           SH: 27 floats, DIRS: n x 3 floats (raw, native); OUT: the 27 folded coefficients,
//                                        then vct_sky_eval of every direction (n x 3 floats)
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_sky_check.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool read_floats(const char* path, std::vector<float>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(bytes > 0 ? (size_t)bytes / sizeof(float) : 0);
    const bool ok = bytes >= 0 && (size_t)bytes % sizeof(float) == 0 && fread(out.data(), sizeof(float), out.size(), f) == out.size();
    fclose(f);
    return ok;
}

static int evaluate(const char* sh_path, const char* dirs_path, const char* out_path) {
    std::vector<float> sh, dirs;
    if (!read_floats(sh_path, sh) || sh.size() != VCT_SKY_FLOATS || !read_floats(dirs_path, dirs) || dirs.size() % 3 != 0) return 2;
    std::vector<float> out(VCT_SKY_FLOATS + dirs.size());          // exactly sized: a write past it is an ASan report
    vct_sky_fold(sh.data(), out.data());
    for (size_t i = 0; i < dirs.size() / 3; ++i) vct_sky_eval(out.data(), &dirs[3 * i], &out[VCT_SKY_FLOATS + 3 * i]);
    FILE* f = fopen(out_path, "wb");
    if (!f) return 2;
    const bool ok = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 4) return evaluate(argv[1], argv[2], argv[3]);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float denorm = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
    size_t bad = 99;
    // exactly-sized heap tables: a read past 27 floats is an ASan report
    std::vector<float> t(VCT_SKY_FLOATS, 0.0f);
    EXPECT(vct_sky_check(nullptr, &bad) == VCT_SKY_DETACH);
    EXPECT(vct_sky_check(nullptr, nullptr) == VCT_SKY_DETACH);
    EXPECT(vct_sky_check(t.data(), &bad) == VCT_SKY_DETACH);               // all +0
    for (size_t i = 0; i < t.size(); i += 2) t[i] = -0.0f;
    EXPECT(vct_sky_check(t.data(), &bad) == VCT_SKY_DETACH);               // +0 and -0
    for (size_t at = 0; at < t.size(); ++at) {
        for (float v : {denorm, -denorm, 1.0f, -1.0f, big, -big}) {          // one value that is not zero: a sky
            std::vector<float> u = t;
            u[at] = v;
            EXPECT(vct_sky_check(u.data(), &bad) == VCT_SKY_OK);
            EXPECT(vct_sky_check(u.data(), nullptr) == VCT_SKY_OK);
        }
        for (float v : {nan, -nan, inf, -inf}) {
            std::vector<float> u(VCT_SKY_FLOATS, 0.25f);
            u[at] = v;
            bad = 99;
            EXPECT(vct_sky_check(u.data(), &bad) == VCT_SKY_BAD);
            EXPECT(bad == at);
            EXPECT(vct_sky_check(u.data(), nullptr) == VCT_SKY_BAD);
            std::vector<float> z = t;                                      // ... also in a table that is otherwise zero
            z[at] = v;
            EXPECT(vct_sky_check(z.data(), &bad) == VCT_SKY_BAD && bad == at);
        }
    }
    {   // the first bad value is named
        std::vector<float> u(VCT_SKY_FLOATS, 1.0f);
        u[5] = nan; u[20] = inf;
        EXPECT(vct_sky_check(u.data(), &bad) == VCT_SKY_BAD && bad == 5);
    }
    // the folding: (float)(K_i * (double)sh), the constants of the header, zeros stay zeros with their sign
    {
        std::vector<float> sh(VCT_SKY_FLOATS), poly(VCT_SKY_FLOATS, 7.0f);
        for (size_t i = 0; i < sh.size(); ++i) sh[i] = 0.125f * (float)(i + 1) * ((i & 1) ? -1.0f : 1.0f);
        vct_sky_fold(sh.data(), poly.data());
        const double K[9] = {0.28209479177387814, 0.4886025119029199, 0.4886025119029199, 0.4886025119029199, 1.0925484305920792,
                             1.0925484305920792, 0.31539156525252005, 1.0925484305920792, 0.5462742152960396};
        for (size_t i = 0; i < sh.size(); ++i) EXPECT(poly[i] == (float)(K[i / 3] * (double)sh[i]));
        for (int i = 0; i < 9; ++i) EXPECT(vct_sky_basis_constant(i) == K[i]);
        EXPECT(fabs(K[0] * K[0] * 4.0 * 3.14159265358979323846 - 1.0) < 1e-15);
        vct_sky_fold(t.data(), poly.data());
        EXPECT(memcmp(poly.data(), t.data(), sizeof(float) * VCT_SKY_FLOATS) == 0);
        sh.assign(VCT_SKY_FLOATS, denorm);                                 // a denormal folds without a trap: K < 2 rounds it to itself, to 0 or to 2 ulp
        vct_sky_fold(sh.data(), poly.data());
        for (size_t i = 0; i < sh.size(); ++i) EXPECT(poly[i] >= 0.0f && poly[i] <= 2.0f * denorm);
    }
    // the evaluation: a constant sky is the constant; the clamp; a NaN direction gives fmaxf's 0
    {
        std::vector<float> poly(VCT_SKY_FLOATS, 0.0f), out(3, 9.0f);
        poly[0] = 0.5f; poly[1] = 2.0f; poly[2] = -1.0f;
        const float axes[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
        for (const float* d : {axes[0], axes[1], axes[2], axes[3], axes[4], axes[5]}) {
            vct_sky_eval(poly.data(), d, out.data());
            EXPECT(out[0] == 0.5f && out[1] == 2.0f && out[2] == 0.0f);
        }
        poly[3 * 1 + 0] = 1.0f;                                            // + y in red
        vct_sky_eval(poly.data(), axes[2], out.data());
        EXPECT(out[0] == 1.5f);
        vct_sky_eval(poly.data(), axes[3], out.data());
        EXPECT(out[0] == 0.0f);                                            // 0.5 - 1 clamped
        const float dn[3] = {nan, 0.0f, 1.0f};
        vct_sky_eval(poly.data(), dn, out.data());
        EXPECT(out[0] == 0.0f && out[1] == 0.0f && out[2] == 0.0f);
    }
    if (failures) return 1;
    printf("sky_check ok\n");
    return 0;
}
