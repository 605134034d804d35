// Host-only driver of what the dynamic mesh's corner normals add: the argument checks and the size arithmetic of
// csrc/vct_dynamic_check.h, and the arithmetic of csrc/vct_import_check.h that the NRM prepare kernels call --
// vct_import_cofactor, vct_import_cofactor_normal and vct_import_corner_frame -- on the adversarial corners and the
// matrices of tests/dynnormalcases.py, against the bit patterns the NumPy restatement (tests/dynamic_normals_ref.py) gives
// for them.  The two tables below are written out by tests/test_dynamic_normals_host.py host_literals(), which also
// holds them against the restatement.  For a run under -fsanitize=address,undefined, built with -ffp-contract=off.
// No GPU call.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../voxel-cone-tracing_amd/csrc/vct_dynamic_check.h"
#include "../voxel-cone-tracing_amd/csrc/vct_import_check.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct CornerCase {
    const char* name;
    uint32_t n[3];
    uint32_t face[9];        // u_f, t_f, b_f
    uint32_t want[9];        // u, t, b
    int path;                // 0 the corner's own frame, 1 the accept test fails, 2 t_c is all zero
};
struct MatrixCase {
    const char* name;
    uint32_t m[12];
    uint32_t n[3];
    uint32_t want[3];
};

static const CornerCase kCorners[] = {
    {"nan", {0x7fc00000u, 0x3f000000u, 0x3f000000u}, {0x3e4fabc8u, 0x3f591869u, 0x3efaae2au, 0x00000000u, 0xbf000005u, 0x3f5db3d3u, 0x3f7aae1fu, 0xbe33d92cu, 0xbdcfabd0u},
     {0x3e4fabc8u, 0x3f591869u, 0x3efaae2au, 0x00000000u, 0xbf000005u, 0x3f5db3d3u, 0x3f7aae1fu, 0xbe33d92cu, 0xbdcfabd0u}, 1},
    {"+inf", {0x7f800000u, 0x00000000u, 0x00000000u}, {0xbe4fabb3u, 0x3f591872u, 0x3efaae11u, 0x00000000u, 0xbeffffeeu, 0x3f5db3dbu, 0x3f7aae20u, 0x3e33d920u, 0x3dcfaba4u},
     {0xbe4fabb3u, 0x3f591872u, 0x3efaae11u, 0x00000000u, 0xbeffffeeu, 0x3f5db3dbu, 0x3f7aae20u, 0x3e33d920u, 0x3dcfaba4u}, 1},
    {"-inf", {0x3e4ccccdu, 0xff800000u, 0x3dcccccdu}, {0xbefaae22u, 0x3f59186fu, 0x3e4fab96u, 0x00000000u, 0xbe6e2b7du, 0x3f78fab3u, 0x3f5f3792u, 0x3ef3ce2eu, 0x3de93879u},
     {0xbefaae22u, 0x3f59186fu, 0x3e4fab96u, 0x00000000u, 0xbe6e2b7du, 0x3f78fab3u, 0x3f5f3792u, 0x3ef3ce2eu, 0x3de93879u}, 1},
    {"zero", {0x00000000u, 0x00000000u, 0x00000000u}, {0xbefaae24u, 0x3f59186du, 0xbe4fab98u, 0x00000000u, 0x3e6e2b81u, 0x3f78fab3u, 0x3f5f3790u, 0x3ef3ce30u, 0xbde9387fu},
     {0xbefaae24u, 0x3f59186du, 0xbe4fab98u, 0x00000000u, 0x3e6e2b81u, 0x3f78fab3u, 0x3f5f3790u, 0x3ef3ce30u, 0xbde9387fu}, 1},
    {"at 90 degrees", {0x3f800000u, 0x00000000u, 0x00000000u}, {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u},
     {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u}, 1},
    {"beyond 90 degrees", {0x3e99999au, 0x00000000u, 0xbf800000u}, {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u},
     {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u}, 1},
    {"length overflows", {0x00000000u, 0x00000000u, 0x7f61b1e6u}, {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u},
     {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u}, 1},
    {"square underflows", {0x00000000u, 0x00000000u, 0x0da24260u}, {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u},
     {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u}, 1},
    {"parallel to t_f", {0x3f800000u, 0x00000000u, 0x0da24260u}, {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u},
     {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u}, 2},
    {"good on the flat", {0x3f19999au, 0x3e99999au, 0x3f333333u}, {0x00000000u, 0x00000000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x3f800000u, 0x00000000u},
     {0x3f1e6d23u, 0x3e9e6d23u, 0x3f38d4a8u, 0x3f4916fcu, 0xbe79a0f6u, 0xbf119de5u, 0xb2800000u, 0x3f6b4d18u, 0xbec9afccu}, 0},
};
static const MatrixCase kMatrices[] = {
    {"identity", {0x3f800000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x3f800000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x3f800000u, 0x00000000u},
     {0x3ef5c28fu, 0xbf19999au, 0x3f23d70au}, {0x3ef5c28fu, 0xbf19999au, 0x3f23d70au}},
    {"rotation", {0x3f5563ebu, 0xbd755c26u, 0x3f0c96ecu, 0x42c698bdu, 0x3e1fab89u, 0x3f7aac7du, 0xbe04fb19u, 0xc1980de9u, 0xbf07ac4cu, 0x3e4688c3u, 0x3f53577du, 0xc1df4ee1u},
     {0x3ef5c28fu, 0xbf19999au, 0x3f23d70au}, {0x3f499b0bu, 0xbf188554u, 0x3e216c12u}},
    {"scale", {0x3f800000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x40400000u, 0x00000000u, 0xc1cccccdu, 0x00000000u, 0x00000000u, 0x3e800000u, 0xc2f00000u},
     {0x3ef5c28fu, 0xbf19999au, 0x3f23d70au}, {0x3eb851ebu, 0xbe19999au, 0x3ff5c28fu}},
    {"mirror", {0xbf800000u, 0x00000000u, 0x00000000u, 0x42000000u, 0x00000000u, 0x3f800000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x3f800000u, 0x00000000u},
     {0x3ef5c28fu, 0xbf19999au, 0x3f23d70au}, {0x3ef5c28fu, 0x3f19999au, 0xbf23d70au}},
    {"singular", {0x3f800000u, 0x40000000u, 0x40400000u, 0x43e33333u, 0x40000000u, 0x40800000u, 0x40c00000u, 0x445e6666u, 0x3f000000u, 0x00000000u, 0x3f800000u, 0xc1000000u},
     {0x3ef5c28fu, 0xbf19999au, 0x3f23d70au}, {0x3d23d700u, 0xbca3d700u, 0x00000000u}},
    {"nan", {0x3f5563ebu, 0xbd755c26u, 0x3f0c96ecu, 0x42b698bdu, 0x3e1fab89u, 0x3f7aac7du, 0x7fc00000u, 0xc1b80de9u, 0xbf07ac4cu, 0x3e4688c3u, 0x3f53577du, 0xc1af4ee1u},
     {0x3ef5c28fu, 0xbf19999au, 0x3f23d70au}, {0x7fc00000u, 0xbf188554u, 0x7fc00000u}},
    {"tiny", {0x1e3ce508u, 0x00000000u, 0x00000000u, 0x41800000u, 0x00000000u, 0x1e3ce508u, 0x00000000u, 0x414ccccdu, 0x00000000u, 0x00000000u, 0x1e3ce508u, 0xc3200000u},
     {0x3ef5c28fu, 0xbf19999au, 0x3f23d70au}, {0x000085ceu, 0x8000a741u, 0x0000b268u}},
};

static void floats(const uint32_t* bits, int n, float* out) { memcpy(out, bits, (size_t)n * sizeof(float)); }
static bool same(const float* got, const uint32_t* want, int n) { return memcmp(got, want, (size_t)n * sizeof(float)) == 0; }

int main() {
    // ---- vct_dynamic_check.h ----
    const float* dangling = reinterpret_cast<const float*>(8);
    EXPECT(!vct_dynamic_check_normals(true, 1) && !vct_dynamic_check_normals(true, VCT_DYNAMIC_TRIS_MAX));
    EXPECT(vct_dynamic_check_normals(false, 96) && vct_dynamic_check_normals(true, 0) && vct_dynamic_check_normals(false, 0));
    EXPECT(!vct_dynamic_check_normals_update(true, true, dangling, VCT_MEM_HOST));           // the values are never read
    EXPECT(!vct_dynamic_check_normals_update(true, true, dangling, VCT_MEM_DEVICE));
    EXPECT(vct_dynamic_check_normals_update(false, false, dangling, VCT_MEM_HOST));
    EXPECT(vct_dynamic_check_normals_update(false, true, dangling, VCT_MEM_HOST));
    EXPECT(vct_dynamic_check_normals_update(true, false, dangling, VCT_MEM_HOST));
    EXPECT(vct_dynamic_check_normals_update(true, true, nullptr, VCT_MEM_HOST));
    EXPECT(vct_dynamic_check_normals_update(true, true, dangling, 2) && vct_dynamic_check_normals_update(true, true, dangling, -1));
    for (uintptr_t off = 1; off < 4; ++off)
        EXPECT(vct_dynamic_check_normals_update(true, true, reinterpret_cast<const float*>(8 + off), VCT_MEM_HOST));
    EXPECT(!vct_dynamic_check_frames(true, VCT_DYNAMIC_DRAW_GBUFFER, true) && !vct_dynamic_check_frames(true, VCT_DYNAMIC_DRAW_SHADOW, true));
    EXPECT(vct_dynamic_check_frames(false, VCT_DYNAMIC_DRAW_ALL, true) && vct_dynamic_check_frames(true, 0, true));
    EXPECT(vct_dynamic_check_frames(true, VCT_DYNAMIC_DRAW_ALL, false));
    EXPECT(vct_dynamic_normals_bytes(1) == 36 && vct_dynamic_normals_bytes(96) == 96 * 36);
    EXPECT(vct_dynamic_normals_bytes(VCT_DYNAMIC_TRIS_MAX) == (size_t)VCT_DYNAMIC_TRIS_MAX * 36);
    EXPECT(vct_dynamic_normals_bytes(0) == 0 && vct_dynamic_normals_bytes(-1) == 0 && vct_dynamic_normals_bytes(VCT_DYNAMIC_TRIS_MAX + 1) == 0);
    EXPECT(vct_dynamic_normals_bytes(257) == vct_dynamic_draw_floats(257) * sizeof(float));      // one [ntri][9] array

    // ---- the corner frame, on heap copies of exactly the sizes the functions may touch ----
    int paths[3] = {0, 0, 0};
    for (const CornerCase& k : kCorners) {
        std::vector<float> n(3), f(9), out(9);
        floats(k.n, 3, n.data());
        floats(k.face, 9, f.data());
        const bool own = vct_import_corner_frame(n.data(), &f[0], &f[3], &f[6], &out[0], &out[3], &out[6]);
        if (!same(out.data(), k.want, 9) || own != (k.path == 0)) { printf("FAILED corner '%s'\n", k.name); ++failures; }
        if (k.path != 0) EXPECT(same(out.data(), k.face, 9));       // a fallback IS the face frame, bit for bit
        for (int i = 0; i < 9; ++i) EXPECT(vct_import_finite(out[i]));
        ++paths[k.path];
    }
    EXPECT(paths[0] >= 1 && paths[1] >= 6 && paths[2] >= 1);
    // ---- the cofactor rule ----
    for (const MatrixCase& k : kMatrices) {
        std::vector<float> m(12), n(3), c(9), out(3);
        floats(k.m, 12, m.data());
        floats(k.n, 3, n.data());
        vct_import_cofactor(m.data(), c.data());
        vct_import_cofactor_normal(c.data(), n.data(), out.data());
        if (!same(out.data(), k.want, 3)) { printf("FAILED matrix '%s'\n", k.name); ++failures; }
    }
    {   // the identity's cofactor is the identity, and cross(A a, A b) = C cross(a, b) exactly for a matrix of small integers
        const float id[12] = {1, 0, 0, 5, 0, 1, 0, 6, 0, 0, 1, 7};
        float c[9];
        vct_import_cofactor(id, c);
        for (int i = 0; i < 9; ++i) EXPECT(c[i] == (i % 4 == 0 ? 1.0f : 0.0f));
        const float A[12] = {2, -1, 0, 9, 3, 1, 4, 9, 0, 5, -2, 9}, a[3] = {1, 2, -3}, b[3] = {-2, 0, 5};
        float Aa[3], Ab[3];
        for (int r = 0; r < 3; ++r) {
            Aa[r] = A[4 * r] * a[0] + A[4 * r + 1] * a[1] + A[4 * r + 2] * a[2];
            Ab[r] = A[4 * r] * b[0] + A[4 * r + 1] * b[1] + A[4 * r + 2] * b[2];
        }
        const float ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const float left[3] = {Aa[1] * Ab[2] - Aa[2] * Ab[1], Aa[2] * Ab[0] - Aa[0] * Ab[2], Aa[0] * Ab[1] - Aa[1] * Ab[0]};
        float right[3];
        vct_import_cofactor(A, c);
        vct_import_cofactor_normal(c, ab, right);
        for (int r = 0; r < 3; ++r) EXPECT(left[r] == right[r]);
    }
    if (failures) { printf("dynamic_normals_check: %d failure(s)\n", failures); return 1; }
    printf("dynamic_normals_check ok\n");
    return 0;
}
