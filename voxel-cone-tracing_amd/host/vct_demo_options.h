// vct_demo_options.h -- the list options of vct_demo that are parsed before anything touches a GPU, so that a malformed
// list ends the program with exit status 1 on any machine (tests/test_gloss_restatement.py).
#ifndef VCT_DEMO_OPTIONS_H_
#define VCT_DEMO_OPTIONS_H_

#include <math.h>
#include <cmath>
#include <stdio.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../include/vct.h"

// --gloss-classes TAN,SHIN[;TAN,SHIN...]: 1 .. VCT_GLOSS_CLASSES_MAX classes, tan_specular finite and > 0, shininess finite
// and >= 0 (the contract of vct_set_gloss_classes).  Returns null, or the place in the list where it stops making sense.
static inline const char* vct_demo_parse_gloss_classes(const char* list, std::vector<vct_gloss_class>& out) {
    out.clear();
    for (const char* q = list; *q;) {
        float t = 0.0f, s = 0.0f;
        int used = 0;
        if (sscanf(q, "%f,%f%n", &t, &s, &used) != 2 || !(t > 0.0f) || isinf(t) || !(s >= 0.0f) || isinf(s)) return q;
        if (out.size() == (size_t)VCT_GLOSS_CLASSES_MAX) return q;
        out.push_back(vct_gloss_class{t, s});
        q += used;
        if (*q == ';') { if (!q[1]) return q; ++q; }
        else if (*q) return q;
    }
    return out.empty() ? list : nullptr;
}

// --gloss MATERIAL=CLASS[;MATERIAL=CLASS...]: material indices >= 0 (the range is the scene's to check), classes below
// nclasses.  Returns null or the offending place.
static inline const char* vct_demo_parse_gloss(const char* list, int nclasses, std::vector<std::pair<int, int>>& out) {
    out.clear();
    for (const char* q = list; *q;) {
        int m = -1, k = -1, used = 0;
        if (sscanf(q, "%d=%d%n", &m, &k, &used) != 2 || m < 0 || k < 0 || k >= nclasses) return q;
        out.push_back(std::make_pair(m, k));
        q += used;
        if (*q == ';') { if (!q[1]) return q; ++q; }
        else if (*q) return q;
    }
    return out.empty() ? list : nullptr;
}

// --sky-gradient ZR,ZG,ZB;HR,HG,HB;GR,GG,GB[;UX,UY,UZ]: zenith, horizon and ground colour (finite) and an optional up
// vector (finite, not zero; +y when left out), for vcth_sky_gradient.  Returns null or the offending place.
static inline const char* vct_demo_parse_sky_gradient(const char* list, float zenith[3], float horizon[3], float ground[3], float up[3]) {
    float* const dst[4] = {zenith, horizon, ground, up};
    up[0] = 0.0f; up[1] = 1.0f; up[2] = 0.0f;
    const char* q = list;
    int k = 0;
    for (; k < 4 && *q; ++k) {
        float v[3] = {0.0f, 0.0f, 0.0f};
        int used = 0;
        if (sscanf(q, "%f,%f,%f%n", &v[0], &v[1], &v[2], &used) != 3) return q;
        for (int i = 0; i < 3; ++i)
            if (v[i] != v[i] || isinf(v[i])) return q;
        if (k == 3 && v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f) return q;
        for (int i = 0; i < 3; ++i) dst[k][i] = v[i];
        q += used;
        if (*q == ';') { if (!q[1]) return q; ++q; }
        else if (*q) return q;
    }
    return (k < 3 || *q) ? q : nullptr;
}

// --sky-sh FILE: 27 numbers separated by white space, sh[i][c] with the channel running fastest (the table of vct_set_sky);
// finite, and nothing but white space behind them.  Returns false when the file is unreadable or is not that.
static inline bool vct_demo_read_sky_sh(const char* path, float sh[9][3]) {
    FILE* f = fopen(path, "r");
    if (!f) return false;
    bool ok = true;
    for (int i = 0; i < 27 && ok; ++i) {
        float v = 0.0f;
        ok = fscanf(f, "%f", &v) == 1 && v == v && !isinf(v);
        sh[i / 3][i % 3] = v;
    }
    char extra;
    if (ok && fscanf(f, " %c", &extra) == 1) ok = false;
    fclose(f);
    return ok;
}

// --light X,Y,Z;R,G,B;RADIUS;SRC[;DX,DY,DZ;INNER_DEG;OUTER_DEG]: one point light -- position and colour, the radius it
// reaches and its source radius -- or, with the three further fields, a spot light: axis and the inner and outer half angle
// in degrees (0 <= inner < outer <= 180).  The values are checked against the contract of vct_set_lights.  Returns null
// or the place in the text where it stops making sense.
static inline const char* vct_demo_parse_light(const char* text, vct_light& out) {
    out = vct_light{};
    const char* q = text;
    int used = 0;
    auto sep = [&]() { if (*q != ';' || !q[1]) return false; ++q; return true; };
    auto finite = [](float v) { return v == v && !isinf(v); };
    if (sscanf(q, "%f,%f,%f%n", &out.position[0], &out.position[1], &out.position[2], &used) != 3) return q;
    q += used;
    if (!sep()) return q;
    if (sscanf(q, "%f,%f,%f%n", &out.color[0], &out.color[1], &out.color[2], &used) != 3) return q;
    for (int i = 0; i < 3; ++i)
        if (!finite(out.position[i]) || !finite(out.color[i]) || out.color[i] < 0.0f) return q;
    q += used;
    if (!sep()) return q;
    if (sscanf(q, "%f%n", &out.radius, &used) != 1 || !finite(out.radius) || !(out.radius > 0.0f)) return q;
    q += used;
    if (!sep()) return q;
    if (sscanf(q, "%f%n", &out.source_radius, &used) != 1 || !finite(out.source_radius) || !(out.source_radius > 0.0f)) return q;
    q += used;
    if (!*q) return nullptr;                       // a point light
    if (!sep()) return q;
    if (sscanf(q, "%f,%f,%f%n", &out.direction[0], &out.direction[1], &out.direction[2], &used) != 3) return q;
    const float len = sqrtf((out.direction[0] * out.direction[0] + out.direction[1] * out.direction[1]) + out.direction[2] * out.direction[2]);
    if (!finite(len) || !(len > 0.0f)) return q;
    q += used;
    if (!sep()) return q;
    float inner = 0.0f, outer = 0.0f;
    if (sscanf(q, "%f%n", &inner, &used) != 1 || !finite(inner)) return q;
    q += used;
    if (!sep()) return q;
    if (sscanf(q, "%f%n", &outer, &used) != 1 || !finite(outer) || !(0.0f <= inner && inner < outer && outer <= 180.0f)) return q;
    q += used;
    if (*q) return q;
    out.cos_inner = cosf(inner * 0.017453292519943295f);
    out.cos_outer = cosf(outer * 0.017453292519943295f);
    if (!(out.cos_outer < out.cos_inner)) return text;      // angles too close to tell apart in fp32
    out.flags = VCT_LIGHT_SPOT;
    return nullptr;
}

// --dynamic-draw shadow|gbuffer|both: the stages that draw the --dynamic-obj mesh (vct_set_dynamic_draw).  Returns the
// VCT_DYNAMIC_DRAW_* flags, or -1 for any other word.
#define VCT_DEMO_DYNAMIC_DRAW_USAGE "--dynamic-draw shadow|gbuffer|both (with --dynamic-obj): draw the dynamic mesh into the shadow map, the G-buffer or both"
static inline int vct_demo_parse_dynamic_draw(const char* word) {
    if (!word) return -1;
    if (!strcmp(word, "shadow")) return VCT_DYNAMIC_DRAW_SHADOW;
    if (!strcmp(word, "gbuffer")) return VCT_DYNAMIC_DRAW_GBUFFER;
    if (!strcmp(word, "both")) return VCT_DYNAMIC_DRAW_SHADOW | VCT_DYNAMIC_DRAW_GBUFFER;
    return -1;
}

// --dynamic-emission MATERIAL=R,G,B[;MATERIAL=R,G,B...]: emission of the listed materials of the --dynamic-obj mesh, the
// grammar of --emission, over `table` [nmat][3] (which holds the MTL file's Ke on entry).  Material indices below nmat,
// values finite and >= 0 (the contract of vct_set_dynamic_emission).  Returns null or the offending place.
#define VCT_DEMO_DYNAMIC_EMISSION_USAGE "--dynamic-emission MATERIAL=R,G,B[;...] (with --dynamic-obj): finite values >= 0, material indices of the dynamic OBJ"
static inline const char* vct_demo_parse_dynamic_emission(const char* list, int nmat, std::vector<float>& table) {
    if (!list || !*list) return list ? list : "";
    for (const char* q = list; *q;) {
        int m = -1, used = 0;
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (sscanf(q, "%d=%f,%f,%f%n", &m, &v[0], &v[1], &v[2], &used) != 4 || m < 0 || m >= nmat) return q;
        for (int k = 0; k < 3; ++k)
            if (!(v[k] >= 0.0f) || isinf(v[k])) return q;
        for (int k = 0; k < 3; ++k) table[(size_t)m * 3 + k] = v[k];
        q += used;
        if (*q == ';') { if (!q[1]) return q; ++q; }
        else if (*q) return q;
    }
    return nullptr;
}

// --dynamic-smooth: the --dynamic-obj mesh drawn with the corner normals of its file (vct_set_dynamic_normals) instead of
// face normals.  Only a mesh that is drawn into the G-buffer shows them, so anything else is a usage error.  Returns
// what is wrong, or null.
#define VCT_DEMO_DYNAMIC_SMOOTH_USAGE "--dynamic-smooth (with --dynamic-obj and --dynamic-draw gbuffer|both): the OBJ's vertex normals on the drawn mesh"
static inline const char* vct_demo_check_dynamic_smooth(bool have_obj, int draw_flags) {
    if (!have_obj) return "--dynamic-smooth: needs --dynamic-obj";
    if (draw_flags < 0 || !(draw_flags & VCT_DYNAMIC_DRAW_GBUFFER)) return "--dynamic-smooth: needs --dynamic-draw gbuffer|both";
    return nullptr;
}

// --dynamic-spin AX,AY,AZ;DEG_PER_FRAME: the --dynamic-obj mesh as ONE rigid part (vct_set_dynamic_parts), moved by a
// 3 x 4 matrix per frame (vct_update_dynamic_transforms) instead of a position array per frame: a rotation about the axis
// through the object's bounding-box centre.  Finite numbers, the axis not zero.  Returns false for anything else.
#define VCT_DEMO_DYNAMIC_SPIN_USAGE "--dynamic-spin AX,AY,AZ;DEG_PER_FRAME (with --dynamic-obj): finite numbers, a non-zero axis"
static inline bool vct_demo_parse_dynamic_spin(const char* text, double axis[3], double* deg_per_frame) {
    if (!text) return false;
    int used = 0;
    if (sscanf(text, "%lf,%lf,%lf;%lf%n", &axis[0], &axis[1], &axis[2], deg_per_frame, &used) != 4 || text[used]) return false;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(axis[k])) return false;
    if (!std::isfinite(*deg_per_frame)) return false;
    const double len = sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
    if (!std::isfinite(len) || !(len > 0.0)) return false;
    for (int k = 0; k < 3; ++k) axis[k] /= len;
    return true;
}

// The matrix of one frame, rows first: x -> R (x - centre) + centre + translation, R the rotation by `degrees` about the
// unit `axis` (Rodrigues), built in double and rounded once.
static inline void vct_demo_spin_matrix(const double axis[3], double degrees, const double centre[3], const double translation[3],
                                        float m[12]) {
    const double t = degrees * 0.017453292519943295, c = cos(t), s = sin(t), u = 1.0 - c;
    const double x = axis[0], y = axis[1], z = axis[2];
    const double R[3][3] = {{c + x * x * u, x * y * u - z * s, x * z * u + y * s},
                            {y * x * u + z * s, c + y * y * u, y * z * u - x * s},
                            {z * x * u - y * s, z * y * u + x * s, c + z * z * u}};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) m[4 * r + k] = (float)R[r][k];
        m[4 * r + 3] = (float)(centre[r] - ((R[r][0] * centre[0] + R[r][1] * centre[1]) + R[r][2] * centre[2]) + translation[r]);
    }
}

// --dynamic-bend AX,AY,AZ;DEG_PER_FRAME: the --dynamic-obj mesh skinned to TWO bones (vct_set_dynamic_skin) -- bone 0 the
// identity, bone 1 a rotation about the axis through the object's bounding-box centre that grows by DEG_PER_FRAME per
// frame -- so that the object bends along its longest axis.  The grammar and the checks are the spin's; the two exclude
// each other.
#define VCT_DEMO_DYNAMIC_BEND_USAGE "--dynamic-bend AX,AY,AZ;DEG_PER_FRAME (with --dynamic-obj, not with --dynamic-spin): finite numbers, a non-zero axis"
static inline bool vct_demo_parse_dynamic_bend(const char* text, double axis[3], double* deg_per_frame) {
    return vct_demo_parse_dynamic_spin(text, axis, deg_per_frame);
}

// The influences of the bend for positions [ntri][9] with bounding box lo .. hi: per corner bones (0, 1, 0, 0) and weights
// (w0, w1, 0, 0) with w1 = clamp((c - lo) / (hi - lo), 0, 1) along the box's longest axis (c the corner's coordinate) and
// w0 = 1 - w1.  The unused slots point at bone 0, which is in use.  A box without extent: w1 = 0.
static inline void vct_demo_bend_influences(const float* pos, size_t ntri, const float lo[3], const float hi[3],
                                            std::vector<int32_t>& bone, std::vector<float>& weight) {
    int axis = 0;
    for (int k = 1; k < 3; ++k)
        if (hi[k] - lo[k] > hi[axis] - lo[axis]) axis = k;
    const float extent = hi[axis] - lo[axis];
    bone.assign(ntri * 12, 0);
    weight.assign(ntri * 12, 0.0f);
    for (size_t v = 0; v < ntri * 3; ++v) {
        float w1 = extent > 0.0f ? (pos[3 * v + axis] - lo[axis]) / extent : 0.0f;
        w1 = w1 < 0.0f ? 0.0f : (w1 > 1.0f ? 1.0f : w1);
        bone[4 * v + 1] = 1;
        weight[4 * v] = 1.0f - w1;
        weight[4 * v + 1] = w1;
    }
}

#endif
