// vct_demo_options.h -- the list options of vct_demo that are parsed before anything touches a GPU, so that a malformed
// list ends the program with exit status 1 on any machine (tests/test_gloss_restatement.py).
#ifndef VCT_DEMO_OPTIONS_H_
#define VCT_DEMO_OPTIONS_H_

#include <math.h>
#include <stdio.h>

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

#endif
