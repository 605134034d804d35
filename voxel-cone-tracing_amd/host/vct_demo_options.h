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

#endif
