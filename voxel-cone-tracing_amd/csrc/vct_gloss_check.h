// vct_gloss_check.h -- the table check of vct_set_gloss_classes and the copy of vct_upload_material_gloss's map
// (vct_api_gloss.hip), free of any HIP call so that a host program can run them under the sanitizers
// (tests/gloss_check_main.cpp).
#ifndef VCT_GLOSS_CHECK_H_
#define VCT_GLOSS_CHECK_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vct.h"

#define VCT_GLOSS_OK 0
#define VCT_GLOSS_DETACH 1          // NULL table or nclasses == 0: detaches
#define VCT_GLOSS_BAD_COUNT (-1)    // nclasses outside [1, VCT_GLOSS_CLASSES_MAX]
#define VCT_GLOSS_BAD_VALUE (-2)    // a class outside the contract: *bad_index names the first one

// classes: [nclasses].  Contract: tan_specular finite and > 0, shininess finite and >= 0.  Nothing is read from the table
// unless the count is inside [1, VCT_GLOSS_CLASSES_MAX].
static inline int vct_gloss_check_classes(const vct_gloss_class* classes, int32_t nclasses, int32_t* bad_index) {
    if (!classes || nclasses == 0) return VCT_GLOSS_DETACH;
    if (nclasses < 1 || nclasses > VCT_GLOSS_CLASSES_MAX) return VCT_GLOSS_BAD_COUNT;
    for (int32_t k = 0; k < nclasses; ++k) {
        const float t = classes[k].tan_specular, s = classes[k].shininess;
        if (!(t > 0.0f) || isinf(t) || !(s >= 0.0f) || isinf(s)) {      // (NaN fails the comparisons)
            if (bad_index) *bad_index = k;
            return VCT_GLOSS_BAD_VALUE;
        }
    }
    return VCT_GLOSS_OK;
}

// bytes the material map of a mesh with nmat materials holds: nmat <= 0 is a map without values
static inline size_t vct_gloss_map_bytes(int32_t nmat) { return nmat > 0 ? (size_t)nmat : 0; }

// mat_class[nmat] -> out[nmat], as given: a value >= nclasses is kept, the trace clamps what it reads
static inline void vct_gloss_map_copy(const uint8_t* mat_class, int32_t nmat, uint8_t* out) {
    const size_t n = vct_gloss_map_bytes(nmat);
    for (size_t i = 0; i < n; ++i) out[i] = mat_class[i];
}

#endif
