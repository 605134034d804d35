// vct_emission_check.h -- the table check of vct_upload_emission (vct_api_emission.hip) and the padding of the table to
// the colour-table stride of the voxelizer, free of any HIP call so that a host program can run them under the
// sanitizers (tests/emission_check_main.cpp).
#ifndef VCT_EMISSION_CHECK_H_
#define VCT_EMISSION_CHECK_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define VCT_EMISSION_OK 0          // finite, >= 0, at least one value above 0
#define VCT_EMISSION_ZERO 1        // every value is +0 or -0: counts as detached
#define VCT_EMISSION_BAD (-1)      // a value is NaN, infinite or below 0: *bad_index names the first one

// emission: [nmat][3].  nmat <= 0 is a table without values: VCT_EMISSION_ZERO.
static inline int vct_emission_check(const float* emission, int32_t nmat, size_t* bad_index) {
    bool any = false;
    const size_t n = nmat > 0 ? (size_t)nmat * 3 : 0;
    for (size_t i = 0; i < n; ++i) {
        const float v = emission[i];
        if (!(v >= 0.0f) || isinf(v)) {      // (NaN fails the comparison)
            if (bad_index) *bad_index = i;
            return VCT_EMISSION_BAD;
        }
        any = any || v > 0.0f;
    }
    return any ? VCT_EMISSION_OK : VCT_EMISSION_ZERO;
}

// [nmat][3] -> [nmat][4] (rgb, 0): the stride of the voxelizer's colour table; out holds nmat * 4 floats
static inline void vct_emission_pad(const float* emission, int32_t nmat, float* out) {
    for (int32_t m = 0; m < nmat; ++m) {
        for (int k = 0; k < 3; ++k) out[(size_t)m * 4 + k] = emission[(size_t)m * 3 + k];
        out[(size_t)m * 4 + 3] = 0.0f;
    }
}

#endif
