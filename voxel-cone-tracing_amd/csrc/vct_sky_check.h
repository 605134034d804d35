// vct_sky_check.h -- the table check of vct_set_sky (vct_api_sky.hip), the folding of the basis constants into the
// coefficients and the evaluation chain of include/vct.h "sky light", free of any HIP call so that a host program can
// run them under the sanitizers (tests/sky_check_main.cpp).
#ifndef VCT_SKY_CHECK_H_
#define VCT_SKY_CHECK_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define VCT_SKY_COEFFS 9
#define VCT_SKY_FLOATS (VCT_SKY_COEFFS * 3)

#define VCT_SKY_OK 0             // finite, at least one value that is not +0 or -0
#define VCT_SKY_DETACH 1         // NULL, or every value is +0 or -0: detaches
#define VCT_SKY_BAD (-1)         // a value is NaN or infinite: *bad_index names the first one

// sh: [9][3] or NULL.  Exactly 27 floats are read.
static inline int vct_sky_check(const float* sh, size_t* bad_index) {
    if (!sh) return VCT_SKY_DETACH;
    bool any = false;
    for (size_t i = 0; i < VCT_SKY_FLOATS; ++i) {
        const float v = sh[i];
        if (v != v || isinf(v)) {
            if (bad_index) *bad_index = i;
            return VCT_SKY_BAD;
        }
        any = any || v != 0.0f;
    }
    return any ? VCT_SKY_OK : VCT_SKY_DETACH;
}

// K_i of the orthonormal real basis, i = l(l+1)+m, over the polynomials 1, y, z, x, xy, yz, 3z^2-1, xz, x^2-y^2
static inline double vct_sky_basis_constant(int i) {
    static const double K[VCT_SKY_COEFFS] = {
        0.28209479177387814,                                              // sqrt(1/4pi)
        0.4886025119029199, 0.4886025119029199, 0.4886025119029199,        // sqrt(3/4pi)
        1.0925484305920792, 1.0925484305920792,                            // sqrt(15/4pi)
        0.31539156525252005,                                              // sqrt(5/16pi)
        1.0925484305920792,
        0.5462742152960396,                                               // sqrt(15/16pi)
    };
    return K[i];
}

// poly[i][c] = (float)(K_i * (double)sh[i][c]): what the device sees
static inline void vct_sky_fold(const float* sh, float* poly) {
    for (int i = 0; i < VCT_SKY_COEFFS; ++i)
        for (int c = 0; c < 3; ++c) poly[i * 3 + c] = (float)(vct_sky_basis_constant(i) * (double)sh[i * 3 + c]);
}

// sky radiance of the unit direction d, per channel: the chain of include/vct.h, in fp32, in exactly that order (the
// kernels' epilogue is the same chain: vct_trace.hip sky_epilogue).  Build with -ffp-contract=off.
static inline void vct_sky_eval(const float* poly, const float d[3], float out[3]) {
    const float x = d[0], y = d[1], z = d[2];
    const float xy = x * y, yz = y * z, zz = fmaf(3.0f * z, z, -1.0f), xz = x * z, xxyy = fmaf(x, x, -(y * y));
    for (int c = 0; c < 3; ++c) {
        float s = poly[0 * 3 + c];
        s = fmaf(poly[1 * 3 + c], y, s);
        s = fmaf(poly[2 * 3 + c], z, s);
        s = fmaf(poly[3 * 3 + c], x, s);
        s = fmaf(poly[4 * 3 + c], xy, s);
        s = fmaf(poly[5 * 3 + c], yz, s);
        s = fmaf(poly[6 * 3 + c], zz, s);
        s = fmaf(poly[7 * 3 + c], xz, s);
        s = fmaf(poly[8 * 3 + c], xxyy, s);
        out[c] = fmaxf(s, 0.0f);
    }
}

#endif
