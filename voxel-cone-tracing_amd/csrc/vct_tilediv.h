// vct_tilediv.h -- what the host works out once per launch so that the tile kernels need not: the exact division of a tile
// index by tiles_x as a multiply-high and a shift, and the unit vector of the light direction.  Host and device, no HIP
// call and no exported symbol, so that a host program can run both under the sanitizers (tests/tilediv_check_main.cpp).
#ifndef VCT_TILEDIV_H_
#define VCT_TILEDIV_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VCT_TILEDIV_HD __host__ __device__ __forceinline__
#else
#define VCT_TILEDIV_HD static inline
#endif

// ---- n / d for a launch-constant divisor d --------------------------------------------------------------------------------
// q = mulhi(n, mul) >> shift with mul = ceil(2^(31 + l) / d), l = ceil(log2 d), shift = l - 1 (Granlund & Montgomery 1994,
// theorem 4.2 with N = 31).  Write mul * d = 2^(31 + l) + e: 0 <= e < d <= 2^l by construction, and for n = q0 * d + r
//     n * mul / 2^(31 + l) = q0 + r / d + n * e / (d * 2^(31 + l)) < q0 + 1   whenever   n * e < 2^(31 + l),
// which e < 2^l gives for every n < 2^31.  Tile indices are non-negative ints, so 2^31 bounds every n a kernel can form;
// vct_create accepts any positive int32 width, so d = tiles_x ranges over 1 .. 2^28 (VCT_TILEDIV_MAX_D), and
// mul < 2^(31 + l) / 2^(l - 1) + 1 = 2^32 + 1 fits 32 bits for all of them but the powers of two's own edge d = 1
// (l = 0: no shift of -1).  The host certifies a divisor by checking the inequalities above in 64-bit arithmetic -- not
// by trusting the construction -- and a divisor it cannot certify (d = 1, d > VCT_TILEDIV_MAX_D) gets mul = 0: the plain
// division, behind a wave-uniform branch.
#define VCT_TILEDIV_MAX_N 0x80000000u        // exclusive bound of the dividends the certificate covers
#define VCT_TILEDIV_MAX_D 0x10000000u        // tiles_x of the widest frame vct_create accepts: ceil((2^31 - 1) / 8)

struct VctTileDiv {
    uint32_t mul;          // 0: not certified, divide
    uint32_t shift;
};

static inline VctTileDiv vct_tilediv_make(uint32_t d) {
    VctTileDiv t = {0u, 0u};
    if (d < 2u || d > VCT_TILEDIV_MAX_D) return t;
    uint32_t l = 0;
    while (((uint64_t)1 << l) < d) ++l;                                  // ceil(log2 d), 1 .. 28
    const uint64_t pow = (uint64_t)1 << (31u + l);
    const uint64_t mul = (pow + d - 1u) / d;
    const uint64_t e = mul * d - pow;                                    // mul * d < 2^60: no overflow
    // the certificate: mul fits, and (VCT_TILEDIV_MAX_N - 1) * e < 2^(31 + l)
    if (mul > 0xffffffffull || e >= d || (uint64_t)(VCT_TILEDIV_MAX_N - 1u) * e >= pow) return t;
    t.mul = (uint32_t)mul;
    t.shift = l - 1u;
    return t;
}

// n / d, for n < VCT_TILEDIV_MAX_N and (mul, shift) = vct_tilediv_make(d).  The 64-bit product's high word is one
// v_mul_hi_u32, or s_mul_hi_u32 where n is wave-uniform.
VCT_TILEDIV_HD uint32_t vct_tilediv(uint32_t n, uint32_t d, uint32_t mul, uint32_t shift) {
    if (mul == 0u) return n / d;
    return (uint32_t)(((uint64_t)n * mul) >> 32) >> shift;
}

// ---- the light direction, normalised once per launch ------------------------------------------------------------------------
// normalize(LightDirection) of trace.fs:179 with the oracle's operations in the oracle's order, every one of them a
// correctly rounded fp32 operation on the host as on the device (build with -ffp-contract=off): the bits are those the
// composite used to compute per pixel.  A zero vector gives 0 / 0 = NaN in all three components, as it did there.
static inline void vct_light_unit(const float light[3], float unit[3]) {
    const float l = sqrtf((light[0] * light[0] + light[1] * light[1]) + light[2] * light[2]);
    unit[0] = light[0] / l;
    unit[1] = light[1] / l;
    unit[2] = light[2] / l;
}

#endif
