// vct_api_sky.hip -- the C ABI of sky light (include/vct.h "sky light"): the context's one spherical-harmonic sky, its
// folded polynomial form on the device.
#include "vct_ctx.h"
#include "vct_sky_check.h"

extern "C" {

int vct_set_sky(vct_ctx* c, const float sh[9][3]) {
    if (!c) return VCT_ERR_INVALID;
    const float* table = sh ? &sh[0][0] : nullptr;
    size_t bad = 0;
    const int verdict = vct_sky_check(table, &bad);
    if (verdict == VCT_SKY_BAD) {
        char msg[160];
        snprintf(msg, sizeof msg, "vct_set_sky: channel %zu of coefficient %zu (%g) is not finite", bad % 3, bad / 3, (double)table[bad]);
        return vct_fail(c, VCT_ERR_INVALID, msg);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (verdict == VCT_SKY_DETACH) {          // NULL or all zero: no sky forms launched, no cost
        if (!c->sky.attached) return VCT_OK;
        PIPE_TRY(vct_synchronize(c));         // a trace in flight may still read the coefficients
        c->sky = VctSky();
        return VCT_OK;
    }
    PIPE_TRY(vct_refuse_conflict(c, "vct_set_sky", VCT_FEAT_SKY, vct_rules_in_force(c).modes));
    float poly[VCT_SKY_FLOATS];
    vct_sky_fold(table, poly);
    PIPE_TRY(vct_synchronize(c));             // the coefficients about to be rewritten may still be read
    // all or nothing: a fresh device table in a local until it is filled
    VctBuf<float> dev;
    if (!c->sky.poly_dev) HIP_TRY(c, dev.alloc(VCT_SKY_DEV_FLOATS));
    float* dst = c->sky.poly_dev ? c->sky.poly_dev.get() : dev.get();
    float padded[VCT_SKY_DEV_FLOATS] = {};
    memcpy(padded, poly, sizeof poly);
    HIP_TRY(c, hipMemcpy(dst, padded, sizeof padded, hipMemcpyHostToDevice));
    if (dev) c->sky.poly_dev = std::move(dev);
    memcpy(c->sky.sh, table, sizeof c->sky.sh);
    memcpy(c->sky.poly, poly, sizeof c->sky.poly);
    c->sky.attached = true;
    return VCT_OK;
}

int vct_get_sky(const vct_ctx* c, float sh[9][3], float poly[9][3], int32_t* attached) {
    if (!c) return VCT_ERR_INVALID;
    if (sh) memcpy(&sh[0][0], c->sky.sh, sizeof c->sky.sh);
    if (poly) memcpy(&poly[0][0], c->sky.poly, sizeof c->sky.poly);
    if (attached) *attached = c->sky.attached ? 1 : 0;
    return VCT_OK;
}

}  // extern "C"
