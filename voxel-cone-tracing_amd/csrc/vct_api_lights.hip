// vct_api_lights.hip -- the C ABI of local lights (include/vct.h "local lights"): the context's point and spot lights,
// their folded table on the device, and the lit planes of the frame slots.
#include "vct_ctx.h"
#include "vct_lights_check.h"

// three planes, tiled like the emission planes; fresh planes have not been filled: their timer starts over
hipError_t vct_lights_planes(const vct_ctx* c, VctFrameSlot& s, bool* fresh) {
    bool made = false;
    const hipError_t e = vct_planes_ensure(s.lit, vct_emis_tiled_floats(c), s.stream.get(), &made);
    if (made) s.lit_timer = VctTimer();
    if (fresh) *fresh = made;
    return e;
}
static void lights_planes_drop(VctFrameSlot& s) { s.lit.reset(); s.lit_timer = VctTimer(); }

// no lights from here on; the caller has made sure nothing in flight reads the table or the planes
static void lights_detach(vct_ctx* c) {
    c->lights = VctLights();
    for (VctFrameSlot& sl : c->slots) lights_planes_drop(sl);
}

extern "C" {

int vct_set_lights(vct_ctx* c, const vct_light* lights, int32_t n) {
    if (!c) return VCT_ERR_INVALID;
    if (n < 0 || n > VCT_LIGHTS_MAX) return vct_fail(c, VCT_ERR_INVALID, "vct_set_lights: 0 <= n <= VCT_LIGHTS_MAX (64)");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!lights || n == 0) {      // detached: no table, no planes, the launches of a context that never had lights
        if (!c->lights.n) return VCT_OK;
        PIPE_TRY(vct_synchronize(c));         // a kernel in flight may still read the table or the planes
        lights_detach(c);
        return VCT_OK;
    }
    int32_t bad = 0;
    const char* why = nullptr;
    if (vct_lights_check(lights, n, &bad, &why) != VCT_LIGHTS_OK) {
        char msg[160];
        snprintf(msg, sizeof msg, "vct_set_lights: light %d: %s", (int)bad, why);
        return vct_fail(c, VCT_ERR_INVALID, msg);
    }
    if (!c->cfg.voxel_attributes)
        return vct_fail(c, VCT_ERR_INVALID, "vct_set_lights: needs config.voxel_attributes = 1 (the voxels' albedo and normal)");
    PIPE_TRY(vct_refuse_conflict(c, "vct_set_lights", VCT_FEAT_LIGHTS, vct_rules_in_force(c).modes));
    VctLightDev folded[VCT_LIGHTS_MAX] = {};
    for (int32_t i = 0; i < n; ++i) vct_light_fold(&lights[i], &folded[i]);
    PIPE_TRY(vct_synchronize(c));             // the table about to be rewritten may still be read
    // all or nothing: a fresh table in a local, planes only for slots that have none
    VctBuf<VctLightDev> table;
    PIPE_TRY(vct_planes_attach(c, "vct_set_lights", vct_lights_planes, lights_planes_drop, c->lights.table ? hipSuccess : table.alloc(VCT_LIGHTS_MAX)));
    const hipError_t e = hipMemcpy(table ? table.get() : c->lights.table.get(), folded, sizeof folded, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        // a failed copy into the table the context already had leaves lights attached whose table is undefined; a context
        // without a table had no lights and no lit planes, so that every plane there is now is this call's: detach either way
        lights_detach(c);
        HIP_TRY(c, e);
    }
    if (table) c->lights.table = std::move(table);
    c->lights.n = n;
    memset(c->lights.given, 0, sizeof c->lights.given);
    memcpy(c->lights.given, lights, (size_t)n * sizeof(vct_light));
    return VCT_OK;
}

int vct_get_lights(const vct_ctx* c, vct_light out[VCT_LIGHTS_MAX], int32_t* n) {
    if (!c) return VCT_ERR_INVALID;
    if (out) memcpy(out, c->lights.given, sizeof c->lights.given);
    if (n) *n = c->lights.n;
    return VCT_OK;
}

int vct_download_pixel_lights(vct_ctx* c, float* planes) {
    if (!c || !planes) return VCT_ERR_INVALID;
    VctFrameSlot& s = cur(c);
    if (!s.lit || !s.lit_timer.have)
        return vct_fail(c, VCT_ERR_INVALID, "vct_download_pixel_lights: no composite launch with lights attached has run on this frame slot");
    HIP_TRY(c, hipSetDevice(c->device));
    return vct_planes_download(c, s.lit.get(), planes, VCT_EMIS_NPLANES, sizeof(float));
}

int vct_last_lights_ms(vct_ctx* c, float ms[2]) {
    if (!c || !ms) return VCT_ERR_INVALID;
    const VctFrameSlot& s = cur(c);
    const char* never = "vct_last_lights_ms: needs lights attached, a vct_inject_light and a composite launch on this frame slot since";
    const char* untimed = "vct_last_lights_ms: the last kernels were issued with timing off (vct_set_trace_timing)";
    if (!c->lights.n || !s.lit_timer.have) return vct_fail(c, VCT_ERR_INVALID, never);      // (both have run before either is asked for its time)
    PIPE_TRY(vct_timer_ms(c, c->lights.vox_timer, &ms[0], never, untimed));
    return vct_timer_ms(c, s.lit_timer, &ms[1], never, untimed);
}

}  // extern "C"
