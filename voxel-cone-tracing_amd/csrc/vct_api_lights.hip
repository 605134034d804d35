// vct_api_lights.hip -- the C ABI of local lights (include/vct.h "local lights"): the context's point and spot lights,
// their folded table on the device, and the lit planes of the frame slots.
#include "vct_ctx.h"
#include "vct_lights_check.h"

// zeroed lit planes and the timing events around their kernel for a slot that has none, on the slot's stream
hipError_t vct_lights_planes(const vct_ctx* c, VctFrameSlot& s) {
    if (s.lit) return hipSuccess;
    const size_t n = vct_emis_tiled_floats(c);      // three planes, tiled like the emission planes
    hipError_t e = s.lit.alloc(n);
    if (e == hipSuccess) e = hipMemsetAsync(s.lit.get(), 0, n * sizeof(float), s.stream.get());
    if (e == hipSuccess) e = s.lit_ev0.create();
    if (e == hipSuccess) e = s.lit_ev1.create();
    if (e != hipSuccess) { s.lit.reset(); s.lit_ev0.reset(); s.lit_ev1.reset(); }
    s.have_lit = false;
    return e;
}

// no lights from here on; the caller has made sure nothing in flight reads the table or the planes
static void lights_detach(vct_ctx* c) {
    c->lights = VctLights();
    for (VctFrameSlot& sl : c->slots) {
        sl.lit.reset(); sl.lit_ev0.reset(); sl.lit_ev1.reset();
        sl.have_lit = sl.lit_timed = false;
    }
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
    if (c->cfg.trace_variant != 0)
        return vct_fail(c, VCT_ERR_INVALID, "vct_set_lights: config.trace_variant 1 .. 4 has no pixel-emission planes to carry the lit planes");
    VctLightDev folded[VCT_LIGHTS_MAX] = {};
    for (int32_t i = 0; i < n; ++i) vct_light_fold(&lights[i], &folded[i]);
    PIPE_TRY(vct_synchronize(c));             // the table about to be rewritten may still be read
    // all or nothing: a fresh table and fresh events in locals, planes only for slots that have none (released on a failure)
    VctBuf<VctLightDev> table;
    VctEvent ev0, ev1;
    bool fresh_planes[2] = {false, false};
    hipError_t e = hipSuccess;
    if (!c->lights.table) {
        e = table.alloc(VCT_LIGHTS_MAX);
        if (e == hipSuccess) e = ev0.create();
        if (e == hipSuccess) e = ev1.create();
    }
    for (int k = 0; k < c->frames_in_flight && e == hipSuccess; ++k) {
        fresh_planes[k] = !c->slots[k].lit;
        e = vct_lights_planes(c, c->slots[k]);
        if (e == hipSuccess) e = hipStreamSynchronize(c->slots[k].stream.get());
    }
    if (e == hipSuccess)
        e = hipMemcpy(table ? table.get() : c->lights.table.get(), folded, sizeof folded, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        // (a failed copy into the table the context already had leaves lights attached whose table is undefined: detach)
        const bool own_table_hit = !table && c->lights.table;
        for (int k = 0; k < 2; ++k)
            if (fresh_planes[k]) { c->slots[k].lit.reset(); c->slots[k].lit_ev0.reset(); c->slots[k].lit_ev1.reset(); }
        if (own_table_hit) lights_detach(c);
        return vct_fail(c, e == hipErrorOutOfMemory ? VCT_ERR_NOMEM : VCT_ERR_DEVICE, std::string("vct_set_lights: ") + hipGetErrorString(e));
    }
    if (table) {
        c->lights.table = std::move(table);
        c->lights.ev0 = std::move(ev0);
        c->lights.ev1 = std::move(ev1);
    }
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
    if (!s.lit || !s.have_lit)
        return vct_fail(c, VCT_ERR_INVALID, "vct_download_pixel_lights: no composite launch with lights attached has run on this frame slot");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npix = (size_t)c->cfg.width * c->cfg.height;
    PIPE_TRY(vct_staging_free(c));
    HIP_TRY(c, c->gb_linear.reserve(npix * VCT_GB_NPLANES));
    HIP_TRY(c, vct_launch_untile_emission(s.lit.get(), c->gb_linear.get(), c->cfg.width, c->cfg.height, s.stream.get()));
    HIP_TRY(c, hipMemcpyAsync(planes, c->gb_linear.get(), npix * VCT_EMIS_NPLANES * sizeof(float), hipMemcpyDeviceToHost, s.stream.get()));
    HIP_TRY(c, hipStreamSynchronize(s.stream.get()));
    return VCT_OK;
}

int vct_last_lights_ms(vct_ctx* c, float ms[2]) {
    if (!c || !ms) return VCT_ERR_INVALID;
    const VctFrameSlot& s = cur(c);
    if (!c->lights.n || !c->lights.vox_have || !s.have_lit)
        return vct_fail(c, VCT_ERR_INVALID, "vct_last_lights_ms: needs lights attached, a vct_inject_light and a composite launch on this frame slot since");
    if (!c->lights.vox_timed || !s.lit_timed)
        return vct_fail(c, VCT_ERR_INVALID, "vct_last_lights_ms: the last kernels were issued with timing off (vct_set_trace_timing)");
    HIP_TRY(c, hipEventSynchronize(c->lights.ev1.get()));
    HIP_TRY(c, hipEventElapsedTime(&ms[0], c->lights.ev0.get(), c->lights.ev1.get()));
    HIP_TRY(c, hipEventSynchronize(s.lit_ev1.get()));
    HIP_TRY(c, hipEventElapsedTime(&ms[1], s.lit_ev0.get(), s.lit_ev1.get()));
    return VCT_OK;
}

}  // extern "C"
