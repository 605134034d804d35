// vct_api_gloss.hip -- the C ABI of per-material gloss (include/vct.h "per-material gloss"): the class table with its step
// tables, the material map of the mesh, and the pixel-gloss plane of a frame slot.
#include "vct_ctx.h"
#include "vct_gloss_check.h"

// a zeroed plane for a slot that has none, on the slot's stream
hipError_t vct_gloss_plane(const vct_ctx* c, VctFrameSlot& s) {
    if (s.gloss) return hipSuccess;
    hipError_t e = s.gloss.alloc(vct_gloss_tiled_bytes(c));
    if (e == hipSuccess) e = hipMemsetAsync(s.gloss.get(), 0, vct_gloss_tiled_bytes(c), s.stream.get());
    if (e != hipSuccess) s.gloss.reset();
    return e;
}

// The caller has made sure nothing in flight reads the map (vct_pipeline_drain + the selected stream).
void vct_material_gloss_detach(vct_ctx* c) { c->mesh.mat_gloss.reset(); }

extern "C" {

int vct_set_gloss_classes(vct_ctx* c, const vct_gloss_class* classes, int32_t nclasses) {
    if (!c) return VCT_ERR_INVALID;
    int32_t bad = 0;
    const int verdict = vct_gloss_check_classes(classes, nclasses, &bad);
    if (verdict == VCT_GLOSS_BAD_COUNT) return vct_fail(c, VCT_ERR_INVALID, "vct_set_gloss_classes: nclasses outside [1, VCT_GLOSS_CLASSES_MAX]");
    if (verdict == VCT_GLOSS_BAD_VALUE) {
        char msg[160];
        snprintf(msg, sizeof msg, "vct_set_gloss_classes: class %d (tan_specular %g, shininess %g): tan_specular must be finite and > 0, shininess finite and >= 0",
                 (int)bad, (double)classes[bad].tan_specular, (double)classes[bad].shininess);
        return vct_fail(c, VCT_ERR_INVALID, msg);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (verdict == VCT_GLOSS_DETACH) {
        if (!c->gloss.n) return VCT_OK;
        PIPE_TRY(vct_synchronize(c));           // a trace in flight may still read the tables and the planes
        c->gloss = VctGloss();
        for (VctFrameSlot& sl : c->slots) sl.gloss.reset();
        return VCT_OK;
    }
    if (c->cfg.trace_variant != 0)
        return vct_fail(c, VCT_ERR_INVALID, "vct_set_gloss_classes: config.trace_variant 1 .. 4 has no gloss classes");
    if (c->cfg.anisotropic_mips)
        return vct_fail(c, VCT_ERR_INVALID, "vct_set_gloss_classes: config.anisotropic_mips has no gloss classes");
    if (c->vol.want_cells)
        return vct_fail(c, VCT_ERR_INVALID, "vct_set_gloss_classes: footprint records are on (vct_set_footprint_records(ctx, 0) first)");
    // every table once on the host: the limits are checked before anything changes
    int nsteps[VCT_GLOSS_CLASSES_MAX] = {};
    for (int k = 0; k < nclasses; ++k) {
        std::vector<VctStep> t;
        if (vct_build_steps(c->cfg, classes[k].tan_specular, t))
            return vct_fail(c, VCT_ERR_INVALID, "vct_set_gloss_classes: class " + std::to_string(k) + " needs more than VCT_MAX_STEPS march steps");
        if (c->cfg.debug_outputs && t.size() > 255)
            return vct_fail(c, VCT_ERR_INVALID, "vct_set_gloss_classes: debug_outputs keeps per-cone step counts as uint8: class " +
                                                std::to_string(k) + " needs more than 255 steps");
        nsteps[k] = (int)t.size();
    }
    PIPE_TRY(vct_synchronize(c));               // the tables about to be rewritten may still be read
    // all or nothing: the device table in a local, planes only for slots that have none (released again on a failure)
    VctBuf<VctGlossTable> table;
    bool fresh_plane[2] = {false, false};
    hipError_t e = c->gloss.table ? hipSuccess : table.alloc(1);
    for (int k = 0; k < c->frames_in_flight && e == hipSuccess; ++k) {
        fresh_plane[k] = !c->slots[k].gloss;
        e = vct_gloss_plane(c, c->slots[k]);
        if (e == hipSuccess) e = hipStreamSynchronize(c->slots[k].stream.get());
    }
    if (e != hipSuccess) {
        for (int k = 0; k < 2; ++k)
            if (fresh_plane[k]) c->slots[k].gloss.reset();
        return vct_fail(c, e == hipErrorOutOfMemory ? VCT_ERR_NOMEM : VCT_ERR_DEVICE, std::string("vct_set_gloss_classes: ") + hipGetErrorString(e));
    }
    if (table) c->gloss.table = std::move(table);
    c->gloss.n = nclasses;
    for (int k = 0; k < VCT_GLOSS_CLASSES_MAX; ++k) {
        c->gloss.cls[k] = k < nclasses ? classes[k] : vct_gloss_class{0.0f, 0.0f};
        c->gloss.nsteps[k] = nsteps[k];
    }
    // the tables go to the device now, with the context's one division verdict over all of them: a new divisor pays its
    // device check here and not in the first trace
    c->steps_dirty = true;
    return vct_refresh_steps(c);
}

int vct_get_gloss_classes(const vct_ctx* c, vct_gloss_class out[8], int32_t* nclasses, int32_t steps[8]) {
    if (!c) return VCT_ERR_INVALID;
    if (nclasses) *nclasses = c->gloss.n;
    for (int k = 0; k < VCT_GLOSS_CLASSES_MAX; ++k) {
        if (out) out[k] = c->gloss.cls[k];
        if (steps) steps[k] = k < c->gloss.n ? c->gloss.nsteps[k] : 0;
    }
    return VCT_OK;
}

int vct_upload_material_gloss(vct_ctx* c, const uint8_t* mat_class) {
    if (!c) return VCT_ERR_INVALID;
    if (!c->mesh.tri_pos) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_material_gloss: call vct_upload_triangles first");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_drain(c));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    if (c->fork.aux) HIP_TRY(c, hipStreamSynchronize(c->fork.aux.get()));      // vct_gi_pass shades on it
    if (!mat_class) {
        vct_material_gloss_detach(c);
        return VCT_OK;
    }
    const int32_t nmat = c->mesh.nmat;
    std::vector<uint8_t> map(vct_gloss_map_bytes(nmat) ? vct_gloss_map_bytes(nmat) : 1);
    vct_gloss_map_copy(mat_class, nmat, map.data());
    VctBuf<uint8_t> dev;
    HIP_TRY(c, dev.alloc(map.size()));
    HIP_TRY(c, hipMemcpy(dev.get(), map.data(), map.size(), hipMemcpyHostToDevice));
    c->mesh.mat_gloss = std::move(dev);
    return VCT_OK;
}

int vct_set_pixel_gloss(vct_ctx* c, const uint8_t* classes, int32_t layout, int32_t location) {
    if (!c) return VCT_ERR_INVALID;
    VctFrameSlot& s = cur(c);
    if (!c->gloss.n || !s.gloss) return vct_fail(c, VCT_ERR_INVALID, "vct_set_pixel_gloss: no gloss classes attached (vct_set_gloss_classes)");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!classes) {
        HIP_TRY(c, hipMemsetAsync(s.gloss.get(), 0, vct_gloss_tiled_bytes(c), s.stream.get()));
        return VCT_OK;
    }
    if (layout != VCT_GB_LINEAR && layout != VCT_GB_TILED) return vct_fail(c, VCT_ERR_INVALID, "vct_set_pixel_gloss: unknown layout");
    if (location != VCT_MEM_HOST && location != VCT_MEM_DEVICE) return vct_fail(c, VCT_ERR_INVALID, "vct_set_pixel_gloss: unknown location");
    const size_t npix = (size_t)c->cfg.width * c->cfg.height;
    if (layout == VCT_GB_TILED) {
        HIP_TRY(c, hipMemcpyAsync(s.gloss.get(), classes, vct_gloss_tiled_bytes(c),
                                  location == VCT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s.stream.get()));
    } else {
        const uint8_t* src = classes;
        if (location == VCT_MEM_HOST) {
            PIPE_TRY(vct_staging_free(c));
            HIP_TRY(c, c->gb_linear.reserve(npix * VCT_GB_NPLANES));
            HIP_TRY(c, hipMemcpyAsync(c->gb_linear.get(), classes, npix, hipMemcpyHostToDevice, s.stream.get()));
            src = (const uint8_t*)c->gb_linear.get();
        }
        HIP_TRY(c, vct_launch_tile_gloss(src, s.gloss.get(), c->cfg.width, c->cfg.height, s.stream.get()));
    }
    if (location == VCT_MEM_HOST) HIP_TRY(c, hipStreamSynchronize(s.stream.get()));      // the caller's memory is free again
    return VCT_OK;
}

int vct_download_pixel_gloss(vct_ctx* c, uint8_t* out) {
    if (!c || !out) return VCT_ERR_INVALID;
    if (!cur(c).gloss) return vct_fail(c, VCT_ERR_INVALID, "vct_download_pixel_gloss: no pixel-gloss plane (vct_set_gloss_classes)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npix = (size_t)c->cfg.width * c->cfg.height;
    PIPE_TRY(vct_staging_free(c));
    HIP_TRY(c, c->gb_linear.reserve(npix * VCT_GB_NPLANES));
    HIP_TRY(c, vct_launch_untile_gloss(cur(c).gloss.get(), (uint8_t*)c->gb_linear.get(), c->cfg.width, c->cfg.height, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(out, c->gb_linear.get(), npix, hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

}  // extern "C"
