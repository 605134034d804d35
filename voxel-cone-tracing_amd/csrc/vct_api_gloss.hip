// vct_api_gloss.hip -- the C ABI of per-material gloss (include/vct.h "per-material gloss"): the class table with its step
// tables, the material map of the mesh, and the pixel-gloss plane of a frame slot.
#include "vct_ctx.h"
#include "vct_gloss_check.h"

hipError_t vct_gloss_plane(const vct_ctx* c, VctFrameSlot& s, bool* fresh) {
    return vct_planes_ensure(s.gloss, vct_gloss_tiled_bytes(c), s.stream.get(), fresh);
}
static void gloss_plane_drop(VctFrameSlot& s) { s.gloss.reset(); }

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
        for (VctFrameSlot& sl : c->slots) gloss_plane_drop(sl);
        return VCT_OK;
    }
    PIPE_TRY(vct_refuse_conflict(c, "vct_set_gloss_classes", VCT_FEAT_GLOSS, vct_rules_in_force(c).modes));
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
    // all or nothing: the device table in a local, planes only for slots that have none
    VctBuf<VctGlossTable> table;
    PIPE_TRY(vct_planes_attach(c, "vct_set_gloss_classes", vct_gloss_plane, gloss_plane_drop, c->gloss.table ? hipSuccess : table.alloc(1)));
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
    return vct_planes_set(c, s.gloss.get(), classes, layout, location, 1, sizeof(uint8_t));
}

int vct_download_pixel_gloss(vct_ctx* c, uint8_t* out) {
    if (!c || !out) return VCT_ERR_INVALID;
    if (!cur(c).gloss) return vct_fail(c, VCT_ERR_INVALID, "vct_download_pixel_gloss: no pixel-gloss plane (vct_set_gloss_classes)");
    HIP_TRY(c, hipSetDevice(c->device));
    return vct_planes_download(c, cur(c).gloss.get(), out, 1, sizeof(uint8_t));
}

}  // extern "C"
