// vct_api_emission.hip -- the C ABI of emissive materials (include/vct.h "emissive materials"): the material table with
// its emission pool, and the pixel-emission planes of a frame slot.
#include "vct_ctx.h"
#include "vct_emission_check.h"

// No material emission from here on: the table, the pool and every slot's planes that the table (not the caller) attached.
// The caller has made sure nothing in flight reads them (vct_pipeline_drain + the selected stream, or a hipFree's own wait).
void vct_emission_detach(vct_ctx* c) {
    c->mesh.mat_emission.reset();
    c->vox.emis_pool.reset();
    c->vox.emis_dirty = true;
    c->vox.pass_emis = false;
    vct_emission_planes_release(c);
}

void vct_emission_planes_release(vct_ctx* c) {
    if (vct_emission_table_attached(c)) return;      // the other table still writes them
    for (VctFrameSlot& sl : c->slots)
        if (!sl.emis_user) sl.emis.reset();
}

hipError_t vct_emission_planes(const vct_ctx* c, VctFrameSlot& s, bool* fresh) {
    return vct_planes_ensure(s.emis, vct_emis_tiled_floats(c), s.stream.get(), fresh);
}
void vct_emission_planes_drop(VctFrameSlot& s) { s.emis.reset(); }

extern "C" {

int vct_upload_emission(vct_ctx* c, const float* emission) {
    if (!c) return VCT_ERR_INVALID;
    if (!c->mesh.tri_pos) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_emission: call vct_upload_triangles first");
    const int32_t nmat = c->mesh.nmat;
    size_t bad = 0;
    const int verdict = emission ? vct_emission_check(emission, nmat, &bad) : VCT_EMISSION_ZERO;
    if (verdict == VCT_EMISSION_BAD) {
        char msg[160];
        snprintf(msg, sizeof msg, "vct_upload_emission: channel %zu of material %zu (%g) is not finite or below 0",
                 bad % 3, bad / 3, (double)emission[bad]);
        return vct_fail(c, VCT_ERR_INVALID, msg);
    }
    if (verdict == VCT_EMISSION_OK) PIPE_TRY(vct_refuse_conflict(c, "vct_upload_emission", VCT_FEAT_EMISSION, vct_rules_in_force(c).modes));
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_drain(c));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    if (verdict == VCT_EMISSION_ZERO) {       // NULL or all zero: detached -- no pool, no planes, no cost
        vct_emission_detach(c);
        return VCT_OK;
    }
    // all or nothing: the table and the pool in locals, planes only for slots that have none
    std::vector<float> padded((size_t)nmat * 4);
    vct_emission_pad(emission, nmat, padded.data());
    VctBuf<float> table;
    VctBuf<uint32_t> pool;
    hipError_t e = table.alloc(padded.size());
    if (e == hipSuccess) e = hipMemcpy(table.get(), padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && !c->vox.emis_pool) e = pool.alloc((size_t)(c->vox.nslots ? c->vox.nslots : 1u) * 512);
    PIPE_TRY(vct_planes_attach(c, "vct_upload_emission", vct_emission_planes, vct_emission_planes_drop, e));
    c->mesh.mat_emission = std::move(table);
    if (pool) c->vox.emis_pool = std::move(pool);
    c->vox.emis_dirty = true;       // the next north-star pass rebuilds the pool from this table
    return VCT_OK;
}

int vct_set_pixel_emission(vct_ctx* c, const float* planes, int32_t layout, int32_t location) {
    if (!c) return VCT_ERR_INVALID;
    VctFrameSlot& s = cur(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!planes) {       // detach the caller's planes; with material emission the slot keeps planes, zeroed until the next G-buffer pass
        s.emis_user = false;
        if (!s.emis) return VCT_OK;
        if (vct_emission_table_attached(c)) {
            HIP_TRY(c, hipMemsetAsync(s.emis.get(), 0, vct_emis_tiled_floats(c) * sizeof(float), s.stream.get()));
        } else {
            HIP_TRY(c, hipStreamSynchronize(s.stream.get()));      // a trace in flight may still read them
            s.emis.reset();
        }
        return VCT_OK;
    }
    if (layout != VCT_GB_LINEAR && layout != VCT_GB_TILED) return vct_fail(c, VCT_ERR_INVALID, "vct_set_pixel_emission: unknown layout");
    if (location != VCT_MEM_HOST && location != VCT_MEM_DEVICE) return vct_fail(c, VCT_ERR_INVALID, "vct_set_pixel_emission: unknown location");
    PIPE_TRY(vct_refuse_conflict(c, "vct_set_pixel_emission", VCT_FEAT_EMISSION, vct_rules_in_force(c).modes));
    HIP_TRY(c, vct_emission_planes(c, s));
    PIPE_TRY(vct_planes_set(c, s.emis.get(), planes, layout, location, VCT_EMIS_NPLANES, sizeof(float)));
    s.emis_user = true;
    return VCT_OK;
}

int vct_download_pixel_emission(vct_ctx* c, float* planes) {
    if (!c || !planes) return VCT_ERR_INVALID;
    if (!cur(c).emis) return vct_fail(c, VCT_ERR_INVALID, "vct_download_pixel_emission: no pixel-emission planes (vct_upload_emission, vct_set_pixel_emission)");
    HIP_TRY(c, hipSetDevice(c->device));
    return vct_planes_download(c, cur(c).emis.get(), planes, VCT_EMIS_NPLANES, sizeof(float));
}

}  // extern "C"
