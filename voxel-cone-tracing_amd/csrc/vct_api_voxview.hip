// vct_api_voxview.hip -- the C ABI's voxel view: vct_render_voxels, vct_last_voxel_view_ms.
#include "vct_ctx.h"

extern "C" {

int vct_render_voxels(vct_ctx* c, const float inv_view_proj[16], int32_t source, int32_t level) {
    if (!c) return VCT_ERR_INVALID;
    if (!inv_view_proj) return vct_fail(c, VCT_ERR_INVALID, "vct_render_voxels: null matrix");
    for (int i = 0; i < 16; ++i)
        if (!isfinite(inv_view_proj[i])) return vct_fail(c, VCT_ERR_INVALID, "vct_render_voxels: the matrix has a non-finite element");
    if (source < VCT_VOXVIEW_CURRENT || source > VCT_VOXVIEW_NORMAL) return vct_fail(c, VCT_ERR_INVALID, "vct_render_voxels: unknown source");
    if (level < 0 || level >= c->vol.nlev) return vct_fail(c, VCT_ERR_INVALID, "vct_render_voxels: level outside [0, levels of the chain)");
    if (c->comm) return vct_fail(c, VCT_ERR_INVALID, "vct_render_voxels: a rank of a multi-GPU frame (views are not gathered)");
    const bool attribute = source == VCT_VOXVIEW_ALBEDO || source == VCT_VOXVIEW_NORMAL;
    VctVoxViewParams p;
    memset(&p, 0, sizeof(p));
    if (attribute) {
        if (!c->cfg.voxel_attributes) return vct_fail(c, VCT_ERR_INVALID, "vct_render_voxels: ALBEDO / NORMAL need config.voxel_attributes = 1");
        if (level != 0) return vct_fail(c, VCT_ERR_INVALID, "vct_render_voxels: the voxel attributes exist at level 0 only");
        if (!c->vox.attr_albedo || !c->vox.brick_slot)
            return vct_fail(c, VCT_ERR_INVALID, "vct_render_voxels: no voxel attributes yet (vct_upload_triangles, vct_voxelize + vct_inject_light)");
        p.texels = source == VCT_VOXVIEW_ALBEDO ? c->vox.attr_albedo.get() : c->vox.attr_normal.get();
        p.brick_slot = c->vox.brick_slot.get();
    } else {
        // like a trace: coarse levels that describe an older level 0 would be shown without any sign of it
        if (level > 0 && !c->vol.mips_valid)
            return vct_fail(c, VCT_ERR_INVALID, "vct_render_voxels: level 0 changed since the last vct_build_mips (call it first, or view level 0)");
        const uint32_t* chain = source == VCT_VOXVIEW_RADIANCE ? c->vol.chain.get() : c->vol.active();
        p.texels = chain + vct_level_offset(c->cfg.voxel_dim, level);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    VctFrameSlot& s = cur(c);
    p.N = c->cfg.voxel_dim >> level;
    p.occ_dim = p.N >= 32 ? p.N >> 5 : 1;
    p.G = c->cfg.grid_world_size;
    p.max_alpha = c->cfg.max_alpha;
    memcpy(p.m, inv_view_proj, sizeof(p.m));
    p.width = c->cfg.width;
    p.height = c->cfg.height;
    p.tiles_x = vct_tiles_x(c);
    p.tiles_y = vct_tiles_y(c);
    p.out = s.frame_out();
    // VCT_VOXVIEW_SKIP=0 (A/B): the walk's instantiation without the occupancy look-ups -- same frame, every cell fetched.
    // Read per call, so that one process can alternate the two on one context (tools/voxel_view_probe.py).
    const char* skip_env = getenv("VCT_VOXVIEW_SKIP");
    const bool skip = !(skip_env && skip_env[0] == '0');
    if (skip) {
        // one word per 32^3 texels of level 0 holds any level; rebuilt on this slot's stream when what it describes changed
        if (!s.vv_occ) {
            const size_t d0 = c->cfg.voxel_dim >= 32 ? (size_t)c->cfg.voxel_dim >> 5 : 1;
            HIP_TRY(c, s.vv_occ.alloc(d0 * d0 * d0));
            s.vv_texels = nullptr;
        }
        p.occ = s.vv_occ.get();
        if (s.vv_texels != p.texels || s.vv_gen != c->vol.gen) {
            s.vv_texels = nullptr;
            HIP_TRY(c, vct_launch_voxview_occupancy(p, s.stream.get()));
            s.vv_texels = p.texels;
            s.vv_gen = c->vol.gen;
        }
    }
    HIP_TRY(c, s.vv_timer.begin(s.stream.get(), c->time_traces));
    HIP_TRY(c, vct_launch_voxview(p, skip, s.stream.get()));
    HIP_TRY(c, s.vv_timer.end(s.stream.get()));
    return VCT_OK;
}

int vct_last_voxel_view_ms(vct_ctx* c, float* ms) {
    if (!c || !ms) return VCT_ERR_INVALID;
    return vct_timer_ms(c, cur(c).vv_timer, ms, "vct_last_voxel_view_ms: no voxel view has run on this frame slot",
                        "vct_last_voxel_view_ms: the last view was issued with timing off (vct_set_trace_timing)");
}

}  // extern "C"
