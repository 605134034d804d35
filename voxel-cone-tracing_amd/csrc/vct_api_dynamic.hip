// vct_api_dynamic.hip -- the C ABI of the dynamic mesh (include/vct.h "dynamic mesh"): a second, small mesh whose
// positions change every frame, voxelized by itself in every pass and merged into level 0 behind the static resolve.
// Everything the per-pass path needs is allocated by vct_set_dynamic_mesh (the emission table and its sums by
// vct_set_dynamic_emission); a pass with the mesh attached issues a memset of four words and kernels on the selected
// slot's stream, nothing else.
#include "vct_ctx.h"
#include "vct_dynamic_check.h"

namespace {

// the voxelizer's parameters for the dynamic mesh: its own triangles and table, the context's grid and shadow map, no
// plan and no textures
VctVoxParams dyn_vox_params(const vct_ctx* c, const VctDynamic& d) {
    VctVoxParams p;
    memset(&p, 0, sizeof(p));
    p.V = c->cfg.voxel_dim;
    p.G = c->cfg.grid_world_size;
    p.model_scale = c->cfg.model_scale;
    p.pos = d.pos.get();
    p.material = d.mat.get();
    p.albedo = d.albedo.get();
    p.ntri = d.ntri;
    p.shadow = c->shadow.words.get();
    p.shadow_tiles = c->shadow.words ? c->shadow.tiles.get() : nullptr;
    p.shadow_ebase = c->shadow.ebase;
    p.shadow_size = c->shadow.size;
    memcpy(p.light_vp, c->shadow.light_vp, 64);
    return p;
}

VctDynArgs dyn_args(const vct_ctx* c, const VctDynamic& d) {
    VctDynArgs a;
    memset(&a, 0, sizeof(a));
    a.words = d.words.get();
    a.brick_slot = d.brick_slot.get();
    a.slot_brick = d.slot_brick.get();
    a.big_list = d.big_list.get();
    a.max_bricks = d.max_bricks;
    a.vertex_limit = VCT_VERTEX_LIMIT_GRIDS * c->cfg.grid_world_size;
    a.acc = d.acc.get();
    a.acc_attr = d.acc_attr.get();
    return a;
}

int launch_merge(vct_ctx* c, bool discard) {
    VctDynamic& d = c->dyn;
    VctDynMergeArgs a;
    memset(&a, 0, sizeof(a));
    a.d = dyn_args(c, d);
    a.nbricks = (uint32_t)c->vol.nbricks();
    a.set = 1 - d.set;
    a.discard = discard ? 1 : 0;
    a.res_brick = d.res_brick.get();
    a.pool_rad = d.pool_rad.get(); a.pool_alb = d.pool_alb.get(); a.pool_nrm = d.pool_nrm.get();
    a.level0 = c->vol.chain.get();
    a.brick_prev = c->vol.brick_prev.get();
    // a pass voxelized with the emission table: the EMIS form resolves (or, discarding, only re-zeroes) the sums as well
    HIP_TRY(c, vct_launch_dynamic_merge(a, cur(c).stream.get(), d.pass_emis ? d.acc_emis.get() : nullptr));
    return VCT_OK;
}

// The draw copy and the face frames of layer `d` (vct_ctx.h VctDynamic): allocated if the layer has none, rebuilt from its
// positions on stream s.  Called where the positions change or a draw flag goes on, never from a raster stage.
int draw_prepare(vct_ctx* c, VctDynamic& d, hipStream_t s) {
    const size_t n = vct_dynamic_draw_floats(d.ntri);
    if (!d.draw_pos) {
        HIP_TRY(c, d.draw_pos.alloc(n));
        HIP_TRY(c, d.draw_nrm.alloc(n));
        HIP_TRY(c, d.draw_tan.alloc(n));
        HIP_TRY(c, d.draw_bit.alloc(n));
    }
    HIP_TRY(c, vct_launch_dynamic_draw_prepare(d.pos.get(), d.ntri, c->cfg.model_scale, VCT_VERTEX_LIMIT_GRIDS * c->cfg.grid_world_size,
                                               d.draw_pos.get(), d.draw_nrm.get(), d.draw_tan.get(), d.draw_bit.get(), s));
    return VCT_OK;
}

// The layer's positions from its rest positions and the matrix table on stream s: k_dyn_transform, or -- drawn -- the PARTS
// form of the prepare kernel, which goes on to the draw copy and the frames.  The draw arrays exist whenever a flag is on
// and a mesh is attached (vct_set_dynamic_mesh, vct_set_dynamic_draw), so nothing is allocated here.
int transform(vct_ctx* c, VctDynamic& d, hipStream_t s) {
    const VctDynPartsArgs a = {d.rest.get(), d.part.get(), d.part_m.get(), d.pos.get()};
    if (d.draw_flags && d.draw_pos)
        HIP_TRY(c, vct_launch_dynamic_transform_prepare(a, d.ntri, c->cfg.model_scale, VCT_VERTEX_LIMIT_GRIDS * c->cfg.grid_world_size,
                                                        d.draw_pos.get(), d.draw_nrm.get(), d.draw_tan.get(), d.draw_bit.get(), s));
    else
        HIP_TRY(c, vct_launch_dynamic_transform(a, d.ntri, s));
    return VCT_OK;
}

// one pooled volume of the last resolved pass -> dense Morton -> linear staging -> host, synchronised
int download_pool(vct_ctx* c, const uint32_t* pool, uint32_t* dense, uint8_t* dst) {
    const VctDynamic& d = c->dyn;
    hipStream_t s = cur(c).stream.get();
    HIP_TRY(c, vct_launch_dynamic_unpool(pool, d.res_brick.get(), d.words.get(), d.set, d.max_bricks, (uint32_t)c->vol.nbricks(), dense, s));
    PIPE_TRY(vct_staging_free(c));
    HIP_TRY(c, c->vol.staging.reserve(c->vol.nvox()));
    HIP_TRY(c, vct_launch_morton_to_linear(dense, c->vol.staging.get(), c->vol.V, s));
    HIP_TRY(c, hipMemcpyAsync(dst, c->vol.staging.get(), c->vol.nvox() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return VCT_OK;
}

}  // namespace

int vct_dynamic_draw_prepare(vct_ctx* c) {
    VctDynamic& d = c->dyn;
    if (!d.attached() || !d.draw_flags) return VCT_OK;
    return draw_prepare(c, d, cur(c).stream.get());
}

int vct_dynamic_voxelize(vct_ctx* c) {
    VctDynamic& d = c->dyn;
    if (!d.attached()) return VCT_OK;
    hipStream_t s = cur(c).stream.get();
    if (d.pending) PIPE_TRY(launch_merge(c, true));      // a pass that was never resolved: accumulators and table back to empty
    HIP_TRY(c, d.vox_timer.begin(s, c->time_traces));
    HIP_TRY(c, hipMemsetAsync(d.words.get(), 0, 4 * sizeof(uint32_t), s));      // need, fragments, skipped, big triangles
    const VctDynEmisArgs ea = {d.emission.get(), d.acc_emis.get()};
    HIP_TRY(c, vct_launch_dynamic_voxelize(dyn_vox_params(c, d), dyn_args(c, d), false, s, d.emission ? &ea : nullptr));
    HIP_TRY(c, d.vox_timer.end(s));
    d.pass_emis = (bool)d.emission;       // the pass carries the table it was voxelized under
    d.pending = true;
    return VCT_OK;
}

int vct_dynamic_merge(vct_ctx* c) {
    VctDynamic& d = c->dyn;
    if (!d.attached() || !d.pending) return VCT_OK;
    hipStream_t s = cur(c).stream.get();
    HIP_TRY(c, d.merge_timer.begin(s, c->time_traces));
    PIPE_TRY(launch_merge(c, false));
    HIP_TRY(c, d.merge_timer.end(s));
    d.set = 1 - d.set;
    d.pending = false;
    // local lights over the layer's own attribute pools: every slot is visited, a slot without a brick has empty pools
    if (c->lights.n && d.pool_alb) {
        VctLightVoxArgs la;
        memset(&la, 0, sizeof(la));
        la.lights = c->lights.table.get(); la.nlights = c->lights.n;
        la.V = c->cfg.voxel_dim; la.G = c->cfg.grid_world_size;
        la.level0 = c->vol.chain.get(); la.attr_albedo = d.pool_alb.get(); la.attr_normal = d.pool_nrm.get();
        la.slot_brick = d.res_brick.get(); la.brick_prev = c->vol.brick_prev.get(); la.nslots = d.max_bricks;
        HIP_TRY(c, vct_launch_light_voxels(la, s));
    }
    return VCT_OK;
}

extern "C" {

int vct_set_dynamic_mesh(vct_ctx* c, const float* pos, const int32_t* material, int32_t ntri, const float* albedo,
                         int32_t nmat, int32_t max_bricks) {
    if (!c) return VCT_ERR_INVALID;
    if (!pos || ntri == 0) {      // detach: the next static resolve clears what the object left (brick_prev is raised there)
        if (!c->dyn.attached()) return VCT_OK;
        HIP_TRY(c, hipSetDevice(c->device));
        PIPE_TRY(vct_synchronize(c));         // a kernel in flight may still read the layer
        VctDynamic none;
        none.keep_draw_state(c->dyn);         // vct_set_dynamic_draw is context state: it outlives the mesh
        none.keep_bounce_state(c->dyn);       // and so is vct_set_dynamic_bounce
        c->dyn = std::move(none);
        vct_emission_planes_release(c);       // the emission table went with the mesh
        return VCT_OK;
    }
    if (const char* why = vct_dynamic_check_args(pos, material, ntri, albedo, nmat, max_bricks))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_mesh: ") + why);
    const bool attr = c->cfg.voxel_attributes != 0;
    const uint32_t nbricks = vct_dynamic_grid_bricks(c->cfg.voxel_dim);
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));
    // all or nothing: a fresh layer in a local; the context keeps what it had until everything below has succeeded
    VctDynamic d;
    hipStream_t s = cur(c).stream.get();
    VctDynamicSizes z = vct_dynamic_sizes(ntri, nmat, 0u, c->cfg.voxel_dim, attr);
    if (!z.ok) return vct_fail(c, VCT_ERR_INVALID, "vct_set_dynamic_mesh: buffer sizes overflow");
    HIP_TRY(c, d.pos.alloc((size_t)ntri * 9));
    HIP_TRY(c, d.mat.alloc((size_t)ntri));
    HIP_TRY(c, d.albedo.alloc((size_t)nmat * 4));
    HIP_TRY(c, d.big_list.alloc((size_t)ntri));
    HIP_TRY(c, d.words.alloc(VCT_DYN_WORDS));
    HIP_TRY(c, d.brick_slot.alloc(nbricks));
    HIP_TRY(c, hipMemcpyAsync(d.pos.get(), pos, z.pos, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d.mat.get(), material, z.material, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d.albedo.get(), albedo, z.albedo, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(d.words.get(), 0, z.words, s));
    HIP_TRY(c, hipMemsetAsync(d.brick_slot.get(), 0xff, z.brick_slot, s));
    d.ntri = ntri; d.nmat = nmat;
    uint32_t touched = 0u;
    if (max_bricks == 0) {
        // the bricks these positions touch: the slots kernels with no slot to hand out, the counter read back
        HIP_TRY(c, vct_launch_dynamic_voxelize(dyn_vox_params(c, d), dyn_args(c, d), true, s));
        HIP_TRY(c, hipMemcpyAsync(&touched, d.words.get() + VCT_DYN_W_NEED, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, hipMemsetAsync(d.words.get(), 0, z.words, s));
        HIP_TRY(c, hipMemsetAsync(d.brick_slot.get(), 0xff, z.brick_slot, s));
    }
    d.max_bricks = vct_dynamic_capacity(max_bricks, touched, nbricks);
    z = vct_dynamic_sizes(ntri, nmat, d.max_bricks, c->cfg.voxel_dim, attr);
    if (!z.ok) return vct_fail(c, VCT_ERR_INVALID, "vct_set_dynamic_mesh: buffer sizes overflow");
    const size_t ns = d.max_bricks;
    HIP_TRY(c, d.slot_brick.alloc(ns));
    HIP_TRY(c, d.res_brick.alloc(ns));
    HIP_TRY(c, d.acc.alloc(ns * 1024));
    HIP_TRY(c, d.pool_rad.alloc(ns * 512));
    HIP_TRY(c, hipMemsetAsync(d.slot_brick.get(), 0, z.slot_list, s));
    HIP_TRY(c, hipMemsetAsync(d.res_brick.get(), 0, z.slot_list, s));
    HIP_TRY(c, hipMemsetAsync(d.acc.get(), 0, z.acc, s));
    HIP_TRY(c, hipMemsetAsync(d.pool_rad.get(), 0, z.pool, s));
    if (attr) {
        HIP_TRY(c, d.acc_attr.alloc(ns * 1536));
        HIP_TRY(c, d.pool_alb.alloc(ns * 512));
        HIP_TRY(c, d.pool_nrm.alloc(ns * 512));
        HIP_TRY(c, hipMemsetAsync(d.acc_attr.get(), 0, z.acc_attr, s));
        HIP_TRY(c, hipMemsetAsync(d.pool_alb.get(), 0, z.pool, s));
        HIP_TRY(c, hipMemsetAsync(d.pool_nrm.get(), 0, z.pool, s));
    }
    HIP_TRY(c, d.vox_timer.create());           // the events now, so that no pass allocates
    HIP_TRY(c, d.merge_timer.create());
    d.keep_draw_state(c->dyn);
    d.keep_bounce_state(c->dyn);
    if (d.draw_flags) PIPE_TRY(draw_prepare(c, d, s));      // drawn: the draw copy and the frames of these positions
    HIP_TRY(c, hipStreamSynchronize(s));        // the caller's arrays are free again
    c->dyn = std::move(d);
    vct_emission_planes_release(c);             // a replaced mesh's emission table went with it
    return VCT_OK;
}

int vct_update_dynamic_positions(vct_ctx* c, const float* pos, int32_t location) {
    if (!c) return VCT_ERR_INVALID;
    if (const char* why = vct_dynamic_check_update(c->dyn.attached(), pos, location))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_update_dynamic_positions: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_join(c));       // the buffer is shared: the other slot's pass may still read the previous positions
    HIP_TRY(c, hipMemcpyAsync(c->dyn.pos.get(), pos, (size_t)c->dyn.ntri * 9 * sizeof(float),
                              location == VCT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, cur(c).stream.get()));
    if (c->dyn.nparts)                    // parts attached: these positions are the new rest positions as well
        HIP_TRY(c, hipMemcpyAsync(c->dyn.rest.get(), c->dyn.pos.get(), (size_t)c->dyn.ntri * 9 * sizeof(float),
                                  hipMemcpyDeviceToDevice, cur(c).stream.get()));
    return vct_dynamic_draw_prepare(c);   // behind the copy, on its stream: ordered before every stage that draws the mesh
}

int vct_set_dynamic_parts(vct_ctx* c, const int32_t* part, int32_t nparts) {
    if (!c) return VCT_ERR_INVALID;
    VctDynamic& d = c->dyn;
    const bool detach = !part && nparts == 0;
    if (detach && !d.attached()) return vct_fail(c, VCT_ERR_INVALID, "vct_set_dynamic_parts: no dynamic mesh attached");
    if (!detach) {
        int32_t bad = -1;
        if (const char* why = vct_dynamic_check_parts(d.attached(), part, d.ntri, nparts, &bad)) {
            if (bad < 0) return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_parts: ") + why);
            char msg[160];
            snprintf(msg, sizeof msg, "vct_set_dynamic_parts: part index %d of triangle %d is outside 0 .. %d", (int)part[bad],
                     (int)bad, (int)nparts - 1);
            return vct_fail(c, VCT_ERR_INVALID, msg);
        }
    }
    if (detach && !d.nparts) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // a transform in flight reads all three buffers
    if (detach) {                         // the current positions stay as they are
        d.drop_parts();
        return VCT_OK;
    }
    // all or nothing: everything in locals; the context keeps what it had until the last call below has succeeded
    const VctDynamicPartsSizes z = vct_dynamic_parts_sizes(d.ntri, nparts);
    if (!z.ok) return vct_fail(c, VCT_ERR_INVALID, "vct_set_dynamic_parts: buffer sizes overflow");
    hipStream_t s = cur(c).stream.get();
    VctBuf<float> rest;
    VctBuf<int32_t> idx;
    VctBuf<float4> table;
    VctTimer timer;
    HIP_TRY(c, rest.alloc((size_t)d.ntri * 9));
    HIP_TRY(c, idx.alloc((size_t)d.ntri));
    HIP_TRY(c, table.alloc((size_t)nparts * 3));
    HIP_TRY(c, timer.create());           // the events now, so that no update allocates
    // the rest positions: what the last vct_set_dynamic_mesh or vct_update_dynamic_positions -- or transform -- put there
    HIP_TRY(c, hipMemcpyAsync(rest.get(), d.pos.get(), z.rest, hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(idx.get(), part, z.part, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(table.get(), 0, z.table, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // the caller's array is free again
    d.rest = std::move(rest);
    d.part = std::move(idx);
    d.part_m = std::move(table);
    d.xform_timer = std::move(timer);
    d.nparts = nparts;
    return VCT_OK;
}

int vct_get_dynamic_parts(vct_ctx* c, int32_t* nparts, int32_t* part) {
    if (!c || !nparts) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    *nparts = d.nparts;
    if (!d.nparts || !part) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(part, d.part.get(), (size_t)d.ntri * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VCT_OK;
}

int vct_update_dynamic_transforms(vct_ctx* c, const float* m, int32_t location) {
    if (!c) return VCT_ERR_INVALID;
    VctDynamic& d = c->dyn;
    if (const char* why = vct_dynamic_check_transforms(d.attached(), d.nparts, m, location))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_update_dynamic_transforms: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_join(c));       // positions and table are shared: the other slot's pass may still read the positions
    hipStream_t s = cur(c).stream.get();
    HIP_TRY(c, hipMemcpyAsync(d.part_m.get(), m, (size_t)d.nparts * 12 * sizeof(float),
                              location == VCT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    HIP_TRY(c, d.xform_timer.begin(s, c->time_traces));
    PIPE_TRY(transform(c, d, s));
    HIP_TRY(c, d.xform_timer.end(s));
    return VCT_OK;
}

int vct_download_dynamic_positions(vct_ctx* c, float* pos) {
    if (!c) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    if (!d.attached()) return vct_fail(c, VCT_ERR_INVALID, "vct_download_dynamic_positions: no dynamic mesh attached");
    if (!pos) return vct_fail(c, VCT_ERR_INVALID, "vct_download_dynamic_positions: null positions");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // the last update may have been issued on the other frame slot's stream
    HIP_TRY(c, hipMemcpy(pos, d.pos.get(), (size_t)d.ntri * 9 * sizeof(float), hipMemcpyDeviceToHost));
    return VCT_OK;
}

int vct_last_dynamic_transform_ms(vct_ctx* c, float* ms) {
    if (!c || !ms) return VCT_ERR_INVALID;
    const char* never = "vct_last_dynamic_transform_ms: needs parts attached and a vct_update_dynamic_transforms since";
    const char* untimed = "vct_last_dynamic_transform_ms: the last transform was issued with timing off (vct_set_trace_timing)";
    if (!c->dyn.nparts || !c->dyn.xform_timer.have) return vct_fail(c, VCT_ERR_INVALID, never);
    return vct_timer_ms(c, c->dyn.xform_timer, ms, never, untimed);
}

int vct_set_dynamic_draw(vct_ctx* c, int32_t flags, const float specular[3]) {
    if (!c) return VCT_ERR_INVALID;
    if (const char* why = vct_dynamic_check_draw(flags, specular))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_draw: ") + why);
    VctDynamic& d = c->dyn;
    const bool goes_on = flags && !d.draw_flags;
    if (goes_on && d.attached()) {
        // the draw copy is shared by both slots like the positions: the other slot's pass may still read the previous one
        HIP_TRY(c, hipSetDevice(c->device));
        PIPE_TRY(vct_pipeline_join(c));
        PIPE_TRY(draw_prepare(c, d, cur(c).stream.get()));
    }
    d.draw_flags = flags;
    for (int k = 0; k < 3; ++k) d.draw_specular[k] = specular ? specular[k] : 0.0f;
    return VCT_OK;
}

int vct_get_dynamic_draw(vct_ctx* c, int32_t* flags, float specular[3]) {
    if (!c || !flags || !specular) return VCT_ERR_INVALID;
    *flags = c->dyn.draw_flags;
    for (int k = 0; k < 3; ++k) specular[k] = c->dyn.draw_specular[k];
    return VCT_OK;
}

int vct_set_dynamic_bounce(vct_ctx* c, int32_t on) {
    if (!c) return VCT_ERR_INVALID;
    if (const char* why = vct_dynamic_check_bounce(on))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_bounce: ") + why);
    c->dyn.bounce_on = on;      // read by the next vct_bounce; nothing in flight depends on it
    return VCT_OK;
}

int vct_get_dynamic_bounce(vct_ctx* c, int32_t* on) {
    if (!c || !on) return VCT_ERR_INVALID;
    *on = c->dyn.bounce_on;
    return VCT_OK;
}

int vct_set_dynamic_emission(vct_ctx* c, const float* emission) {
    if (!c) return VCT_ERR_INVALID;
    VctDynamic& d = c->dyn;
    size_t bad = 0;
    const char* why = nullptr;
    const int verdict = vct_dynamic_check_emission(d.attached(), emission, d.nmat, &bad, &why);
    if (verdict == VCT_EMISSION_BAD) {
        if (bad == (size_t)-1) return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_emission: ") + why);
        char msg[160];
        snprintf(msg, sizeof msg, "vct_set_dynamic_emission: channel %zu of material %zu (%g) is not finite or below 0",
                 bad % 3, bad / 3, (double)emission[bad]);
        return vct_fail(c, VCT_ERR_INVALID, msg);
    }
    if (verdict == VCT_EMISSION_OK) PIPE_TRY(vct_refuse_conflict(c, "vct_set_dynamic_emission", VCT_FEAT_EMISSION, vct_rules_in_force(c).modes));
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // a pass in flight may read the table and add to the sums
    if (verdict == VCT_EMISSION_ZERO) {   // NULL or all zero: detached -- a pending pass resolves without emission
        d.emission.reset();
        d.acc_emis.reset();
        d.pass_emis = false;
        vct_emission_planes_release(c);
        return VCT_OK;
    }
    // all or nothing: the table and (for a first table) the zeroed sums in locals, planes only for slots that have none.
    // A replaced table keeps the sums: a pending pass resolves with the table it was voxelized under.
    const VctDynamicEmissionSizes z = vct_dynamic_emission_sizes(d.nmat, d.max_bricks);
    if (!z.ok) return vct_fail(c, VCT_ERR_INVALID, "vct_set_dynamic_emission: buffer sizes overflow");
    std::vector<float> padded((size_t)d.nmat * 4);
    vct_emission_pad(emission, d.nmat, padded.data());
    VctBuf<float> table;
    VctBuf<unsigned long long> sums;
    hipError_t e = table.alloc(padded.size());
    if (e == hipSuccess) e = hipMemcpy(table.get(), padded.data(), z.table, hipMemcpyHostToDevice);
    if (e == hipSuccess && !d.acc_emis) {
        e = sums.alloc((size_t)d.max_bricks * 1024);
        if (e == hipSuccess) e = hipMemsetAsync(sums.get(), 0, z.sums, cur(c).stream.get());      // (vct_planes_attach waits for the stream)
    }
    PIPE_TRY(vct_planes_attach(c, "vct_set_dynamic_emission", vct_emission_planes, vct_emission_planes_drop, e));
    if (!d.acc_emis) { d.acc_emis = std::move(sums); d.pass_emis = false; }      // attached behind a vct_voxelize: that pass has none
    d.emission = std::move(table);
    return VCT_OK;
}

int vct_get_dynamic_emission(vct_ctx* c, float* emission, int32_t* nmat) {
    if (!c || !nmat) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    *nmat = d.emission ? d.nmat : 0;
    if (!d.emission || !emission) return VCT_OK;
    std::vector<float> padded((size_t)d.nmat * 4);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(padded.data(), d.emission.get(), padded.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int32_t m = 0; m < d.nmat; ++m)
        for (int k = 0; k < 3; ++k) emission[(size_t)m * 3 + k] = padded[(size_t)m * 4 + k];
    return VCT_OK;
}

int vct_get_dynamic(vct_ctx* c, int32_t out[8]) {
    if (!c || !out) return VCT_ERR_INVALID;
    memset(out, 0, 8 * sizeof(int32_t));
    const VctDynamic& d = c->dyn;
    if (!d.attached()) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // the last merge may have been issued on the other frame slot's stream
    uint32_t st[8] = {};
    HIP_TRY(c, hipMemcpyAsync(st, d.words.get() + VCT_DYN_W_STATS + 8 * d.set, sizeof st, hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    out[0] = d.ntri; out[1] = d.nmat; out[2] = (int32_t)d.max_bricks;
    for (int k = 0; k < 5; ++k) out[3 + k] = (int32_t)st[k];
    return VCT_OK;
}

int vct_download_dynamic_voxels(vct_ctx* c, uint8_t* radiance, uint8_t* albedo, uint8_t* normal) {
    if (!c) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    if (!d.attached()) return vct_fail(c, VCT_ERR_INVALID, "vct_download_dynamic_voxels: no dynamic mesh attached");
    if ((albedo || normal) && !d.pool_alb)
        return vct_fail(c, VCT_ERR_INVALID, "vct_download_dynamic_voxels: albedo and normal need config.voxel_attributes = 1");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // the pools may still be written on the other frame slot's stream
    VctBuf<uint32_t> dense;
    HIP_TRY(c, dense.alloc(c->vol.nvox()));
    const uint32_t* src[3] = {d.pool_rad.get(), d.pool_alb.get(), d.pool_nrm.get()};
    uint8_t* dst[3] = {radiance, albedo, normal};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) PIPE_TRY(download_pool(c, src[k], dense.get(), dst[k]));
    return VCT_OK;
}

int vct_last_dynamic_ms(vct_ctx* c, float ms[2]) {
    if (!c || !ms) return VCT_ERR_INVALID;
    const char* never = "vct_last_dynamic_ms: needs a dynamic mesh attached and a vct_voxelize + vct_inject_light since";
    const char* untimed = "vct_last_dynamic_ms: the last kernels were issued with timing off (vct_set_trace_timing)";
    if (!c->dyn.attached() || !c->dyn.vox_timer.have || !c->dyn.merge_timer.have) return vct_fail(c, VCT_ERR_INVALID, never);
    PIPE_TRY(vct_timer_ms(c, c->dyn.vox_timer, &ms[0], never, untimed));
    return vct_timer_ms(c, c->dyn.merge_timer, &ms[1], never, untimed);
}

}  // extern "C"
