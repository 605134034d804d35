// vct_api_dynamic.hip -- the C ABI of the dynamic mesh (include/vct.h "dynamic mesh"): a second, small mesh whose
// positions change every frame, voxelized by itself in every pass and merged into level 0 behind the static resolve.
// Everything the per-pass path needs is allocated by vct_set_dynamic_mesh (the emission table and its sums by
// vct_set_dynamic_emission); a pass with the mesh attached issues a memset of four words and kernels on the selected
// slot's stream, nothing else.
#include "vct_ctx.h"
#include "vct_dynamic_check.h"

namespace {

// Device memory of `bytes` bytes for `b` -- a byte count of vct_dynamic_check.h, the one statement of a buffer's size --
// and the same with every byte set to `fill` on stream s.
template <class T>
hipError_t alloc_bytes(VctBuf<T>& b, size_t bytes) { return b.alloc(bytes / sizeof(T)); }
template <class T>
hipError_t alloc_filled(VctBuf<T>& b, size_t bytes, int fill, hipStream_t s) {
    const hipError_t e = alloc_bytes(b, bytes);
    return e == hipSuccess ? hipMemsetAsync(b.get(), fill, bytes, s) : e;
}

// the statistics set of the last resolved pass (vct_internal.h VCT_DYN_W_STATS): need, used, fragments, skipped, left out
const uint32_t* resolved_stats(const VctDynamic& d) { return d.words.get() + VCT_DYN_W_STATS + 8 * d.pass.set; }

// the voxelizer's parameters for the dynamic mesh: its own triangles and table, the context's grid and shadow map, no
// plan and no textures
VctVoxParams dyn_vox_params(const vct_ctx* c, const VctDynamic& d) {
    VctVoxParams p = vct_vox_params_scene(c);
    p.pos = d.pos.get();
    p.material = d.mat.get();
    p.albedo = d.albedo.get();
    p.ntri = d.ntri;
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
    a.vertex_limit = vct_vertex_limit(c);
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
    a.set = 1 - d.pass.set;
    a.discard = discard ? 1 : 0;
    a.res_brick = d.res_brick.get();
    a.pool_rad = d.pool_rad.get(); a.pool_alb = d.pool_alb.get(); a.pool_nrm = d.pool_nrm.get();
    a.level0 = c->vol.chain.get();
    a.brick_prev = c->vol.brick_prev.get();
    // a pass voxelized with the emission table: the EMIS form resolves (or, discarding, only re-zeroes) the sums as well
    HIP_TRY(c, vct_launch_dynamic_merge(a, cur(c).stream.get(), d.pass.emis ? d.emis.acc.get() : nullptr));
    return VCT_OK;
}

// what the prepare kernels take beside the positions: the vertex contract and the draw arrays of layer `d`
VctDynPrepare prepare_args(const vct_ctx* c, const VctDynamic& d) {
    return {c->cfg.model_scale, vct_vertex_limit(c), d.draw.pos.get(), d.draw.nrm.get(), d.draw.tan.get(), d.draw.bit.get(),
            d.corner_nrm.get()};
}

// The layer's positions from the mover's rest positions and matrix table on stream s: the plain kernel, or -- drawn -- the
// mover's form of the prepare kernel, which goes on to the draw copy and the frames.  The draw arrays exist whenever a
// flag is on and a mesh is attached (vct_set_dynamic_mesh, vct_set_dynamic_draw), so nothing is allocated here.
int transform(vct_ctx* c, VctDynamic& d, hipStream_t s, bool drawn) {
    const VctDynamic::Mover& v = d.mover;
    VctDynMoverArgs a = {};
    a.is_skin = v.kind == VCT_MOVER_SKIN;
    if (a.is_skin) a.skin = {v.rest.get(), v.bone.get(), v.weight.get(), v.m.get(), d.pos.get()};
    else a.parts = {v.rest.get(), v.part.get(), v.m.get(), d.pos.get()};
    const VctDynPrepare p = prepare_args(c, d);
    HIP_TRY(c, vct_launch_dynamic_move(a, d.ntri, drawn ? &p : nullptr, s));
    return VCT_OK;
}

// The draw copy and the frames of layer `d` (vct_ctx.h VctDynamic): allocated if the layer has none, rebuilt from its
// positions on stream s.  Called where the positions change or a draw flag goes on, never from a raster stage.  With
// corner normals AND a mover attached the frames need the mover's matrices (the normals are in rest space), so the
// mover's own kernel runs again over the rest positions and the table: it rewrites the same positions on the way.
int draw_prepare(vct_ctx* c, VctDynamic& d, hipStream_t s) {
    const size_t n = vct_dynamic_draw_floats(d.ntri);
    if (!d.draw.pos)
        for (VctBuf<float>* b : {&d.draw.nrm, &d.draw.tan, &d.draw.bit, &d.draw.pos}) HIP_TRY(c, b->alloc(n));      // (pos last: it says "all four")
    if (d.corner_nrm && d.matrices() && d.mover.moved) return transform(c, d, s, true);
    HIP_TRY(c, vct_launch_dynamic_draw_prepare(d.pos.get(), d.ntri, prepare_args(c, d), s));
    return VCT_OK;
}

// What an attach needs beside the kind's own arrays: byte counts of vct_dynamic_parts_sizes / vct_dynamic_skin_sizes.
struct MoverSizes {
    bool ok;
    size_t rest, table;
};

// Attaches a mover of `kind` with n matrices to the attached mesh, in place of one of the same kind; the other kind attached
// is refused (vct_feature_rules.h).  fill(mover, stream) allocates and copies the kind's own arrays.  All or nothing:
// everything in a local; the context keeps what it had until the last call below has succeeded.
template <class Fill>
int attach_mover(vct_ctx* c, const char* who, VctMover kind, int32_t n, const MoverSizes& z, Fill fill) {
    VctDynamic& d = c->dyn;
    const VctMover hit = vct_mover_conflict(d.mover.kind, kind);
    if (hit != VCT_MOVER_NONE)
        return vct_fail(c, VCT_ERR_INVALID, std::string(who) + ": " + kVctMoverText[kind].name + " and " + kVctMoverText[hit].name +
                                                " do not go together on one mesh (" + kVctMoverText[hit].lift + " lifts it)");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // an update in flight reads all of the previous mover's buffers
    if (!z.ok) return vct_fail(c, VCT_ERR_INVALID, std::string(who) + ": buffer sizes overflow");
    hipStream_t s = cur(c).stream.get();
    VctDynamic::Mover v;
    HIP_TRY(c, alloc_bytes(v.rest, z.rest));
    HIP_TRY(c, v.timer.create());         // the events now, so that no update allocates
    // the rest positions: what the last vct_set_dynamic_mesh or vct_update_dynamic_positions -- or transform -- put there
    HIP_TRY(c, hipMemcpyAsync(v.rest.get(), d.pos.get(), z.rest, hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, fill(v, s));
    HIP_TRY(c, alloc_filled(v.m, z.table, 0, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // the caller's arrays are free again
    v.kind = kind;
    v.n = n;
    std::swap(d.mover, v);
    if (!d.corner_nrm) return VCT_OK;
    // corner normals are read in the space of the new rest positions from here on: the frames of a replaced mover's pose
    // go.  Still all or nothing: a launch that fails puts the previous mover back.
    const int rc = vct_dynamic_draw_prepare(c);
    if (rc != VCT_OK) std::swap(d.mover, v);
    return rc;
}

// Detaches the mover if it is of `kind` -- the other kind, or none, attached: nothing to do.  The current positions stay.
int detach_mover(vct_ctx* c, const char* who, VctMover kind) {
    VctDynamic& d = c->dyn;
    if (!d.attached()) return vct_fail(c, VCT_ERR_INVALID, std::string(who) + ": no dynamic mesh attached");
    if (d.mover.kind != kind) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // an update in flight reads all of its buffers
    VctDynamic::Mover none;
    std::swap(d.mover, none);
    if (!d.corner_nrm) return VCT_OK;
    const int rc = vct_dynamic_draw_prepare(c);      // corner normals are used as given from here on
    if (rc != VCT_OK) std::swap(d.mover, none);      // (a launch that fails leaves the mover attached)
    return rc;
}

// `bytes` bytes of a caller's array into a fresh allocation of `b` on stream s
template <class T>
hipError_t alloc_copied(VctBuf<T>& b, const void* src, size_t bytes, hipStream_t s) {
    const hipError_t e = alloc_bytes(b, bytes);
    return e == hipSuccess ? hipMemcpyAsync(b.get(), src, bytes, hipMemcpyHostToDevice, s) : e;
}

}  // namespace

int vct_dynamic_draw_prepare(vct_ctx* c) {
    if (!c->dyn.attached() || !c->dyn_settings.draw_flags) return VCT_OK;
    return draw_prepare(c, c->dyn, cur(c).stream.get());
}

int vct_dynamic_voxelize(vct_ctx* c) {
    VctDynamic& d = c->dyn;
    if (!d.attached()) return VCT_OK;
    hipStream_t s = cur(c).stream.get();
    if (d.pass.pending) PIPE_TRY(launch_merge(c, true));      // a pass that was never resolved: accumulators and table back to empty
    HIP_TRY(c, d.vox_timer.begin(s, c->time_traces));
    HIP_TRY(c, hipMemsetAsync(d.words.get(), 0, 4 * sizeof(uint32_t), s));      // need, fragments, skipped, big triangles
    const VctDynEmisArgs ea = {d.emis.table.get(), d.emis.acc.get()};
    HIP_TRY(c, vct_launch_dynamic_voxelize(dyn_vox_params(c, d), dyn_args(c, d), false, s, d.emis.table ? &ea : nullptr));
    HIP_TRY(c, d.vox_timer.end(s));
    d.pass.emis = (bool)d.emis.table;     // the pass carries the table it was voxelized under
    d.pass.pending = true;
    return VCT_OK;
}

int vct_dynamic_merge(vct_ctx* c) {
    VctDynamic& d = c->dyn;
    // (vct_bounce: a pass with no layer to merge -- none pending, or the reference mode's -- bounces as the static chain)
    const bool merges = d.pass.pending && c->acc_mode == VCT_VOX_CONSERVATIVE_AVG;
    if (!merges) { d.pass.in_chain = false; return VCT_OK; }
    hipStream_t s = cur(c).stream.get();
    HIP_TRY(c, d.merge_timer.begin(s, c->time_traces));
    PIPE_TRY(launch_merge(c, false));
    HIP_TRY(c, d.merge_timer.end(s));
    d.pass.set = 1 - d.pass.set;
    d.pass.pending = false;
    // local lights over the layer's own attribute pools: every slot is visited, a slot without a brick has empty pools
    if (c->lights.n && d.pool_alb) PIPE_TRY(vct_light_voxels(c, d.pool_alb.get(), d.pool_nrm.get(), d.res_brick.get(), d.max_bricks));
    d.pass.in_chain = true;
    return VCT_OK;
}

void vct_dynamic_raster_mesh(const vct_ctx* c, VctRasterArgs& a) {
    const VctDynamic& d = c->dyn;
    a.pos = d.draw.pos.get();
    a.nrm = d.draw.nrm.get(); a.tan = d.draw.tan.get(); a.bit = d.draw.bit.get();
    a.material = d.mat.get();
    a.albedo = d.albedo.get();
    a.ntri = d.ntri;
}

void vct_dynamic_shade_args(const vct_ctx* c, const VctRasterArgs& da, VctDynShadeArgs& ds) {
    ds.vis = da.vis;
    ds.pos = da.pos; ds.nrm = da.nrm; ds.tan = da.tan; ds.bit = da.bit;
    ds.material = da.material; ds.albedo = da.albedo;
    for (int k = 0; k < 3; ++k) ds.specular[k] = c->dyn_settings.draw_specular[k];
    ds.emission = c->dyn.emis.table.get();
}

int vct_dynamic_bounce_args(vct_ctx* c, VctBounceDynArgs& da, bool* dyn) {
    const VctDynamic& d = c->dyn;
    *dyn = d.attached() && c->dyn_settings.bounce_on && d.pass.in_chain && d.pool_alb;
    if (!*dyn) return VCT_OK;
    const size_t map_bytes = vct_dynamic_bounce_map_bytes(c->cfg.voxel_dim);
    if (!c->bounce_dyn_map) HIP_TRY(c, alloc_bytes(c->bounce_dyn_map, map_bytes));
    memset(&da, 0, sizeof(da));
    da.res_brick = d.res_brick.get();
    da.used = resolved_stats(d) + 1;
    da.pool_rad = d.pool_rad.get(); da.pool_alb = d.pool_alb.get(); da.pool_nrm = d.pool_nrm.get();
    da.brick_res = c->bounce_dyn_map.get();
    da.max_bricks = d.max_bricks;
    da.list_slots = vct_dynamic_bounce_list_slots(c->vox.nslots, d.max_bricks);
    HIP_TRY(c, hipMemsetAsync(da.brick_res, 0xff, map_bytes, cur(c).stream.get()));
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
        c->dyn = VctDynamic();                // (the draw flags and the bounce switch are context state: c->dyn_settings)
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
    HIP_TRY(c, alloc_bytes(d.pos, z.pos));
    HIP_TRY(c, alloc_bytes(d.mat, z.material));
    HIP_TRY(c, alloc_bytes(d.albedo, z.albedo));
    HIP_TRY(c, alloc_bytes(d.big_list, z.big_list));
    HIP_TRY(c, hipMemcpyAsync(d.pos.get(), pos, z.pos, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d.mat.get(), material, z.material, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d.albedo.get(), albedo, z.albedo, hipMemcpyHostToDevice, s));
    HIP_TRY(c, alloc_filled(d.words, z.words, 0, s));
    HIP_TRY(c, alloc_filled(d.brick_slot, z.brick_slot, 0xff, s));
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
    HIP_TRY(c, alloc_filled(d.slot_brick, z.slot_list, 0, s));
    HIP_TRY(c, alloc_filled(d.res_brick, z.slot_list, 0, s));
    HIP_TRY(c, alloc_filled(d.acc, z.acc, 0, s));
    HIP_TRY(c, alloc_filled(d.pool_rad, z.pool, 0, s));
    if (attr) {
        HIP_TRY(c, alloc_filled(d.acc_attr, z.acc_attr, 0, s));
        HIP_TRY(c, alloc_filled(d.pool_alb, z.pool, 0, s));
        HIP_TRY(c, alloc_filled(d.pool_nrm, z.pool, 0, s));
    }
    HIP_TRY(c, d.vox_timer.create());           // the events now, so that no pass allocates
    HIP_TRY(c, d.merge_timer.create());
    if (c->dyn_settings.draw_flags) PIPE_TRY(draw_prepare(c, d, s));      // drawn: the draw copy and the frames of these positions
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
    if (c->dyn.matrices()) {              // parts or a skin attached: these positions are the new rest positions as well
        HIP_TRY(c, hipMemcpyAsync(c->dyn.mover.rest.get(), c->dyn.pos.get(), (size_t)c->dyn.ntri * 9 * sizeof(float),
                                  hipMemcpyDeviceToDevice, cur(c).stream.get()));
        c->dyn.mover.moved = false;
    }
    return vct_dynamic_draw_prepare(c);   // behind the copy, on its stream: ordered before every stage that draws the mesh
}

int vct_set_dynamic_parts(vct_ctx* c, const int32_t* part, int32_t nparts) {
    if (!c) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    if (!part && nparts == 0) return detach_mover(c, "vct_set_dynamic_parts", VCT_MOVER_PARTS);
    int32_t bad = -1;
    if (const char* why = vct_dynamic_check_parts(d.attached(), part, d.ntri, nparts, &bad)) {
        if (bad < 0) return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_parts: ") + why);
        char msg[160];
        snprintf(msg, sizeof msg, "vct_set_dynamic_parts: part index %d of triangle %d is outside 0 .. %d", (int)part[bad],
                 (int)bad, (int)nparts - 1);
        return vct_fail(c, VCT_ERR_INVALID, msg);
    }
    const VctDynamicPartsSizes z = vct_dynamic_parts_sizes(d.ntri, nparts);
    return attach_mover(c, "vct_set_dynamic_parts", VCT_MOVER_PARTS, nparts, {z.ok, z.rest, z.table},
                        [&](VctDynamic::Mover& v, hipStream_t s) { return alloc_copied(v.part, part, z.part, s); });
}

int vct_get_dynamic_parts(vct_ctx* c, int32_t* nparts, int32_t* part) {
    if (!c || !nparts) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    *nparts = d.mover.kind == VCT_MOVER_PARTS ? d.mover.n : 0;
    if (!*nparts || !part) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(part, d.mover.part.get(), (size_t)d.ntri * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VCT_OK;
}

int vct_set_dynamic_skin(vct_ctx* c, const int32_t* bone, const float* weight, int32_t nbones) {
    if (!c) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    if (!bone && !weight && nbones == 0) return detach_mover(c, "vct_set_dynamic_skin", VCT_MOVER_SKIN);
    size_t bad = 0;
    if (const char* why = vct_dynamic_check_skin(d.attached(), bone, weight, d.ntri, nbones, &bad)) {
        if (bad == (size_t)-1) return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_skin: ") + why);
        char msg[200];
        const int tri = (int)(bad / 12), corner = (int)(bad / 4 % 3), slot = (int)(bad % 4);
        if (bone[bad] < 0 || bone[bad] >= nbones)
            snprintf(msg, sizeof msg, "vct_set_dynamic_skin: bone index %d of triangle %d, corner %d, slot %d is outside 0 .. %d",
                     (int)bone[bad], tri, corner, slot, (int)nbones - 1);
        else
            snprintf(msg, sizeof msg, "vct_set_dynamic_skin: weight %g of triangle %d, corner %d, slot %d is not finite",
                     (double)weight[bad], tri, corner, slot);
        return vct_fail(c, VCT_ERR_INVALID, msg);
    }
    const VctDynamicSkinSizes z = vct_dynamic_skin_sizes(d.ntri, nbones);
    std::vector<uint16_t> packed((size_t)d.ntri * 12);      // checked above: every index is below nbones <= 2^16
    for (size_t i = 0; i < packed.size(); ++i) packed[i] = (uint16_t)bone[i];
    return attach_mover(c, "vct_set_dynamic_skin", VCT_MOVER_SKIN, nbones, {z.ok, z.rest, z.table},
                        [&](VctDynamic::Mover& v, hipStream_t s) {      // (the attach waits for the stream: `packed` outlives the copy)
                            const hipError_t e = alloc_copied(v.bone, packed.data(), z.bone, s);
                            return e == hipSuccess ? alloc_copied(v.weight, weight, z.weight, s) : e;
                        });
}

int vct_get_dynamic_skin(vct_ctx* c, int32_t* nbones, int32_t* bone, float* weight) {
    if (!c || !nbones) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    *nbones = d.mover.kind == VCT_MOVER_SKIN ? d.mover.n : 0;
    if (!*nbones) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)d.ntri * 12;
    if (bone) {
        std::vector<uint16_t> packed(n);
        HIP_TRY(c, hipMemcpy(packed.data(), d.mover.bone.get(), n * sizeof(uint16_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) bone[i] = (int32_t)packed[i];
    }
    if (weight) HIP_TRY(c, hipMemcpy(weight, d.mover.weight.get(), n * sizeof(float), hipMemcpyDeviceToHost));
    return VCT_OK;
}

int vct_update_dynamic_transforms(vct_ctx* c, const float* m, int32_t location) {
    if (!c) return VCT_ERR_INVALID;
    VctDynamic& d = c->dyn;
    if (const char* why = vct_dynamic_check_transforms(d.attached(), d.matrices(), m, location))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_update_dynamic_transforms: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_join(c));       // positions and table are shared: the other slot's pass may still read the positions
    hipStream_t s = cur(c).stream.get();
    HIP_TRY(c, hipMemcpyAsync(d.mover.m.get(), m, (size_t)d.matrices() * 12 * sizeof(float),
                              location == VCT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    d.mover.moved = true;
    HIP_TRY(c, d.mover.timer.begin(s, c->time_traces));
    PIPE_TRY(transform(c, d, s, c->dyn_settings.draw_flags && d.draw.pos));
    HIP_TRY(c, d.mover.timer.end(s));
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

int vct_set_dynamic_normals(vct_ctx* c, const float* nrm) {
    if (!c) return VCT_ERR_INVALID;
    VctDynamic& d = c->dyn;
    if (const char* why = vct_dynamic_check_normals(d.attached(), d.ntri))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_normals: ") + why);
    if (!nrm && !d.corner_nrm) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // a prepare kernel in flight reads the previous array
    hipStream_t s = cur(c).stream.get();
    VctBuf<float> n;                      // all or nothing: the new array (none: detach) in a local until everything has succeeded
    if (nrm) {
        const size_t bytes = vct_dynamic_normals_bytes(d.ntri);
        HIP_TRY(c, alloc_bytes(n, bytes));
        HIP_TRY(c, hipMemcpyAsync(n.get(), nrm, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));      // the caller's array is free again
    }
    std::swap(d.corner_nrm, n);
    // drawn: the frames of these normals, or the face frames again.  (Under a moved mover this is the mover's own kernel,
    // which also rewrites the layer's positions with the values they have: everything in flight was waited for above.)
    const int rc = vct_dynamic_draw_prepare(c);
    if (rc != VCT_OK) std::swap(d.corner_nrm, n);
    return rc;
}

int vct_update_dynamic_normals(vct_ctx* c, const float* nrm, int32_t location) {
    if (!c) return VCT_ERR_INVALID;
    VctDynamic& d = c->dyn;
    if (const char* why = vct_dynamic_check_normals_update(d.attached(), (bool)d.corner_nrm, nrm, location))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_update_dynamic_normals: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_join(c));       // the array is shared: the other slot's prepare kernel may still read the previous normals
    HIP_TRY(c, hipMemcpyAsync(d.corner_nrm.get(), nrm, vct_dynamic_normals_bytes(d.ntri),
                              location == VCT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, cur(c).stream.get()));
    // behind the copy, on its stream.  (Under a moved mover the prepare is the mover's own kernel, which also rewrites the
    // layer's positions with the values they have; the join above has waited for the other slot's readers.)
    return vct_dynamic_draw_prepare(c);
}

int vct_get_dynamic_normals(vct_ctx* c, int32_t* attached, float* nrm) {
    if (!c || !attached) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    *attached = d.corner_nrm ? 1 : 0;
    if (!*attached || !nrm) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // the last update may have been issued on the other frame slot's stream
    HIP_TRY(c, hipMemcpy(nrm, d.corner_nrm.get(), vct_dynamic_normals_bytes(d.ntri), hipMemcpyDeviceToHost));
    return VCT_OK;
}

int vct_download_dynamic_frames(vct_ctx* c, float* nrm, float* tan, float* bit) {
    if (!c) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    if (const char* why = vct_dynamic_check_frames(d.attached(), c->dyn_settings.draw_flags, (bool)d.draw.pos))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_download_dynamic_frames: ") + why);
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));         // the last prepare kernel may have been issued on the other frame slot's stream
    const float* src[3] = {d.draw.nrm.get(), d.draw.tan.get(), d.draw.bit.get()};
    float* dst[3] = {nrm, tan, bit};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) HIP_TRY(c, hipMemcpy(dst[k], src[k], vct_dynamic_draw_floats(d.ntri) * sizeof(float), hipMemcpyDeviceToHost));
    return VCT_OK;
}

int vct_last_dynamic_transform_ms(vct_ctx* c, float* ms) {
    if (!c || !ms) return VCT_ERR_INVALID;
    const char* never = "vct_last_dynamic_transform_ms: needs parts or a skin attached and a vct_update_dynamic_transforms since";
    const char* untimed = "vct_last_dynamic_transform_ms: the last transform was issued with timing off (vct_set_trace_timing)";
    if (!c->dyn.matrices() || !c->dyn.mover.timer.have) return vct_fail(c, VCT_ERR_INVALID, never);
    return vct_timer_ms(c, c->dyn.mover.timer, ms, never, untimed);
}

int vct_set_dynamic_draw(vct_ctx* c, int32_t flags, const float specular[3]) {
    if (!c) return VCT_ERR_INVALID;
    if (const char* why = vct_dynamic_check_draw(flags, specular))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_draw: ") + why);
    VctDynamicSettings& k = c->dyn_settings;
    const bool goes_on = flags && !k.draw_flags;
    if (goes_on && c->dyn.attached()) {
        // the draw copy is shared by both slots like the positions: the other slot's pass may still read the previous one
        HIP_TRY(c, hipSetDevice(c->device));
        PIPE_TRY(vct_pipeline_join(c));
        // (with corner normals under a moved mover this is the mover's own kernel: it rewrites the positions as they are)
        PIPE_TRY(draw_prepare(c, c->dyn, cur(c).stream.get()));
    }
    k.draw_flags = flags;
    for (int i = 0; i < 3; ++i) k.draw_specular[i] = specular ? specular[i] : 0.0f;
    return VCT_OK;
}

int vct_get_dynamic_draw(vct_ctx* c, int32_t* flags, float specular[3]) {
    if (!c || !flags || !specular) return VCT_ERR_INVALID;
    *flags = c->dyn_settings.draw_flags;
    for (int k = 0; k < 3; ++k) specular[k] = c->dyn_settings.draw_specular[k];
    return VCT_OK;
}

int vct_set_dynamic_bounce(vct_ctx* c, int32_t on) {
    if (!c) return VCT_ERR_INVALID;
    if (const char* why = vct_dynamic_check_bounce(on))
        return vct_fail(c, VCT_ERR_INVALID, std::string("vct_set_dynamic_bounce: ") + why);
    c->dyn_settings.bounce_on = on;      // read by the next vct_bounce; nothing in flight depends on it
    return VCT_OK;
}

int vct_get_dynamic_bounce(vct_ctx* c, int32_t* on) {
    if (!c || !on) return VCT_ERR_INVALID;
    *on = c->dyn_settings.bounce_on;
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
        d.emis = VctDynamic::Emission();
        d.pass.emis = false;
        vct_emission_planes_release(c);
        return VCT_OK;
    }
    // all or nothing: the table and (for a first table) the zeroed sums in locals, planes only for slots that have none.
    // A replaced table keeps the sums: a pending pass resolves with the table it was voxelized under.
    const VctDynamicEmissionSizes z = vct_dynamic_emission_sizes(d.nmat, d.max_bricks);
    if (!z.ok) return vct_fail(c, VCT_ERR_INVALID, "vct_set_dynamic_emission: buffer sizes overflow");
    std::vector<float> padded((size_t)d.nmat * 4);
    vct_emission_pad(emission, d.nmat, padded.data());
    VctDynamic::Emission n;
    hipError_t e = alloc_bytes(n.table, z.table);
    if (e == hipSuccess) e = hipMemcpy(n.table.get(), padded.data(), z.table, hipMemcpyHostToDevice);
    if (e == hipSuccess && !d.emis.acc) e = alloc_filled(n.acc, z.sums, 0, cur(c).stream.get());      // (vct_planes_attach waits for the stream)
    PIPE_TRY(vct_planes_attach(c, "vct_set_dynamic_emission", vct_emission_planes, vct_emission_planes_drop, e));
    if (!d.emis.acc) { d.emis.acc = std::move(n.acc); d.pass.emis = false; }      // attached behind a vct_voxelize: that pass has none
    d.emis.table = std::move(n.table);
    return VCT_OK;
}

int vct_get_dynamic_emission(vct_ctx* c, float* emission, int32_t* nmat) {
    if (!c || !nmat) return VCT_ERR_INVALID;
    const VctDynamic& d = c->dyn;
    *nmat = d.emis.table ? d.nmat : 0;
    if (!d.emis.table || !emission) return VCT_OK;
    std::vector<float> padded((size_t)d.nmat * 4);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(padded.data(), d.emis.table.get(), padded.size() * sizeof(float), hipMemcpyDeviceToHost));
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
    HIP_TRY(c, hipMemcpyAsync(st, resolved_stats(d), sizeof st, hipMemcpyDeviceToHost, cur(c).stream.get()));
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
    for (int k = 0; k < 3; ++k) {      // a pooled volume of the last resolved pass -> dense Morton -> linear staging -> host
        if (!dst[k]) continue;
        HIP_TRY(c, vct_launch_dynamic_unpool(src[k], d.res_brick.get(), d.words.get(), d.pass.set, d.max_bricks, (uint32_t)c->vol.nbricks(), dense.get(), cur(c).stream.get()));
        PIPE_TRY(vct_download_level(c, dense.get(), c->vol.V, dst[k]));
    }
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
