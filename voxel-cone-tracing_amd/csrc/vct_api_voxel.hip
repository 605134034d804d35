// vct_api_voxel.hip -- the C ABI's voxel stages: voxelize, inject, mips, bounce, and the up/downloads of the volume.
#include "vct_ctx.h"

namespace {

// glm::ortho / glm::lookAt(eye, origin, up) / mat4 product as the reference builds ProjX/Y/Z
// (VCT.h:128-134; glm defaults: right-handed, NDC z in [-1,1]); column-major, fp32, one rounding per
// operation -- the same operation order as the oracle's restatement.
void glm_ortho(float l, float r, float b, float t, float n, float f, float m[16]) {
    memset(m, 0, 64);
    m[0] = 2.0f / (r - l);
    m[5] = 2.0f / (t - b);
    m[10] = -2.0f / (f - n);
    m[12] = -(r + l) / (r - l);
    m[13] = -(t + b) / (t - b);
    m[14] = -(f + n) / (f - n);
    m[15] = 1.0f;
}
void glm_lookat_origin(const float eye[3], const float up[3], float m[16]) {
    auto norm3 = [](float v[3]) {
        const float l = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        v[0] = v[0] / l; v[1] = v[1] / l; v[2] = v[2] / l;
    };
    auto cross = [](const float a[3], const float b[3], float o[3]) {
        o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
    };
    auto dot = [](const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    float f[3] = {0.0f - eye[0], 0.0f - eye[1], 0.0f - eye[2]}, s[3], u[3];
    norm3(f);
    cross(f, up, s);
    norm3(s);
    cross(s, f, u);
    memset(m, 0, 64);
    m[0] = s[0]; m[4] = s[1]; m[8] = s[2];
    m[1] = u[0]; m[5] = u[1]; m[9] = u[2];
    m[2] = -f[0]; m[6] = -f[1]; m[10] = -f[2];
    m[12] = -dot(s, eye); m[13] = -dot(u, eye); m[14] = dot(f, eye);
    m[15] = 1.0f;
}
void mat_mul(const float a[16], const float b[16], float o[16]) {      // column-major o = a * b
    float t[16];
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            float s = 0.0f;
            for (int k = 0; k < 4; ++k) s += a[k * 4 + r] * b[c * 4 + k];
            t[c * 4 + r] = s;
        }
    memcpy(o, t, sizeof(t));
}

}  // namespace

VctVoxParams vct_vox_params_scene(const vct_ctx* c) {
    VctVoxParams p;
    memset(&p, 0, sizeof(p));
    p.V = c->cfg.voxel_dim;
    p.G = c->cfg.grid_world_size;
    p.model_scale = c->cfg.model_scale;
    p.shadow = c->shadow.words.get();
    p.shadow_tiles = c->shadow.words ? c->shadow.tiles.get() : nullptr;
    p.shadow_ebase = c->shadow.ebase;
    p.shadow_size = c->shadow.size;
    memcpy(p.light_vp, c->shadow.light_vp, 64);
    return p;
}

VctVoxParams vct_vox_params(const vct_ctx* c, const VctVoxelPlan& v) {
    VctVoxParams p = vct_vox_params_scene(c);
    p.pos = c->mesh.tri_pos.get();
    p.material = c->mesh.tri_mat.get();
    p.albedo = c->mesh.mat_albedo.get();
    p.ntri = c->mesh.ntri;
    p.acc = v.acc.get();
    p.brick_slot = v.brick_slot.get();
    p.frag_sorted = v.frag_sorted.get();
    p.frag_bary = v.frag_bary.get();
    p.frag_alb = nullptr;       // vct_voxelize attaches it (scenes with textures)
    p.tri_qnrm = v.tri_qnrm.get();
    p.slot_first = v.slot_first.get();
    p.slot_brick = v.slot_brick.get();
    p.items = v.items.get();
    p.nitems = v.n_items;
    p.acc2 = v.acc2.get();
    p.acc2_attr = v.acc2_attr.get();
    p.multi_slot = v.multi_slot.get();
    p.nmulti = v.n_multi;
    p.nslots = v.nslots;
    p.stage = v.stage.get();
    p.stage_albedo = v.stage_albedo.get();
    p.stage_normal = v.stage_normal.get();
    p.brick_flags = c->vol.brick_flags.get();
    p.tex = vct_textures_of(c);
    return p;
}

void vct_glm_voxel_projections(const vct_ctx* c, float proj[48]) {
    // VCT.h:128-134: ortho(-G/2, G/2, -G/2, G/2, G/2, 3G/2) * lookAt(+-G on the axis) per dominant axis
    const float G = c->cfg.grid_world_size, h = G * 0.5f;
    float o[16], v[16];
    glm_ortho(-h, h, -h, h, h, G * 1.5f, o);
    const float eye[3][3] = {{G, 0, 0}, {0, G, 0}, {0, 0, G}};
    const float up[3][3] = {{0, 1, 0}, {0, 0, -1}, {0, 1, 0}};
    for (int a = 0; a < 3; ++a) {
        glm_lookat_origin(eye[a], up[a], v);
        mat_mul(o, v, proj + 16 * a);
    }
}

int vct_light_voxels(vct_ctx* c, const uint32_t* attr_albedo, const uint32_t* attr_normal, const uint32_t* slot_brick, uint32_t nslots) {
    VctLightVoxArgs la;
    memset(&la, 0, sizeof(la));
    la.lights = c->lights.table.get(); la.nlights = c->lights.n;
    la.V = c->cfg.voxel_dim; la.G = c->cfg.grid_world_size;
    la.level0 = c->vol.chain.get(); la.attr_albedo = attr_albedo; la.attr_normal = attr_normal;
    la.slot_brick = slot_brick; la.brick_prev = c->vol.brick_prev.get(); la.nslots = nslots;
    HIP_TRY(c, vct_launch_light_voxels(la, cur(c).stream.get()));
    return VCT_OK;
}

int vct_download_level(vct_ctx* c, const uint32_t* morton, int N, uint8_t* dst) {
    PIPE_TRY(vct_staging_free(c));
    HIP_TRY(c, c->vol.staging.reserve(c->vol.nvox()));
    HIP_TRY(c, vct_launch_morton_to_linear(morton, c->vol.staging.get(), N, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(dst, c->vol.staging.get(), (size_t)N * N * N * 4, hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

extern "C" {

int vct_voxelize(vct_ctx* c, int32_t mode) {
    if (!c) return VCT_ERR_INVALID;
    if (mode != VCT_VOX_CONSERVATIVE_AVG && mode != VCT_VOX_REFERENCE) return vct_fail(c, VCT_ERR_INVALID, "vct_voxelize: unknown mode");
    if (!c->mesh.tri_pos) return vct_fail(c, VCT_ERR_INVALID, "vct_voxelize: no triangles uploaded");
    if (mode == VCT_VOX_REFERENCE && c->mesh.mat_emission)
        return vct_fail(c, VCT_ERR_INVALID, "vct_voxelize: VCT_VOX_REFERENCE is the reference's shaders as written and has no emission "
                                        "(vct_upload_emission(ctx, NULL) first)");
    if (mode == VCT_VOX_REFERENCE && c->lights.n)
        return vct_fail(c, VCT_ERR_INVALID, "vct_voxelize: VCT_VOX_REFERENCE is the reference's shaders as written and has no local lights "
                                        "(vct_set_lights(ctx, NULL, 0) first)");
    if (mode == VCT_VOX_REFERENCE && c->dyn.attached())
        return vct_fail(c, VCT_ERR_INVALID, "vct_voxelize: VCT_VOX_REFERENCE is the reference's shaders as written and has no dynamic mesh "
                                        "(vct_set_dynamic_mesh(ctx, NULL, ...) first)");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_join(c));       // the staging pool is shared: the other slot's resolve may still read the previous pass
    if (!c->vox.brick_slot || !c->vox.stage || (mode == VCT_VOX_REFERENCE && !c->vox.ref_big))
        return vct_fail(c, VCT_ERR_NOMEM, "vct_voxelize: the voxelization plan of this mesh could not be allocated "
                                      "(vct_upload_triangles reported it)");
    const size_t pool_vox = (size_t)(c->vox.nslots ? c->vox.nslots : 1u) * 512;
    VctVoxelPlan& v = c->vox;
    if (mode == VCT_VOX_REFERENCE && !v.acc) {       // reference mode's accumulators: allocated on first use, zeroed once
        HIP_TRY(c, v.acc.alloc(pool_vox * 2));
        HIP_TRY(c, hipMemsetAsync(v.acc.get(), 0, pool_vox * 16, cur(c).stream.get()));
    }
    if (v.acc_pending) {   // a pass that was never resolved: discard it
        if (c->acc_mode == VCT_VOX_REFERENCE && v.acc) HIP_TRY(c, hipMemsetAsync(v.acc.get(), 0, pool_vox * 16, cur(c).stream.get()));
        HIP_TRY(c, hipMemsetAsync(c->vol.brick_flags.get(), 0, c->vol.nbricks() * sizeof(uint32_t), cur(c).stream.get()));
    }
    VctVoxParams p = vct_vox_params(c, v);
    if (mode == VCT_VOX_REFERENCE) {
        vct_glm_voxel_projections(c, p.proj);
        HIP_TRY(c, vct_launch_voxelize_reference(p, v.ref_big.get() + 1, v.ref_big.get(), cur(c).stream.get()));
    } else {
        v.pass_emis = false;
        if (c->mesh.mat_emission && v.emis_pool) {
            // Emission pool: the brick pass itself over the same sorted fragments with the emission table as the colour
            // table, no shadow map (PCF = 1) and no per-fragment albedo, resolved into the pool instead of the staging
            // slots -- multi-chunk slots through the same accumulators, which their resolve leaves zero for the pass
            // below.  Once per (mesh, table).  It raises the brick flags of exactly the slots the pass below raises.
            if (v.emis_dirty) {
                VctVoxParams q = p;
                q.albedo = c->mesh.mat_emission.get();
                q.shadow = nullptr; q.shadow_tiles = nullptr;
                q.stage = v.emis_pool.get(); q.stage_albedo = nullptr; q.stage_normal = nullptr;
                HIP_TRY(c, vct_launch_voxelize(q, cur(c).stream.get()));
                v.emis_dirty = false;
            }
            v.pass_emis = true;
        }
        if (p.tex.texels && v.n_frags) {
            // every fragment's albedo (texture fetch or material colour): independent of the light, so evaluated once per
            // change of the textures / texture coordinates, not once per pass
            HIP_TRY(c, v.frag_alb.reserve((size_t)v.n_frags * 3, &v.frag_alb_dirty));
            if (v.frag_alb_dirty) {
                HIP_TRY(c, vct_launch_frag_geom(p, nullptr, v.frag_alb.get(), cur(c).stream.get()));
                v.frag_alb_dirty = false;
            }
            p.frag_alb = v.frag_alb.get();
        }
        HIP_TRY(c, vct_launch_voxelize(p, cur(c).stream.get()));      // one workgroup per brick: LDS accumulation + resolve into the staging pool
        PIPE_TRY(vct_dynamic_voxelize(c));     // the dynamic mesh, if one is attached, by itself into its own accumulators
    }
    v.acc_pending = true;
    c->acc_mode = mode;
    return VCT_OK;
}

int vct_inject_light(vct_ctx* c) {
    if (!c) return VCT_ERR_INVALID;
    if (!c->vox.acc_pending) return vct_fail(c, VCT_ERR_INVALID, "vct_inject_light: call vct_voxelize first");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_join(c));       // level 0 is rewritten: the other slot's trace may still read the chain
    const VctVoxelPlan& v = c->vox;
    VctResolveArgs a;
    memset(&a, 0, sizeof(a));
    a.level0 = c->vol.chain.get(); a.flags = c->vol.brick_flags.get(); a.prev = c->vol.brick_prev.get(); a.brick_slot = v.brick_slot.get();
    if (c->acc_mode == VCT_VOX_REFERENCE) a.acc = v.acc.get();
    else {
        a.stage = v.stage.get(); a.stage_albedo = v.stage_albedo.get(); a.stage_normal = v.stage_normal.get();
        a.attr_albedo = v.attr_albedo.get(); a.attr_normal = v.attr_normal.get();
        if (v.pass_emis && v.emis_pool) a.emis = v.emis_pool.get();
    }
    HIP_TRY(c, vct_launch_resolve(a, c->cfg.voxel_dim, c->vol.level0_dirty, cur(c).stream.get()));
    // local lights (include/vct.h "local lights"): their direct term into the bricks the resolve has just written
    if (c->lights.n && c->acc_mode == VCT_VOX_CONSERVATIVE_AVG && v.attr_albedo) {
        HIP_TRY(c, c->lights.vox_timer.begin(cur(c).stream.get(), c->time_traces));
        PIPE_TRY(vct_light_voxels(c, v.attr_albedo.get(), v.attr_normal.get(), v.slot_brick.get(), v.nslots));
        HIP_TRY(c, c->lights.vox_timer.end(cur(c).stream.get()));
    }
    // the dynamic mesh wins per voxel (include/vct.h "dynamic mesh"): behind the static resolve and its lights
    PIPE_TRY(vct_dynamic_merge(c));
    c->vox.acc_pending = false;
    c->vol.level0_resolved();
    c->vox.attrs_valid = c->vox.attr_normal && c->acc_mode == VCT_VOX_CONSERVATIVE_AVG;
    return VCT_OK;
}

// Footprint records of the levels >= 1 (vct_set_footprint_records), rebuilt after every change of those levels.
// Dense: 8 x the bytes of those levels = 1.14 x level 0 written per build (0.04 ms at 256^3, 2.0 ms at 1024^3).
static int build_cells(vct_ctx* c) {
    c->vol.records_valid(false);
    if (!c->vol.want_cells || c->vol.nlev < 2) return VCT_OK;
    if (!c->vol.cells) {
        const hipError_t e = c->vol.cells.alloc((c->vol.chain_texels - c->vol.nvox()) * 2);
        if (e != hipSuccess) { return vct_fail(c, VCT_ERR_NOMEM, std::string("footprint records: ") + hipGetErrorString(e)); }
    }
    HIP_TRY(c, vct_launch_build_cells(c->vol.chain.get(), c->vol.cells.get(), c->cfg.voxel_dim, cur(c).stream.get()));
    c->vol.records_valid(true);
    return VCT_OK;
}

int vct_set_footprint_records(vct_ctx* c, int32_t on) {
    if (!c) return VCT_ERR_INVALID;
    if (on) PIPE_TRY(vct_refuse_conflict(c, "vct_set_footprint_records", vct_rules_in_force(c).features, VCT_MODE_CELLS));
    HIP_TRY(c, hipSetDevice(c->device));
    c->vol.want_cells = on != 0;
    PIPE_TRY(vct_pipeline_drain(c));
    if (!c->vol.want_cells) {
        c->vol.records_valid(false);
        if (c->vol.cells) {
            HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));      // a trace in flight may still read them
            c->vol.cells.reset();
        }
        return VCT_OK;
    }
    return c->vol.mips_valid ? build_cells(c) : VCT_OK;           // a valid chain gets its records now, otherwise at the next build
}

int vct_build_mips(vct_ctx* c) {
    if (!c) return VCT_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_join(c));
    // sparse where the chain's state allows it (vct_ctx.h VctChain); a dense build "sees" every brick as it is now
    VctChain& vol = c->vol;
    const bool sparse = vol.sparse_mips_ok();
    if (!sparse && vol.mip_seen && vol.brick_prev)
        HIP_TRY(c, hipMemcpyAsync(vol.mip_seen.get(), vol.brick_prev.get(), vol.nbricks() * sizeof(uint32_t), hipMemcpyDeviceToDevice, cur(c).stream.get()));
    HIP_TRY(c, vct_launch_build_mips(vol.chain.get(), vol.V, sparse ? vol.brick_prev.get() : nullptr, sparse ? vol.mip_seen.get() : nullptr,
                                     cur(c).stream.get()));
    vol.mips_reduced(sparse);
    if (vol.aniso) HIP_TRY(c, vct_launch_build_mips_aniso(vol.chain.get(), vol.aniso.get(), vol.V, cur(c).stream.get()));
    vol.mips_built();
    return build_cells(c);
}

int vct_bounce(vct_ctx* c) {
    if (!c) return VCT_ERR_INVALID;
    if (vct_dynamic_blocks_bounce(c))      // the plain bounce walks the static slots and their attributes only
        return vct_fail(c, VCT_ERR_INVALID, "vct_bounce: a dynamic mesh is attached and the second bounce does not see its voxels "
                                        "(vct_set_dynamic_mesh(ctx, NULL, ...) first)");
    if (!c->cfg.voxel_attributes || !c->vox.attr_normal)
        return vct_fail(c, VCT_ERR_INVALID, "vct_bounce: needs config.voxel_attributes = 1 and a voxelize + inject pass");
    if (c->vox.acc_pending || !c->vol.mips_valid)
        return vct_fail(c, VCT_ERR_INVALID, "vct_bounce: call vct_inject_light and vct_build_mips first");
    if (!c->vox.attrs_valid)      // a new mesh was uploaded since: level 0 / brick_prev describe the OLD mesh, the slots the new one
        return vct_fail(c, VCT_ERR_INVALID, "vct_bounce: the voxel attributes belong to a mesh uploaded after the last "
                                        "vct_inject_light (voxelize + inject + mips again first)");
    if (c->vol.level0_dirty || c->acc_mode != VCT_VOX_CONSERVATIVE_AVG)
        return vct_fail(c, VCT_ERR_INVALID, "vct_bounce: level 0 must come from a VCT_VOX_CONSERVATIVE_AVG pass (voxel attributes)");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_drain(c));      // (allocates the second chain on first use)
    PIPE_TRY(vct_refresh_steps(c));
    const size_t nvox = c->vol.nvox(), nbricks = c->vol.nbricks();
    bool b_sparse = (bool)c->vol.chain_b;
    if (!c->vol.chain_b) {
        HIP_TRY(c, c->vol.chain_b.alloc(c->vol.chain_texels));
        HIP_TRY(c, hipMemsetAsync(c->vol.chain_b.get(), 0, c->vol.chain_texels * 4, cur(c).stream.get()));
        HIP_TRY(c, c->vol.mip_seen_b.alloc(nbricks));
        HIP_TRY(c, hipMemsetAsync(c->vol.mip_seen_b.get(), 0, nbricks * sizeof(uint32_t), cur(c).stream.get()));
        b_sparse = true;     // zero-filled chain + empty "seen" set: the sparse form is valid from the start
        // occupied-voxel list: surfaces occupy ~1 % of a grid; V^3/8 entries is a generous bound and
        // bricks that do not fit are handled by the per-brick kernel
        HIP_TRY(c, c->bounce_list.alloc(nvox / 8 + 1));      // (+ the counter word in front)
        HIP_TRY(c, c->brick_over.alloc(nbricks));
        HIP_TRY(c, hipMemsetAsync(c->brick_over.get(), 0, nbricks * sizeof(uint32_t), cur(c).stream.get()));   // k_bounce_bricks resets what it serves
    }
    // only the counter: the list itself needs no clear (the one brick that can straddle its end marks its tail empty)
    HIP_TRY(c, hipMemsetAsync(c->bounce_list.get(), 0, sizeof(uint32_t), cur(c).stream.get()));
    VctTraceParams p;
    vct_fill_march_params(c, p, c->vol.chain.get());
    p.attr_albedo = c->vox.attr_albedo.get();
    p.attr_normal = c->vox.attr_normal.get();
    p.brick_slot = c->vox.brick_slot.get();
    p.brick_prev = c->vol.brick_prev.get();
    p.bounce_seen = c->vol.mip_seen_b.get();
    p.bounce_out = c->vol.chain_b.get();
    p.nbricks = (uint32_t)nbricks;
    p.slot_brick = c->vox.slot_brick.get();
    p.nslots = c->vox.nslots;
    p.bounce_list_count = c->bounce_list.get();
    p.bounce_list = c->bounce_list.get() + 1;
    p.bounce_list_cap = (uint32_t)(c->bounce_list.size() - 1);
    p.brick_over = c->brick_over.get();
    HIP_TRY(c, hipMemsetAsync(c->step_counter.get(), 0, VCT_STEP_COUNTERS * sizeof(unsigned long long), cur(c).stream.get()));
    HIP_TRY(c, cur(c).march.begin(cur(c).stream.get(), c->time_traces));
    // the dynamic layer in the chain (include/vct.h "dynamic mesh", the second bounce): the DYN kernels and their table
    VctBounceDynArgs da;
    bool dyn = false;
    PIPE_TRY(vct_dynamic_bounce_args(c, da, &dyn));
    HIP_TRY(c, vct_launch_bounce(p, cur(c).stream.get(), dyn ? &da : nullptr));
    HIP_TRY(c, cur(c).march.end(cur(c).stream.get()));      // step counter / event pair now describe the bounce launch
    c->last_march_form = c->fast_div ? 2 : 1;
    HIP_TRY(c, vct_launch_build_mips(c->vol.chain_b.get(), c->cfg.voxel_dim, b_sparse ? c->vol.brick_prev.get() : nullptr,
                                     b_sparse ? c->vol.mip_seen_b.get() : nullptr, cur(c).stream.get()));
    // the directional chains always describe the chain the trace reads (the bounce itself gathers
    // from the isotropic bounce-0 chain, like the oracle's vcto_bounce)
    if (c->vol.aniso) HIP_TRY(c, vct_launch_build_mips_aniso(c->vol.chain_b.get(), c->vol.aniso.get(), c->cfg.voxel_dim, cur(c).stream.get()));
    c->vol.bounce_done();
    cur(c).last_was_screen_trace = false;
    return VCT_OK;
}

int vct_download_voxel_attributes(vct_ctx* c, uint8_t* albedo, uint8_t* normal) {
    if (!c || !albedo || !normal) return VCT_ERR_INVALID;
    if (!c->vox.attr_albedo) return vct_fail(c, VCT_ERR_INVALID, "no voxel attributes (config.voxel_attributes, vct_voxelize + vct_inject_light)");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t* src[2] = {c->vox.attr_albedo.get(), c->vox.attr_normal.get()};
    uint8_t* dst[2] = {albedo, normal};
    VctBuf<uint32_t> dense;             // pooled [slot][512] -> dense Morton volume -> linear staging
    HIP_TRY(c, dense.alloc(c->vol.nvox()));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(c, vct_launch_unpool(src[k], c->vox.brick_slot.get(), dense.get(), (uint32_t)c->vol.nbricks(), cur(c).stream.get()));
        PIPE_TRY(vct_download_level(c, dense.get(), c->vol.V, dst[k]));
    }
    return VCT_OK;
}

// ---- volume up/download -----------------------------------------------------------------

static int upload_levels(vct_ctx* c, const uint8_t* lin, int nlevels) {
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_drain(c));
    c->vol.level0_uploaded(nlevels > 1);
    HIP_TRY(c, c->vol.staging.reserve(c->vol.nvox()));
    const int V = c->cfg.voxel_dim;
    for (int l = 0; l < nlevels; ++l) {
        const int N = V >> l;
        const size_t off = (size_t)vct_level_offset(V, l), n = (size_t)N * N * N;
        HIP_TRY(c, hipMemcpyAsync(c->vol.staging.get(), lin + off * 4, n * 4, hipMemcpyHostToDevice, cur(c).stream.get()));
        HIP_TRY(c, vct_launch_linear_to_morton(c->vol.staging.get(), c->vol.chain.get() + off, N, cur(c).stream.get()));
        HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    }
    return VCT_OK;
}

int vct_upload_volume_rgba8(vct_ctx* c, const uint8_t* l0) {
    if (!c) return VCT_ERR_INVALID;
    if (!l0) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_volume_rgba8: null volume");
    return upload_levels(c, l0, 1);
}

int vct_upload_chain_rgba8(vct_ctx* c, const uint8_t* chain) {
    if (!c) return VCT_ERR_INVALID;
    if (!chain) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_chain_rgba8: null chain");
    PIPE_TRY(upload_levels(c, chain, c->vol.nlev));
    if (c->vol.aniso) HIP_TRY(c, vct_launch_build_mips_aniso(c->vol.chain.get(), c->vol.aniso.get(), c->cfg.voxel_dim, cur(c).stream.get()));
    return build_cells(c);
}

int vct_download_aniso_rgba8(vct_ctx* c, uint8_t* out) {
    if (!c || !out) return VCT_ERR_INVALID;
    if (!c->vol.aniso) return vct_fail(c, VCT_ERR_INVALID, "context created without anisotropic_mips");
    HIP_TRY(c, hipSetDevice(c->device));
    const int V = c->cfg.voxel_dim;
    const size_t stride = c->vol.chain_texels - c->vol.nvox();
    for (int d = 0; d < 6; ++d)
        for (int l = 1; l < c->vol.nlev; ++l) {
            const size_t off = d * stride + (size_t)vct_level_offset(V, l) - c->vol.nvox();
            PIPE_TRY(vct_download_level(c, c->vol.aniso.get() + off, V >> l, out + off * 4));
        }
    return VCT_OK;
}

int vct_download_chain_rgba8(vct_ctx* c, uint8_t* chain) {
    if (!c) return VCT_ERR_INVALID;
    if (!chain) return vct_fail(c, VCT_ERR_INVALID, "vct_download_chain_rgba8: null destination");
    HIP_TRY(c, hipSetDevice(c->device));
    for (int l = 0; l < c->vol.nlev; ++l) {
        const size_t off = (size_t)vct_level_offset(c->cfg.voxel_dim, l);
        PIPE_TRY(vct_download_level(c, c->vol.active() + off, c->cfg.voxel_dim >> l, chain + off * 4));
    }
    return VCT_OK;
}

}  // extern "C"
