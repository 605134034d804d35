// vct_api_scene.hip -- the C ABI's scene uploads: triangles (with their voxelization plan), mesh attributes, uvs, textures.
#include <algorithm>

#include "vct_ctx.h"

VctTextures vct_textures_of(const vct_ctx* c) {
    VctTextures t;
    memset(&t, 0, sizeof(t));
    const VctMesh& m = c->mesh;
    if (m.tex_texels && m.tri_uv && m.mat_tex) {
        t.texels = m.tex_texels.get(); t.desc = m.tex_desc.get(); t.mat_tex = m.mat_tex.get(); t.uv = m.tri_uv.get(); t.ntex = m.ntex;
        t.mips = c->cfg.texture_mipmaps ? 1 : 0;
    }
    return t;
}

namespace {

// Per-mesh brick slots.  The bricks a fragment of this mesh can land in depend only on geometry, V and G (not on the
// light, the shadow map or the textures), so they are found ONCE per upload -- from the conservative voxelizer's
// fragment list `frags` and a mark-only run of the reference-mode voxelizer -- and every marked brick gets a slot; the
// fragment list is then sorted by slot (counting sort) and the staging pool of the north-star pass is allocated (+ the
// voxel attributes when config.voxel_attributes).  Everything is built in a local plan that becomes the context's as the
// last statement, so a failure on the way leaves the context with the empty plan vct_upload_triangles gave it
// (vct_voxelize then reports it) instead of a half-initialised one.
int build_voxel_slots(vct_ctx* c, const uint2* frags, uint32_t nfrags) {
    const uint32_t nbricks = (uint32_t)c->vol.nbricks();
    const int32_t ntri = c->mesh.ntri;
    VctVoxelPlan v;
    VctBuf<uint32_t> mark, count, cnt, cursor;
    VctVoxParams p = vct_vox_params(c, v);       // the mesh alone: the mark-only run reads nothing of a plan
    HIP_TRY(c, mark.alloc(nbricks));
    HIP_TRY(c, v.brick_slot.alloc(nbricks));
    HIP_TRY(c, count.alloc(1));
    HIP_TRY(c, hipMemsetAsync(mark.get(), 0, (size_t)nbricks * sizeof(uint32_t), cur(c).stream.get()));
    HIP_TRY(c, v.ref_big.alloc((size_t)ntri + 1));
    HIP_TRY(c, vct_launch_frag_mark(frags, nfrags, mark.get(), cur(c).stream.get()));                  // north-star mode's fragments
    p.mark_only = 1;
    p.brick_mark = mark.get();
    p.shadow = nullptr;
    vct_glm_voxel_projections(c, p.proj);
    HIP_TRY(c, vct_launch_voxelize_reference(p, v.ref_big.get() + 1, v.ref_big.get(), cur(c).stream.get()));   // reference mode's (mark only)
    HIP_TRY(c, vct_launch_assign_slots(mark.get(), v.brick_slot.get(), count.get(), nbricks, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(&v.nslots, count.get(), sizeof(v.nslots), hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    // counting sort of the fragments by slot: per-slot counts -> offsets (host prefix sum: once per mesh) -> scatter
    const size_t ns = v.nslots ? v.nslots : 1u;
    HIP_TRY(c, cnt.alloc(ns));
    HIP_TRY(c, cursor.alloc(ns));
    HIP_TRY(c, v.slot_first.alloc(ns + 1));
    HIP_TRY(c, v.slot_brick.alloc(ns));
    HIP_TRY(c, v.frag_sorted.alloc(nfrags ? nfrags : 1u));
    v.n_frags = nfrags;
    HIP_TRY(c, hipMemsetAsync(cnt.get(), 0, ns * sizeof(uint32_t), cur(c).stream.get()));
    HIP_TRY(c, hipMemsetAsync(cursor.get(), 0, ns * sizeof(uint32_t), cur(c).stream.get()));
    HIP_TRY(c, hipMemsetAsync(v.slot_brick.get(), 0, ns * sizeof(uint32_t), cur(c).stream.get()));
    HIP_TRY(c, vct_launch_slot_bricks(v.brick_slot.get(), nbricks, v.slot_brick.get(), cur(c).stream.get()));      // every slot names its brick
    HIP_TRY(c, vct_launch_frag_count(frags, nfrags, v.brick_slot.get(), cnt.get(), cur(c).stream.get()));
    std::vector<uint32_t> hcnt(ns, 0u), hfirst(ns + 1, 0u);
    HIP_TRY(c, hipMemcpyAsync(hcnt.data(), cnt.get(), ns * sizeof(uint32_t), hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    for (size_t i = 0; i < ns; ++i) hfirst[i + 1] = hfirst[i] + hcnt[i];
    HIP_TRY(c, hipMemcpyAsync(v.slot_first.get(), hfirst.data(), (ns + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, vct_launch_frag_scatter(frags, nfrags, v.brick_slot.get(), v.slot_first.get(), cursor.get(), v.frag_sorted.get(),
                                       v.slot_brick.get(), cur(c).stream.get()));
    // the barycentrics of every fragment (geometry only): the pass reads them instead of re-deriving the triangle set-up
    HIP_TRY(c, v.frag_bary.alloc(nfrags ? nfrags : 1u));
    {
        const VctVoxParams q = vct_vox_params(c, v);      // the sorted fragments and their slots
        HIP_TRY(c, vct_launch_frag_geom(q, v.frag_bary.get(), nullptr, cur(c).stream.get()));
        if (c->cfg.voxel_attributes) {
            HIP_TRY(c, v.tri_qnrm.alloc((size_t)(ntri > 0 ? ntri : 1) * 3));
            HIP_TRY(c, vct_launch_tri_nrm(q, v.tri_qnrm.get(), cur(c).stream.get()));
        }
    }
    // Work items of the pass, the heaviest slots first, slots above VCT_VOX_CHUNK fragments cut into chunks.  Fragments
    // per slot are uneven (atrium at 256^3: 425 on average, 1,918 at most; the street at 256^3: 4,138 and 23,128): with
    // one workgroup per slot in slot order the pass ended when an unluckily late heavy slot did.  Longest-first alone:
    // atrium 0.068 -> 0.049 ms, street at 1024^3 1.41 -> 1.27 ms; cutting the few very heavy slots as well: street at
    // 256^3 0.64 -> 0.31 ms.  (Smaller chunks cost more in accumulator atomics than they balance: 1024: 1.43 ms.)
    std::vector<uint32_t> order(ns);
    for (size_t i = 0; i < ns; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hcnt[a] > hcnt[b]; });
    std::vector<uint32_t> hitems;
    hitems.reserve(ns * 4 + 64);
    std::vector<uint32_t> hmulti;
    const uint32_t CH = v.chunk;
    if (v.nslots)
        for (uint32_t sl : order) {
            const uint32_t chunks = hcnt[sl] ? (hcnt[sl] + CH - 1u) / CH : 1u;
            const uint32_t mi = chunks > 1u ? v.n_multi++ : 0xffffffffu;
            if (chunks > 1u) hmulti.push_back(sl);
            for (uint32_t ch = 0; ch < chunks; ++ch) {      // (slot, first fragment, fragments, multi index or ~0)
                const uint32_t nfr = hcnt[sl] - ch * CH < CH ? hcnt[sl] - ch * CH : CH;
                hitems.push_back(sl); hitems.push_back(hfirst[sl] + ch * CH); hitems.push_back(nfr); hitems.push_back(mi);
            }
        }
    v.n_items = (uint32_t)(hitems.size() / 4);
    HIP_TRY(c, v.items.alloc(v.n_items ? v.n_items : 1u));
    if (v.n_items) HIP_TRY(c, hipMemcpyAsync(v.items.get(), hitems.data(), (size_t)v.n_items * 16, hipMemcpyHostToDevice, cur(c).stream.get()));
    const size_t nm = v.n_multi ? v.n_multi : 1u;
    HIP_TRY(c, v.acc2.alloc(nm * 512 * 2));
    HIP_TRY(c, hipMemsetAsync(v.acc2.get(), 0, nm * 512 * 2 * sizeof(unsigned long long), cur(c).stream.get()));
    HIP_TRY(c, v.multi_slot.alloc(nm));
    if (v.n_multi) HIP_TRY(c, hipMemcpyAsync(v.multi_slot.get(), hmulti.data(), (size_t)v.n_multi * sizeof(uint32_t), hipMemcpyHostToDevice, cur(c).stream.get()));
    if (c->cfg.voxel_attributes) {
        HIP_TRY(c, v.acc2_attr.alloc(nm * 512 * 3));
        HIP_TRY(c, hipMemsetAsync(v.acc2_attr.get(), 0, nm * 512 * 3 * sizeof(unsigned long long), cur(c).stream.get()));
    }
    // staging pool of a pass (+ attributes): written in full by every pass, never cleared
    const size_t pool_vox = ns * 512;
    HIP_TRY(c, v.stage.alloc(pool_vox));
    HIP_TRY(c, hipMemsetAsync(v.stage.get(), 0, pool_vox * 4, cur(c).stream.get()));
    if (c->cfg.voxel_attributes) {
        VctBuf<uint32_t>* pools[] = {&v.stage_albedo, &v.stage_normal, &v.attr_albedo, &v.attr_normal};
        for (VctBuf<uint32_t>* b : pools) HIP_TRY(c, b->alloc(pool_vox));
        for (VctBuf<uint32_t>* b : pools) HIP_TRY(c, hipMemsetAsync(b->get(), 0, pool_vox * 4, cur(c).stream.get()));
    }
    // (these describe the chain, not the mesh: allocated with the first plan, kept from then on)
    const size_t flag_bytes = (size_t)nbricks * sizeof(uint32_t);
    VctBuf<uint32_t>* flags[] = {&c->vol.brick_flags, &c->vol.brick_prev, &c->vol.mip_seen};
    for (VctBuf<uint32_t>* f : flags)
        if (!*f) {
            HIP_TRY(c, f->alloc(nbricks));
            HIP_TRY(c, hipMemsetAsync(f->get(), 0, flag_bytes, cur(c).stream.get()));
        }
    HIP_TRY(c, hipMemsetAsync(c->vol.brick_flags.get(), 0, flag_bytes, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    c->vox = std::move(v);
    c->vol.touched();      // fresh (zeroed) attribute pools and slots: a voxel view of the attributes rebuilds its occupancy
    return VCT_OK;
}

}  // namespace

extern "C" {

int vct_upload_triangles(vct_ctx* c, const float* pos, const int32_t* material, int32_t ntri,
                         const float* albedo, int32_t nmat) {
    if (!c) return VCT_ERR_INVALID;
    if (!pos || !material || !albedo || ntri <= 0 || nmat <= 0)
        return vct_fail(c, VCT_ERR_INVALID, "vct_upload_triangles: null or empty input");
    for (int32_t i = 0; i < ntri; ++i)
        if (material[i] < 0 || material[i] >= nmat)
            return vct_fail(c, VCT_ERR_INVALID, "vct_upload_triangles: material index out of range");
    // The vertex contract of include/vct.h, checked before anything of the current mesh is touched: a refused mesh
    // leaves the context as it was.  The product is formed in fp32, as every kernel forms it; !(x <= lim) is also
    // true for NaN and the infinities.
    {
        const float ms = c->cfg.model_scale, lim = vct_vertex_limit(c);
        const size_t nfloat = (size_t)ntri * 9;
        for (size_t i = 0; i < nfloat; ++i)
            if (!(fabsf(pos[i] * ms) <= lim)) {
                char msg[256];
                snprintf(msg, sizeof msg, "vct_upload_triangles: vertex %zu of triangle %zu (%g, times model_scale %g) is not "
                         "finite or beyond 2^20 grid widths (%g): outside the vertex contract of vct.h",
                         (i / 3) % 3, i / 9, (double)pos[i], (double)ms, (double)lim);
                return vct_fail(c, VCT_ERR_INVALID, msg);
            }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_drain(c));
    VctMesh& m = c->mesh;
    m.tri_pos.reset(); m.tri_mat.reset(); m.tri_alpha.reset(); m.mat_albedo.reset();
    m.tri_alpha_dirty = true;
    c->shadow.raster.release_mesh();
    for (VctFrameSlot& sl : c->slots) sl.raster.release_mesh();
    c->raster_form.restart();       // the raster form is measured again for the new mesh
    // Everything indexed by the OLD mesh's triangles or slots goes BEFORE anything below can fail, so that a failed upload
    // leaves the context without a plan (vct_voxelize then refuses) instead of with the old mesh's plan over the new
    // mesh's triangles.  Level 0 / brick_prev keep describing what the chain shows.
    c->vox = VctVoxelPlan();
    vct_emission_detach(c);         // the table is indexed by the old materials, the pool by the old slots
    vct_material_gloss_detach(c);   // the class map too
    c->vol.touched();
    m.tri_nrm.reset(); m.tri_tan.reset(); m.tri_bit.reset(); m.tri_uv.reset();       // belong to the old mesh
    m.mat_tex.reset();                                                                // indexed by the old materials
    if (ntri >= (1 << 23))
        return vct_fail(c, VCT_ERR_INVALID, "vct_upload_triangles: more than 2^23 - 1 triangles (the voxelizer's fragment "
                                        "entries carry 23 bits of triangle index)");
    HIP_TRY(c, m.tri_pos.alloc((size_t)ntri * 9));
    HIP_TRY(c, m.tri_mat.alloc((size_t)ntri));
    HIP_TRY(c, m.mat_albedo.alloc((size_t)nmat * 4));
    HIP_TRY(c, c->plan.reserve(4));
    HIP_TRY(c, hipMemcpyAsync(m.tri_pos.get(), pos, (size_t)ntri * 9 * sizeof(float), hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(m.tri_mat.get(), material, (size_t)ntri * sizeof(int32_t), hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(m.mat_albedo.get(), albedo, (size_t)nmat * 4 * sizeof(float), hipMemcpyHostToDevice, cur(c).stream.get()));
    m.ntri = ntri;
    m.nmat = nmat;
    // Voxelization plan (geometry only): the exact conservative fragments of every triangle -- count, allocate, fill;
    // triangles with a huge bounding box are enumerated by a workgroup each -- then sorted by brick (build_voxel_slots).
    const VctVoxParams p = vct_vox_params(c, c->vox);
    uint32_t counts[4] = {0, 0, 0, 0};
    uint32_t* plan = c->plan.get();
    VctBuf<int32_t> big_tmp;
    VctBuf<uint2> frags;
    HIP_TRY(c, big_tmp.alloc((size_t)ntri));
    HIP_TRY(c, hipMemsetAsync(plan, 0, 4 * sizeof(uint32_t), cur(c).stream.get()));
    HIP_TRY(c, vct_launch_vox_plan(p, plan, nullptr, big_tmp.get(), false, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(counts, plan, sizeof(counts), hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    const uint32_t n_small = counts[0];
    const int n_big = (int)counts[1];
    HIP_TRY(c, vct_launch_vox_plan_big(p, big_tmp.get(), n_big, plan, nullptr, false, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(counts, plan, sizeof(counts), hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    const unsigned long long total = (unsigned long long)n_small + counts[2];
    // counts[3]: one of the 32-bit device counters wrapped while counting (k_vox_plan / k_vox_plan_big flag it) -- the
    // totals above would then look small
    if (total >= (1ull << 32) || counts[3] != 0u)
        return vct_fail(c, VCT_ERR_INVALID, "vct_upload_triangles: the mesh has 2^32 or more conservative fragments at this grid size");
    HIP_TRY(c, frags.alloc((size_t)(total ? total : 1ull)));
    const uint32_t restart[4] = {0u, 0u, n_small, 0u};          // small triangles fill [0, n_small), the big ones behind
    HIP_TRY(c, hipMemcpyAsync(plan, restart, sizeof(restart), hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, vct_launch_vox_plan(p, plan, frags.get(), nullptr, true, cur(c).stream.get()));
    HIP_TRY(c, vct_launch_vox_plan_big(p, big_tmp.get(), n_big, plan, frags.get(), true, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    big_tmp.reset();
    return build_voxel_slots(c, frags.get(), (uint32_t)total);
}

int vct_upload_mesh_attributes(vct_ctx* c, const float* normal, const float* tangent,
                               const float* bitangent, const float* specular) {
    if (!c) return VCT_ERR_INVALID;
    if (!normal || !tangent || !bitangent || !specular) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_mesh_attributes: null input");
    if (!c->mesh.tri_pos) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_mesh_attributes: call vct_upload_triangles first");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_drain(c));
    VctBuf<float>* dst[3] = {&c->mesh.tri_nrm, &c->mesh.tri_tan, &c->mesh.tri_bit};
    const float* src[3] = {normal, tangent, bitangent};
    const size_t n = (size_t)c->mesh.ntri * 9;
    for (int k = 0; k < 3; ++k) {
        HIP_TRY(c, dst[k]->alloc(n));
        HIP_TRY(c, hipMemcpyAsync(dst[k]->get(), src[k], n * sizeof(float), hipMemcpyHostToDevice, cur(c).stream.get()));
    }
    HIP_TRY(c, c->mesh.mat_specular.alloc((size_t)c->mesh.nmat * 3));
    HIP_TRY(c, hipMemcpyAsync(c->mesh.mat_specular.get(), specular, (size_t)c->mesh.nmat * 3 * sizeof(float),
                              hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

int vct_upload_mesh_uvs(vct_ctx* c, const float* uv) {
    if (!c) return VCT_ERR_INVALID;
    if (!uv) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_mesh_uvs: null input");
    if (!c->mesh.tri_pos) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_mesh_uvs: call vct_upload_triangles first");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_drain(c));
    const size_t n = (size_t)c->mesh.ntri * 6;
    c->mesh.tri_alpha_dirty = true;          // textures take effect once the coordinates are there
    c->vox.frag_alb_dirty = true;
    HIP_TRY(c, c->mesh.tri_uv.alloc(n));
    HIP_TRY(c, hipMemcpyAsync(c->mesh.tri_uv.get(), uv, n * sizeof(float), hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

int vct_upload_textures(vct_ctx* c, const uint8_t* const* rgba8, const int32_t* width, const int32_t* height,
                        int32_t ntex, const int32_t* mat_tex) {
    if (!c) return VCT_ERR_INVALID;
    if (!c->mesh.tri_pos) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_textures: call vct_upload_triangles first");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_drain(c));
    VctMesh& m = c->mesh;
    m.tex_texels.reset(); m.tex_desc.reset(); m.mat_tex.reset();
    m.ntex = 0;
    m.tri_alpha_dirty = true;
    c->vox.frag_alb_dirty = true;
    m.has_alpha_textures = false;
    c->raster_form.restart();
    if (ntex == 0) return VCT_OK;                     // detach: flat colours again
    if (ntex < 0 || !rgba8 || !width || !height || !mat_tex)
        return vct_fail(c, VCT_ERR_INVALID, "vct_upload_textures: null or negative input");
    // Packed buffer: every texture's level 0, followed (config.texture_mipmaps) by its mip chain down to 1 x 1 --
    // glGenerateMipmap (R/Model.h:168), built here on the GPU level by level (k_tex_mip).
    std::vector<VctTexDesc> desc((size_t)ntex);
    size_t total = 0;
    for (int32_t i = 0; i < ntex; ++i) {
        if (!rgba8[i] || width[i] <= 0 || height[i] <= 0 || width[i] > 16384 || height[i] > 16384)
            return vct_fail(c, VCT_ERR_INVALID, "vct_upload_textures: bad texture size");
        VctTexDesc& d = desc[(size_t)i];
        memset(&d, 0, sizeof(d));
        d.off = (uint32_t)total;
        d.w = width[i];
        d.h = height[i];
        const size_t n = (size_t)width[i] * height[i];
        uint32_t flags = 0;
        for (size_t k = 0; k < n; ++k)
            if (rgba8[i][4 * k + 3] != 255) { flags = 1u; break; }
        // bit 1: a square power-of-two map -- its level offsets have a closed form (vct_tex_level_offset), which saves the
        // samplers the dependent load of lvl[k]
        if (width[i] == height[i] && (width[i] & (width[i] - 1)) == 0) flags |= 2u;
        d.flags = flags;
        d.nlev = 1;
        if (c->cfg.texture_mipmaps)
            for (int side = width[i] > height[i] ? width[i] : height[i]; side > 1; side >>= 1) ++d.nlev;
        size_t off = 0;
        for (int k = 0; k < d.nlev; ++k) {
            d.lvl[k] = (uint32_t)off;
            off += (size_t)(width[i] >> k > 1 ? width[i] >> k : 1) * (size_t)(height[i] >> k > 1 ? height[i] >> k : 1);
        }
        total += off;
        if (total > 0xffffffffull) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_textures: more than 2^32 texels");
    }
    for (int32_t k = 0; k < m.nmat * 3; ++k)
        if (mat_tex[k] >= ntex) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_textures: texture index out of range");
    HIP_TRY(c, m.tex_texels.alloc(total));
    HIP_TRY(c, m.tex_desc.alloc((size_t)ntex));
    HIP_TRY(c, m.mat_tex.alloc((size_t)m.nmat * 3));
    uint32_t* texels = m.tex_texels.get();
    for (int32_t i = 0; i < ntex; ++i) {
        const VctTexDesc& d = desc[(size_t)i];
        HIP_TRY(c, hipMemcpyAsync(texels + d.off, rgba8[i], (size_t)width[i] * height[i] * 4, hipMemcpyHostToDevice, cur(c).stream.get()));
        for (int k = 1; k < d.nlev; ++k) {
            const int pw = d.w >> (k - 1) > 1 ? d.w >> (k - 1) : 1, ph = d.h >> (k - 1) > 1 ? d.h >> (k - 1) : 1;
            const int w = d.w >> k > 1 ? d.w >> k : 1, h = d.h >> k > 1 ? d.h >> k : 1;
            HIP_TRY(c, vct_launch_tex_mip(texels + d.off + d.lvl[k - 1], pw, ph, texels + d.off + d.lvl[k], w, h, cur(c).stream.get()));
        }
    }
    HIP_TRY(c, hipMemcpyAsync(m.tex_desc.get(), desc.data(), (size_t)ntex * sizeof(VctTexDesc), hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(m.mat_tex.get(), mat_tex, (size_t)m.nmat * 3 * sizeof(int32_t), hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    m.ntex = ntex;
    for (int32_t k = 0; k < m.nmat; ++k)               // a diffuse map with non-opaque texels: its fragments are alpha-tested
        if (mat_tex[3 * k] >= 0 && (desc[(size_t)mat_tex[3 * k]].flags & 1u)) m.has_alpha_textures = true;
    return VCT_OK;
}

}  // extern "C"
