// vct_api_raster.hip -- the C ABI's raster stages: the shadow map, the G-buffer, and the automatic choice of the main draw's form.
#include "vct_ctx.h"

static size_t shadow_tile_count(int S) { const size_t nb = ((size_t)S + 7) >> 3; return nb * nb; }

// Scratch `r` of one raster pass on stream `s`: `pixels` 64-bit visibility words (main draw) or 32-bit ones (depth_only,
// the shadow-map words).  `dyn` false: a pass over the static mesh.  Otherwise the dynamic mesh's own pass over its draw
// copy (include/vct.h "dynamic mesh", drawing): direct form, its triangle count and records (vct_dynamic_raster_mesh).
static int raster_args(vct_ctx* c, VctRasterScratch& r, int side_w, int side_h, bool depth_only, bool binned, hipStream_t s,
                       VctRasterArgs& a, bool dyn = false) {
    if (!c->mesh.tri_pos) return vct_fail(c, VCT_ERR_INVALID, "no triangles uploaded");
    const size_t pixels = (size_t)side_w * side_h;
    memset(&a, 0, sizeof(a));
    if (dyn) vct_dynamic_raster_mesh(c, a);
    else {
        const VctMesh& sm = c->mesh;
        a.pos = sm.tri_pos.get();
        a.nrm = sm.tri_nrm.get(); a.tan = sm.tri_tan.get(); a.bit = sm.tri_bit.get();
        a.material = sm.tri_mat.get();
        a.albedo = sm.mat_albedo.get();
        a.specular = sm.mat_specular.get();
        a.emission = depth_only ? nullptr : sm.mat_emission.get();
        a.mat_gloss = depth_only ? nullptr : sm.mat_gloss.get();
        a.ntri = sm.ntri;
    }
    const int32_t ntri = a.ntri;      // what sizes the scratch
    if (!depth_only) HIP_TRY(c, r.vis.reserve(pixels, &r.dirty));
    const uint32_t bins = (uint32_t)(((size_t)side_w + 15) / 16 * (((size_t)side_h + 15) / 16));
    if (binned) {
        // Scratch of the tile-binned form (vct_raster.hip).  One 160-byte record per visible sub-triangle (back faces are
        // always culled, a near-clipped triangle is two sub-triangles: ntri + 4096 holds every scene that is not mostly
        // near-clipped) and one 8-byte entry per (sub-triangle, 16x16 bin) overlap -- 3.3 per visible sub-triangle on the
        // Bistro-class street at 4K -- plus the bins' counters.  Whatever does not fit takes the huge list or is
        // rasterised in place (k_bin_setup), so these are sizes, not limits.  ~200 B per triangle and pass kind,
        // replicated per rank of a multi-GPU frame.
        const uint32_t want_recs = (uint32_t)ntri + 4096u;
        const size_t want_ent_sz = (size_t)ntri * 4 + (size_t)bins * 4 + 65536;
        const uint32_t want_ent = (uint32_t)(want_ent_sz < 0x7fffffffull ? want_ent_sz : 0x7fffffffull);
        HIP_TRY(c, r.bin_recs.reserve((size_t)want_recs * 160));
        HIP_TRY(c, r.bin_entries.reserve((size_t)want_ent + 1));      // + the spare entry k_bin_fill's idle lanes write
        // sum over bins of ceil(entries / slice)
        HIP_TRY(c, r.bin_items.reserve(bins + (r.bin_entries.size() - 1) / 512u + 1u));
        HIP_TRY(c, r.bin_count.reserve((size_t)bins * 2 * VCT_BIN_CSTRIDE, &r.dirty));
        HIP_TRY(c, r.bin_huge.reserve((size_t)(VCT_BIN_HUGE_CAP + 16 + 32), &r.dirty));
    } else {
        HIP_TRY(c, r.lists.reserve((size_t)ntri * 4));
        HIP_TRY(c, r.recs.reserve((size_t)ntri * 2 * 96));
        HIP_TRY(c, r.counts.reserve(8, &r.dirty));
        // tile work items: 16x16-pixel pieces of large triangles; pixels/16 entries is ~16x the typical
        // demand (sum of visible bounding boxes ~ a few frames' worth of pixels); overflow is handled
        HIP_TRY(c, r.items.reserve(pixels / 16 + 4096));
    }
    if (r.dirty) {   // first pass, resized buffers, or a pass that failed half way: clear this kind's state once
        if (depth_only) c->shadow.restart_epochs();      // the shadow words restart their epoch cycle with a memset (below)
        else HIP_TRY(c, hipMemsetAsync(r.vis.get(), 0xff, r.vis.size() * sizeof(unsigned long long), s));
        if (binned) {
            HIP_TRY(c, hipMemsetAsync(r.bin_count.get(), 0, r.bin_count.size() * sizeof(uint32_t), s));
            HIP_TRY(c, hipMemsetAsync(r.bin_huge.get() + VCT_BIN_HUGE_CAP, 0, (16 + 32) * sizeof(uint32_t), s));
        } else {
            HIP_TRY(c, hipMemsetAsync(r.counts.get(), 0, 8 * sizeof(uint32_t), s));
        }
        r.dirty = false;
    }
    a.binned = binned ? 1 : 0;
    if (binned) {
        a.bin_recs = r.bin_recs.get(); a.bin_rec_cap = (uint32_t)(r.bin_recs.size() / 160);
        a.bin_entries = r.bin_entries.get(); a.bin_entry_cap = (uint32_t)(r.bin_entries.size() - 1);
        if (c->raster_form.bin_test_caps[0] && c->raster_form.bin_test_caps[0] < a.bin_rec_cap) a.bin_rec_cap = c->raster_form.bin_test_caps[0];
        if (c->raster_form.bin_test_caps[1] && c->raster_form.bin_test_caps[1] < a.bin_entry_cap) a.bin_entry_cap = c->raster_form.bin_test_caps[1];
        a.bin_count = r.bin_count.get(); a.bin_cursor = r.bin_count.get() + r.bin_count.size() / 2;
        a.bin_items = r.bin_items.get(); a.bin_item_cap = (uint32_t)r.bin_items.size();
        a.bin_huge = r.bin_huge.get(); a.bin_huge_cap = VCT_BIN_HUGE_CAP;
        a.bin_ctr = r.bin_huge.get() + VCT_BIN_HUGE_CAP + 8 * r.bin_set;
        a.bin_next_ctr = r.bin_huge.get() + VCT_BIN_HUGE_CAP + 8 * (r.bin_set ^ 1);
        r.bin_set ^= 1;
    }
    a.model_scale = c->cfg.model_scale;
    a.vis = r.vis.get();
    a.vis32 = nullptr;          // vct_render_shadow_map points it at the shadow-map words
    a.vis32_ebase = 0u;
    if (!binned) {
        a.items = r.items.get();
        // [wave, group, item, -]: the wave and group counters are one 8-byte-aligned pair, k_raster_vis reserves both
        // lists of a workgroup with a single 64-bit atomic
        uint32_t* ctr = r.counts.get() + 4 * r.set;
        a.wave_list = r.lists.get();
        a.wave_count = ctr;
        a.group_list = r.lists.get() + (size_t)ntri * 2;
        a.group_count = ctr + 1;
        a.item_count = ctr + 2;
        a.next_counts = r.counts.get() + 4 * (r.set ^ 1);
        a.recs = r.recs.get();
        r.set ^= 1;
        a.item_capacity = (uint32_t)r.items.size();
    }
    if (dyn) return VCT_OK;
    a.tex = vct_textures_of(c);
    if (!depth_only) {          // the main draw's alpha-test class per triangle: once per mesh / texture set
        VctMesh& sm = c->mesh;
        HIP_TRY(c, sm.tri_alpha.reserve((size_t)ntri, &sm.tri_alpha_dirty));
        if (sm.tri_alpha_dirty) {
            HIP_TRY(c, vct_launch_tri_alpha(a, sm.tri_alpha.get(), s));
            sm.tri_alpha_dirty = false;
            c->xslot.note_producer();      // (shared by both frame slots: the other slot's next pass follows this one)
        }
        a.tri_alpha = sm.tri_alpha.get();
    }
    return VCT_OK;
}

// One shadow pass into the map's words under the next epoch (vct_ctx.h VctShadowMap), then the tile bounds.
static int shadow_pass(vct_ctx* c, const float light_vp[16], int S) {
    VctShadowMap& sm = c->shadow;
    VctRasterArgs a, da;
    PIPE_TRY(raster_args(c, sm.raster, S, S, true, c->raster_form.mode == 2, cur(c).stream.get(), a));
    // VCT_DYNAMIC_DRAW_SHADOW: the dynamic mesh's draw copy behind the static mesh, into the same words under the same epoch
    const bool draw_dyn = vct_dynamic_drawn(c, VCT_DYNAMIC_DRAW_SHADOW);
    if (draw_dyn) {      // (a failure here leaves the static scratch's counter sets swapped and unused: cleared by the next pass)
        const int rc = raster_args(c, sm.dyn_raster, S, S, true, false, cur(c).stream.get(), da, true);
        if (rc) { sm.raster.dirty = true; return rc; }
    }
    bool memset_due = false;
    const uint32_t epoch = sm.next_epoch(&memset_due);
    if (memset_due) HIP_TRY(c, hipMemsetAsync(sm.words.get(), 0xff, (size_t)S * S * sizeof(uint32_t), cur(c).stream.get()));
    a.vis32 = sm.words.get();
    a.vis32_ebase = VCT_SHADOW_EPOCH(epoch);
    memcpy(sm.light_vp, light_vp, 64);
    const hipError_t e = vct_launch_shadow_raster(a, light_vp, S, cur(c).stream.get());
    if (e != hipSuccess) { sm.raster.dirty = true; HIP_TRY(c, e); }
    if (draw_dyn) {
        // direct form: atomicMin lowers whatever the static pass left, the plain stores of its binned form included
        da.vis32 = sm.words.get();
        da.vis32_ebase = VCT_SHADOW_EPOCH(epoch);
        const hipError_t ed = vct_launch_shadow_raster(da, light_vp, S, cur(c).stream.get());
        if (ed != hipSuccess) { sm.raster.dirty = sm.dyn_raster.dirty = true; HIP_TRY(c, ed); }
    }
    sm.pass_done(epoch);
    // depth bounds per (dilated) 8 x 8 tile of the new map: the PCF consumers (voxelizer, G-buffer shade) decide most windows on them
    if (sm.tiles) HIP_TRY(c, vct_launch_shadow_minmax(sm.words.get(), sm.ebase, S, sm.tiles.get(), cur(c).stream.get()));
    return VCT_OK;
}

// Automatic choice: six passes -- direct (warm-up: the first pass after an upload pays for cold caches), direct timed,
// binned (warm-up: it also allocates its scratch), binned timed, direct timed, binned timed -- then the form with the
// smaller minimum is kept until the mesh or the textures change.  (Rounds 3-4 compared ONE cold direct pass with one
// warm binned pass: biased towards the binned form -- advisor, round 4.)  Results are identical either way.
static const struct { int form, slot; } kAutoSeq[6] = {{0, -1}, {0, 0}, {1, -1}, {1, 1}, {0, 2}, {1, 3}};

int VctRasterForm::pick(int row0, int row1, bool has_alpha_textures, bool* binned) {
    *binned = mode == 2;
    in_sequence = false;
    if (mode != 0 || !has_alpha_textures) return -1;
    if (state == 6 && choice < 0 && hipEventQuery(ev[7].get()) == hipSuccess) {      // all sampled and finished: the verdict
        float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool ok = true;
        for (int k = 0; k < 4; ++k) ok = ok && hipEventElapsedTime(&t[k], ev[2 * k].get(), ev[2 * k + 1].get()) == hipSuccess;
        if (ok) choice = fminf(t[1], t[3]) < fminf(t[0], t[2]) ? 1 : 0;
    }
    if (choice >= 0) { *binned = choice == 1; return -1; }
    if (state >= 6) { *binned = true; return -1; }      // all sampled, the last event still pending: stay on the last form
    // the samples must cover the same rows (a rank of a multi-GPU frame only ever rasterises its slab, and the
    // slab may move while the load-aware boundaries settle: a sequence over different rows starts again)
    if (state > 0 && (row0 != rows[0] || row1 != rows[1])) state = 0;
    if (row1 <= row0) return -1;
    in_sequence = true;
    *binned = kAutoSeq[state].form == 1;
    rows[0] = row0; rows[1] = row1;
    return kAutoSeq[state].slot;
}

int vct_render_gbuffer_rows_on(vct_ctx* c, const float view_proj[16], int32_t row0, int32_t row1, hipStream_t s, hipEvent_t shadow_ready) {
    if (!view_proj) return vct_fail(c, VCT_ERR_INVALID, "vct_render_gbuffer: null matrix");
    if (!c->mesh.tri_nrm) return vct_fail(c, VCT_ERR_INVALID, "vct_render_gbuffer: call vct_upload_mesh_attributes first");
    if (!vct_rows_in_frame(c, row0, row1)) return vct_fail(c, VCT_ERR_INVALID, "vct_render_gbuffer_rows: tile-row range outside the frame");
    HIP_TRY(c, hipSetDevice(c->device));
    // (two frames in flight: each frame slot has raster scratch of its own, so this pass waits for nothing of the other slot's frame)
    VctRasterForm& form = c->raster_form;
    bool binned = false;
    const int slot = form.pick(row0, row1, c->mesh.has_alpha_textures, &binned);      // >= 0: this pass is timed sample `slot`
    VctRasterArgs a, da;
    VctRasterScratch& r = cur(c).raster;
    VctRasterScratch& dr = cur(c).dyn_raster;
    PIPE_TRY(raster_args(c, r, c->cfg.width, c->cfg.height, false, binned, s, a));
    // VCT_DYNAMIC_DRAW_GBUFFER: the dynamic mesh's draw copy into the slot's second visibility buffer, resolved by the shade kernel
    const bool draw_dyn = vct_dynamic_drawn(c, VCT_DYNAMIC_DRAW_GBUFFER);
    if (draw_dyn) {      // (a failure here leaves the static scratch's counter sets swapped and unused: cleared by the next pass)
        const int rc = raster_args(c, dr, c->cfg.width, c->cfg.height, false, false, s, da, true);
        if (rc) { r.dirty = true; return rc; }
    }
    if (slot >= 0) HIP_TRY(c, hipEventRecord(form.ev[2 * slot].get(), s));
    hipError_t e = vct_launch_gbuffer_visibility(a, view_proj, c->cfg.width, c->cfg.height, row0, row1, s);
    if (slot >= 0 && e == hipSuccess) e = hipEventRecord(form.ev[2 * slot + 1].get(), s);
    if (e == hipSuccess) form.launched();
    // (behind the timed bracket's end event: the automatic form choice measures the static pass alone)
    if (e == hipSuccess && draw_dyn) e = vct_launch_dynamic_visibility(da, view_proj, c->cfg.width, c->cfg.height, row0, row1, s);
    if (e == hipSuccess && shadow_ready) e = hipStreamWaitEvent(s, shadow_ready, 0);
    VctDynShadeArgs ds;
    if (draw_dyn) vct_dynamic_shade_args(c, da, ds);
    // only the dynamic table is attached and this pass does not draw the dynamic mesh: no kernel writes the planes, and
    // the rows may hold an earlier pass's dynamic pixels -- they show the static table's values, which are 0
    if (e == hipSuccess && !draw_dyn && vct_dynamic_emission_attached(c) && !a.emission && cur(c).emis && row1 > row0) {
        const size_t per_row = (size_t)vct_tiles_x(c) * VCT_EMIS_NPLANES * VCT_TILE_PIX;
        e = hipMemsetAsync(cur(c).emis.get() + (size_t)row0 * per_row, 0, (size_t)(row1 - row0) * per_row * sizeof(float), s);
    }
    if (e == hipSuccess)
        e = vct_launch_gbuffer_shade(a, view_proj, c->cfg.width, c->cfg.height, row0, row1, c->shadow.words.get(), c->shadow.ebase,
                                     c->shadow.size, c->shadow.tiles.get(), c->shadow.light_vp, cur(c).gb_tiled.get(), cur(c).emis.get(), cur(c).gloss.get(), s,
                                     draw_dyn ? &ds : nullptr);
    if (e != hipSuccess) { r.dirty = true; if (draw_dyn) dr.dirty = true; HIP_TRY(c, e); }
    cur(c).gb_current = cur(c).gb_tiled.get();
    form.last_form = binned ? 2 : 1;
    cur(c).last_row0 = row0;
    cur(c).last_row1 = row1;
    cur(c).last_row_stride = 1;
    cur(c).have_gbuffer = true;
#if defined(VCT_BIN_STATS) && VCT_BIN_STATS
    if (binned && getenv("VCT_BIN_STATS_DUMP")) {       // instrumented builds only (tools/r04_binstats.sh)
        uint32_t st[48];
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, hipMemcpy(st, r.bin_huge.get() + VCT_BIN_HUGE_CAP, sizeof(st), hipMemcpyDeviceToHost));
        const uint32_t* ctr = st + 8 * (r.bin_set ^ 1);
        fprintf(stderr, "binstats: entries %u records %u items %u huge %u | ", ctr[0], ctr[1], ctr[2], ctr[4]);
        // (the adopted form of k_bin_raster only counts its alpha-queue flushes and the fragments they fetched; the
        // per-step counters of the earlier forms are in profiles/experiments/README.md)
        fprintf(stderr, "alpha_queue_flushes %u fragments_fetched %u\n", st[16 + 7], st[16 + 8]);
        HIP_TRY(c, hipMemset(r.bin_huge.get() + VCT_BIN_HUGE_CAP + 16, 0, 32 * sizeof(uint32_t)));
    }
#endif
    return VCT_OK;
}

extern "C" {

int vct_upload_shadow_map(vct_ctx* c, const float* depth, int32_t size, const float light_vp[16]) {
    if (!c) return VCT_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_drain(c));
    c->shadow.drop();
    if (!depth) return VCT_OK;
    if (size <= 0 || !light_vp) return vct_fail(c, VCT_ERR_INVALID, "vct_upload_shadow_map: bad size");
    // the map lives as shadow-map words (vct_internal.h): depths clamped to [0, 1] like a GL depth texture, epoch 0;
    // a later vct_render_shadow_map starts a fresh epoch cycle over this buffer (shadow_passes = 0: memset first).
    // Built in locals: a failure leaves the context without a map.
    const size_t n = (size_t)size * size;
    VctBuf<uint32_t> words;
    VctBuf<float> tmp;
    VctBuf<uint2> tiles;
    HIP_TRY(c, words.alloc(n));
    HIP_TRY(c, tmp.alloc(n));
    HIP_TRY(c, hipMemcpyAsync(tmp.get(), depth, n * sizeof(float), hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, vct_launch_shadow_encode(tmp.get(), words.get(), n, 0u, cur(c).stream.get()));
    HIP_TRY(c, tiles.alloc(shadow_tile_count(size)));
    HIP_TRY(c, vct_launch_shadow_minmax(words.get(), 0u, size, tiles.get(), cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    c->shadow.words = std::move(words);
    c->shadow.tiles = std::move(tiles);
    c->shadow.size = size;
    c->shadow.ebase = 0u;
    c->shadow.restart_epochs();
    memcpy(c->shadow.light_vp, light_vp, 64);
    return VCT_OK;
}

int vct_render_shadow_map(vct_ctx* c, const float light_vp[16]) {
    if (!c) return VCT_ERR_INVALID;
    if (!light_vp) return vct_fail(c, VCT_ERR_INVALID, "vct_render_shadow_map: null matrix");
    const int S = c->cfg.shadow_map_size;
    if (S <= 0) return vct_fail(c, VCT_ERR_INVALID, "vct_render_shadow_map: config.shadow_map_size <= 0");
    HIP_TRY(c, hipSetDevice(c->device));
    VctShadowMap& sm = c->shadow;
    if (sm.words && sm.size == S) PIPE_TRY(vct_pipeline_join(c)); else PIPE_TRY(vct_pipeline_drain(c));   // (re)allocation: host wait
    if (sm.words && sm.size != S) sm.drop();
    if (!sm.words) {
        HIP_TRY(c, sm.words.alloc((size_t)S * S));
        sm.restart_epochs();
    }
    // Tile bounds of the map (vct_launch_shadow_minmax) cost one more pass over it (~0.03 ms at 4096^2) and save the PCF
    // consumers their window fetches away from shadow boundaries: 14-28 % of the voxelize pass (street: 0.536 -> 0.461 ms at
    // 1024^3, 0.176 -> 0.126 at 256^3; atrium 0.033 -> 0.031).  Built where that repays the pass: meshes of >= 4 M
    // voxel fragments (VCT_SHADOW_TILES=0 / 1 in the environment: never / always).  Results are identical either way.
    bool want_tiles = c->vox.n_frags >= 4000000u;
    if (const char* st = getenv("VCT_SHADOW_TILES")) want_tiles = st[0] == '1';
    if (want_tiles && !sm.tiles) HIP_TRY(c, sm.tiles.alloc(shadow_tile_count(S)));
    if (!want_tiles) sm.tiles.reset();
    sm.size = S;
    return sm.pass_result(shadow_pass(c, light_vp, S));      // (a pass that fails from here on leaves no tile bounds)
}

int vct_download_shadow_map(vct_ctx* c, float* depth) {
    if (!c || !depth) return VCT_ERR_INVALID;
    if (!c->shadow.words) return vct_fail(c, VCT_ERR_INVALID, "no shadow map");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->shadow.size * c->shadow.size;
    VctBuf<float> tmp;
    HIP_TRY(c, tmp.alloc(n));
    HIP_TRY(c, vct_launch_shadow_decode(c->shadow.words.get(), tmp.get(), n, c->shadow.ebase, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(depth, tmp.get(), n * sizeof(float), hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

int vct_render_gbuffer_rows(vct_ctx* c, const float view_proj[16], int32_t row0, int32_t row1) {
    if (!c) return VCT_ERR_INVALID;
    return vct_render_gbuffer_rows_on(c, view_proj, row0, row1, cur(c).stream.get());
}

int vct_render_gbuffer(vct_ctx* c, const float view_proj[16]) {
    if (!c) return VCT_ERR_INVALID;
    return vct_render_gbuffer_rows(c, view_proj, 0, vct_tiles_y(c));
}

int vct_download_gbuffer(vct_ctx* c, float* planes) {
    if (!c || !planes) return VCT_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    return vct_planes_download(c, cur(c).gb_current, planes, VCT_GB_NPLANES, sizeof(float));
}

}  // extern "C"
