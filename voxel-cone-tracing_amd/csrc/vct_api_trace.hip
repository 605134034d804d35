// vct_api_trace.hip -- the C ABI's cone trace: step tables, march parameters, every vct_trace* entry point, vct_gi_pass, outputs, counts, self-tests.
#include <stddef.h>

#include <algorithm>
#include <map>
#include <mutex>

#include "vct_ctx.h"
#include "vct_divisors.h"

// The step sequence of trace.fs:90-104, evaluated with the reference's operation order:
//   dist = vs; while (dist < MAX) { diameter = max(vs, 2*t*dist); lod = log2(diameter/vs); ...
//   dist += diameter; }   and the [GL] textureLod level selection for that lod.
int vct_build_steps(const vct_config& cfg, float tan_half, std::vector<VctStep>& out) {
    out.clear();
    const int maxl = vct_ilog2(cfg.voxel_dim);
    const float vs = cfg.grid_world_size / (float)cfg.voxel_dim;
    float dist = vs;
    while (dist < cfg.max_distance) {
        if ((int)out.size() >= VCT_MAX_STEPS) return -1;
        VctStep s;
        const float diameter = fmaxf(vs, 2.0f * tan_half * dist);
        const float lod = log2f(diameter / vs);
        s.dist = dist;
        s.occ_den = 1.0f + 0.03f * diameter;
        s.occ_rcp = 1.0f / s.occ_den;
        float lam = lod;
        if (!(lam > 0.0f)) {
            s.two_levels = 0; s.level = 0; s.level2 = 0; s.frac = 0.0f;
        } else {
            if (lam > (float)maxl) lam = (float)maxl;
            const float fl = floorf(lam);
            s.two_levels = 1;
            s.level = (int)fl;
            s.level2 = s.level + 1 > maxl ? maxl : s.level + 1;
            s.frac = lam - fl;
        }
        // frac == 0: the blend is fma(0, tri(level2), 1*tri(level)) = tri(level) exactly (texels are
        // finite and >= +0), so the second level need not be sampled.
        if (s.two_levels && s.frac == 0.0f) s.two_levels = 0;
        s.omf = 1.0f - s.frac;
        auto ref = [&](int level) {
            VctLevelRef r;
            const int lg = maxl - level;
            r.off = (uint32_t)vct_level_offset(cfg.voxel_dim, level);
            r.mask_x = 0x09249249u & (uint32_t)((1ull << (3 * lg)) - 1ull);
            r.fN = (float)(1 << lg);
            r.m = (1 << lg) - 1;
            return r;
        };
        s.l1 = ref(s.level);
        s.l2 = ref(s.level2);
        out.push_back(s);
        const float nd = dist + diameter;
        if (!(nd > dist)) return -1;   // would never terminate
        dist = nd;
    }
    return 0;
}

namespace {

// The result words of a self-test kernel (pairs of mismatches, one example), through the statistics words as scratch
// (never the step-counter bank: vct_last_step_count sums that).
template <size_t N, class Launch>
int selftest_words(vct_ctx* c, unsigned long long (&v)[N], Launch launch) {
    static_assert(N <= 32, "the statistics words");
    HIP_TRY(c, hipMemsetAsync(c->stats.get(), 0, N * sizeof(unsigned long long), cur(c).stream.get()));
    HIP_TRY(c, launch(c->stats.get(), cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(v, c->stats.get(), N * sizeof(unsigned long long), hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

// The kernel divides by wave-uniform constants (half_G, the per-step occlusion denominators) with
// q = fma(x, r_hi, x * r_lo), r_hi + r_lo = 1/d to 48 bits (vct_trace.hip div_const) -- exact only for some divisors, so every divisor of
// a step table is first verified on the device against the IEEE divide over all fp32 inputs
// (divisors_verified below); structural preconditions: significand not all ones, d and 1/d normal.
// Anything else switches the kernel to the IEEE-divide instantiation.
bool divisor_ok(float d) {
    uint32_t b;
    memcpy(&b, &d, 4);
    const uint32_t e = (b >> 23) & 0xffu, m = b & 0x7fffffu;
    if (!(d > 0.0f) || e == 0xffu) return false;
    return m != 0x7fffffu && e >= 4 && e <= 250;   // d and 1/d both far from the subnormal range
}

// Is the kernel's constant division exact for divisor d (vct_trace.hip div_const<1>)?  The divisors of the BASELINE
// grids and apertures ship as a table (vct_divisors.h: verified on the device, and every entry re-verified by
// tests/test_gpu_parity.py::test_const_divide_exhaustive), so a fresh process pays nothing for them; any other
// divisor is checked exhaustively on the device the first time a step table uses it (k_divide_selftest, 2 ms per
// divisor, synchronous -- an aperture animated per frame pays it once per new divisor) and the verdict is cached for
// the life of the process.  The cache is shared by every context of the process (one host thread per context, so
// two GPUs' threads may race here): guarded by a mutex.
int divisor_verified(vct_ctx* c, float d, bool* ok) {
    static std::map<uint32_t, bool> cache;
    static std::mutex cache_lock;
    uint32_t bits;
    memcpy(&bits, &d, 4);
    const uint32_t* end = kVerifiedDivisors + sizeof(kVerifiedDivisors) / sizeof(kVerifiedDivisors[0]);
    if (std::binary_search(kVerifiedDivisors, end, bits)) { *ok = true; return VCT_OK; }
    {
        std::lock_guard<std::mutex> g(cache_lock);
        auto it = cache.find(bits);
        if (it != cache.end()) { *ok = it->second; return VCT_OK; }
    }
    unsigned long long v[2] = {1, 0};
    PIPE_TRY(selftest_words(c, v, [&](unsigned long long* w, hipStream_t st) { return vct_launch_divide_selftest(d, w, st); }));
    *ok = v[0] == 0ull;
    std::lock_guard<std::mutex> g(cache_lock);
    cache[bits] = *ok;
    return VCT_OK;
}

}  // namespace

int vct_refresh_steps(vct_ctx* c) {
    if (!c->steps_dirty) return VCT_OK;
    PIPE_TRY(vct_pipeline_drain(c));      // the other slot's trace may still read the table that is rewritten below
    std::vector<VctStep> d, s;
    if (vct_build_steps(c->cfg, c->cfg.tan_diffuse, d) || vct_build_steps(c->cfg, c->cfg.tan_specular, s))
        return vct_fail(c, VCT_ERR_INVALID, "cone aperture needs more than VCT_MAX_STEPS march steps");
    // the tables of the gloss classes (include/vct.h "per-material gloss"): built like `s`, under the same verdict
    std::vector<VctStep> g[VCT_GLOSS_CLASSES_MAX];
    for (int k = 0; k < c->gloss.n; ++k)
        if (vct_build_steps(c->cfg, c->gloss.cls[k].tan_specular, g[k]))      // (vct_set_gloss_classes built it once already)
            return vct_fail(c, VCT_ERR_INVALID, "a gloss class's aperture needs more than VCT_MAX_STEPS march steps");
    c->n_diffuse = (int)d.size();
    c->n_specular = (int)s.size();
    // preconditions of the kernel's FMA division (vct_trace.hip div_const): admissible divisors, and
    // occlusion numerators bounded away from the underflow range (blend factors 0 or >= 2^-10,
    // 1 - alpha >= 2^-5 while a cone is live)
    bool ok = divisor_ok(c->cfg.grid_world_size * 0.5f) && (1.0f - c->cfg.max_alpha) >= 0x1p-5f;
    auto blend_ok = [](const VctStep& st) {
        if (!st.two_levels) return true;
        return st.frac >= 0x1p-10f && (1.0f - st.frac) >= 0x1p-10f;
    };
    for (const VctStep& st : d) ok = ok && divisor_ok(st.occ_den) && blend_ok(st);
    for (const VctStep& st : s) ok = ok && divisor_ok(st.occ_den) && blend_ok(st);
    for (int k = 0; k < c->gloss.n; ++k)
        for (const VctStep& st : g[k]) ok = ok && divisor_ok(st.occ_den) && blend_ok(st);
    if (ok) {      // every divisor of the tables passes the device's exhaustive check of the kernel's division
        std::vector<float> divs = {c->cfg.grid_world_size * 0.5f};
        for (const VctStep& st : d) divs.push_back(st.occ_den);
        for (const VctStep& st : s) divs.push_back(st.occ_den);
        for (int k = 0; k < c->gloss.n; ++k)
            for (const VctStep& st : g[k]) divs.push_back(st.occ_den);
        for (float dv : divs) {
            bool good = false;
            PIPE_TRY(divisor_verified(c, dv, &good));
            if (!good) { ok = false; break; }
        }
    }
    c->fast_div = ok;
    // a table for the verified division carries what div_const<1> takes beside the reciprocal (its low word)
    // in the divisor's place; the IEEE-divide kernels of an unverified table keep the divisor
    if (ok) {
        for (VctStep& st : d) st.occ_den = vct_div_aux(st.occ_den, st.occ_rcp);
        for (VctStep& st : s) st.occ_den = vct_div_aux(st.occ_den, st.occ_rcp);
        for (int k = 0; k < c->gloss.n; ++k)
            for (VctStep& st : g[k]) st.occ_den = vct_div_aux(st.occ_den, st.occ_rcp);
    }
    HIP_TRY(c, hipMemcpyAsync(c->steps_dev.get(), d.data(), d.size() * sizeof(VctStep), hipMemcpyHostToDevice, cur(c).stream.get()));
    HIP_TRY(c, hipMemcpyAsync(c->steps_dev.get() + VCT_MAX_STEPS, s.data(), s.size() * sizeof(VctStep),
                              hipMemcpyHostToDevice, cur(c).stream.get()));
    if (c->gloss.n) {      // the class headers, then each class's table
        VctGlossTable* t = c->gloss.table.get();
        struct { int32_t nclasses, pad0[3], nsteps[8]; float shininess[8]; } head = {};
        head.nclasses = c->gloss.n;
        for (int k = 0; k < c->gloss.n; ++k) {
            head.nsteps[k] = c->gloss.nsteps[k] = (int)g[k].size();
            head.shininess[k] = c->gloss.cls[k].shininess;
        }
        static_assert(sizeof(head) <= offsetof(VctGlossTable, steps), "the headers fit in front of the tables");
        HIP_TRY(c, hipMemcpyAsync(t, &head, sizeof(head), hipMemcpyHostToDevice, cur(c).stream.get()));
        for (int k = 0; k < c->gloss.n; ++k)
            HIP_TRY(c, hipMemcpyAsync(&t->steps[k][0], g[k].data(), g[k].size() * sizeof(VctStep), hipMemcpyHostToDevice, cur(c).stream.get()));
        HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));   // head goes out of scope
    }
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));   // d, s go out of scope
    c->steps_dirty = false;
    return VCT_OK;
}

void vct_fill_march_params(const vct_ctx* c, VctTraceParams& p, const uint32_t* chain) {
    memset(&p, 0, sizeof(p));
    p.chain = chain;
    for (int l = 0; l < c->vol.nlev; ++l) p.level_off[l] = (uint32_t)vct_level_offset(c->cfg.voxel_dim, l);
    p.V = c->cfg.voxel_dim;
    p.nlev = c->vol.nlev;
    p.G = c->cfg.grid_world_size;
    p.half_G = c->cfg.grid_world_size * 0.5f;                       // trace.fs:61
    p.vs = c->cfg.grid_world_size / (float)c->cfg.voxel_dim;        // trace.fs:90
    p.half_G_rcp = 1.0f / p.half_G;
    p.half_G_aux = c->fast_div ? vct_div_aux(p.half_G, p.half_G_rcp) : p.half_G;
    p.fast_div = c->fast_div ? 1 : 0;
    p.max_alpha = c->cfg.max_alpha;
    p.wrap_repeat = c->cfg.wrap_repeat;
    p.spread_lut = c->spread_lut.get();
    p.chain_form = c->chain_form ? 1 : 0;
    // records of `c->vol.chain` only (the bounce chain has none), biased by the first level's offset
    p.cells_biased = (c->vol.cells_valid && chain == c->vol.chain.get())
                         ? (const char*)c->vol.cells.get() - ((size_t)vct_level_offset(c->cfg.voxel_dim, 1) << 5) : nullptr;
    p.steps_diffuse = c->steps_dev.get();
    p.steps_specular = c->steps_dev.get() + VCT_MAX_STEPS;
    p.n_diffuse = c->n_diffuse;
    p.n_specular = c->n_specular;
    p.step_counter = c->step_counter.get();
    p.tile_steps = cur(c).tile_steps.get();
#if defined(VCT_STATS) && VCT_STATS
    p.stats = c->stats.get();
#endif
}

// VctTraceParams::comp of a launch with lighting components: the mask, the cone groups something reads (include/vct.h),
// the outputs, whether the launch has pixel-emission planes, and the bit that selects the COMP kernel
uint32_t component_word(uint32_t mask, uint32_t aov_which, bool emission) {
    const bool diffuse = (mask & (VCT_SHOW_INDIRECT_DIFFUSE | VCT_SHOW_AMBIENT_OCCLUSION)) || (aov_which & VCT_AOV_INDIRECT_DIFFUSE);
    const bool specular = (mask & VCT_SHOW_INDIRECT_SPECULAR) ||
                          ((mask & VCT_SHOW_AMBIENT_OCCLUSION) && (mask & VCT_SHOW_SPECULAR)) ||
                          (aov_which & VCT_AOV_INDIRECT_SPECULAR);
    const uint32_t groups = (diffuse ? 1u : 0u) | (specular ? 2u : 0u);
    return VCT_COMP_ON | (emission ? VCT_COMP_EMISSION : 0u) | (aov_which << VCT_COMP_AOV_SHIFT) | (groups << VCT_COMP_GROUPS_SHIFT) |
           (mask & VCT_SHOW_ALL);
}

// `out_base`: where the kernel writes (full-frame addressing); null = the caller's vct_set_frame_target or the
// context-owned frame.  vct_frame_step passes its gather buffer here instead of re-pointing the frame target, which
// on a non-root rank would leave a pointer BEFORE a one-slab allocation behind for every later full-frame call.
int vct_launch_trace_rows(vct_ctx* c, int row0, int row1, uint16_t* out_base, int row_stride, bool pack_rows) {
    // the reference rebuilds the mips right after every voxelization (VCT.h:248); tracing a chain whose
    // coarse levels describe an older level 0 would return wrong GI without any sign of it
    if (!c->vol.mips_valid) return vct_fail(c, VCT_ERR_INVALID, "trace: level 0 changed since the last vct_build_mips (call it first)");
    PIPE_TRY(vct_refresh_steps(c));
    if (c->cfg.debug_outputs && (c->n_diffuse > 255 || c->n_specular > 255))
        return vct_fail(c, VCT_ERR_INVALID, "debug_outputs keeps per-cone step counts as uint8: this aperture needs more than 255 steps");
    VctTraceParams p;
    vct_fill_march_params(c, p, c->vol.active());
    for (int i = 0; i < 3; ++i) { p.cam[i] = c->cam[i]; p.light[i] = c->light[i]; }
    p.ambient = c->cfg.ambient_factor;
    p.shininess = c->cfg.shininess;
    p.width = c->cfg.width;
    p.height = c->cfg.height;
    p.tiles_x = vct_tiles_x(c);
    p.tiles_y = vct_tiles_y(c);
    p.tile_row0 = row0;
    p.tile_row1 = row1;
    p.row_stride = row_stride;
    p.pack_rows = pack_rows ? 1 : 0;
    const int variant = c->cfg.trace_variant;
    // what is attached against how this context traces (vct_feature_rules.h): the setters keep such a pair from coming about
    const VctRulesInForce rules = vct_rules_in_force(c);
    PIPE_TRY(vct_refuse_conflict(c, "trace", rules.features, rules.modes));
    const bool compacting = variant == 4 && !c->cfg.anisotropic_mips;      // variant 4 is in effect (it has no directional form)
    if ((row_stride > 1 || pack_rows) && !vct_variant_takes_row_subsets(variant))
        return vct_fail(c, VCT_ERR_INVALID, "interleaved tile rows need the default trace kernel (config.trace_variant 0 or 3)");
    const int rstride = row_stride > 1 ? row_stride : 1;
    p.spec_prio = ((row1 - row0) / rstride) * 2 <= vct_tiles_y(c) ? 1 : 0;
    p.gbuf = cur(c).gb_current;
    p.aniso = c->cfg.anisotropic_mips ? c->vol.aniso.get() : nullptr;
    p.aniso_alt_slab = 128;     // k_trace_tile_split<ANISO>: slabs [level 1][level 2][-axis of 1][-axis of 2]
    p.aniso_stride = (uint32_t)(c->vol.chain_texels - c->vol.nvox());
    p.out = out_base ? out_base : (cur(c).frame_out());
    p.dbg_steps = c->cfg.debug_outputs ? c->dbg_steps.get() : nullptr;
    p.dbg_cones = c->cfg.debug_outputs ? c->dbg_cones.get() : nullptr;
    // lighting components (include/vct.h): the COMP kernel only when the mask or an output asks for it.  A packed slab
    // (interleaved ranks, whose contexts refuse outputs; the one-GPU self-test) writes no outputs.
    const uint32_t aov_which = pack_rows ? 0u : c->aov_which;
    // half-rate diffuse gather (include/vct.h): whole frames only; the pass composites in the COMP kernel whatever the mask
    // (VCT_SHOW_ALL there is the unmasked arithmetic), and when nothing reads the diffuse group it is rate 1's launch
    const bool half = c->diffuse_rate == 2;
    bool half_march = false;
    // pixel-emission planes of the slot (include/vct.h "emissive materials"): the composite adds them, in the COMP kernel
    const float* pix_emis = cur(c).emis.get();
    // local lights (include/vct.h "local lights"): the slot's lit planes -- filled below, right in front of the launch, with
    // E + Lit -- take the planes' place
    const float* lit = c->lights.n ? cur(c).lit.get() : nullptr;
    const float* slot_emis = pix_emis;
    if (lit) pix_emis = lit;
    p.pix_emis = pix_emis;
    // gloss classes (include/vct.h "per-material gloss"): the slot's plane and the class tables, in the COMP kernel's
    // GLOSS form; config.shininess and the specular table are then not read by this launch
    const uint8_t* pix_gloss = c->gloss.n ? cur(c).gloss.get() : nullptr;
    if (pix_gloss) { p.gloss = c->gloss.table.get(); p.pix_gloss = pix_gloss; }
    // sky light (include/vct.h "sky light"): the context's folded coefficients, in the COMP kernel's SKY form
    const float* sky = c->sky.dev();
    p.sky = sky;
    if (half) {
        if (row0 != 0 || row1 != vct_tiles_y(c) || row_stride > 1 || pack_rows)
            return vct_fail(c, VCT_ERR_INVALID, "trace: diffuse rate 2 traces whole frames only (no slabs, tile-row ranges or interleaved rows)");
        if (!cur(c).dr_ind) return vct_fail(c, VCT_ERR_INVALID, "trace: diffuse rate 2 on a frame slot without its buffers");
        p.comp = component_word(c->show_mask, aov_which, pix_emis != nullptr);
        p.aov = aov_which ? cur(c).aov.get() : nullptr;
        half_march = ((p.comp >> VCT_COMP_GROUPS_SHIFT) & 1u) != 0u;
        if (half_march) {
            p.dr_ind = cur(c).dr_ind.get(); p.dr_coarse = cur(c).dr_coarse.get(); p.dr_anchor = cur(c).dr_anchor.get();
            p.dr_list = cur(c).dr_list.get(); p.dr_ctr = cur(c).dr_ctr.get();
            p.dr_waves = c->diffuse_rate_waves;
        }
    } else if (c->show_mask != VCT_SHOW_ALL || aov_which || pix_emis || pix_gloss || sky) {
        p.comp = component_word(c->show_mask, aov_which, pix_emis != nullptr);
        p.aov = aov_which ? cur(c).aov.get() : nullptr;
    }
#if defined(VCT_STATS) && VCT_STATS
    HIP_TRY(c, hipMemsetAsync(c->stats.get(), 0, 32 * sizeof(unsigned long long), cur(c).stream.get()));
#endif
    if (compacting) {       // live-pixel compaction (experiment): list + counter, zeroed per launch
        const size_t nt = (size_t)vct_tiles_x(c) * vct_tiles_y(c);
        HIP_TRY(c, c->vt_pix.reserve(nt * 64 + 4));
        p.vt_pix = c->vt_pix.get();
        p.vt_count = c->vt_pix.get() + nt * 64;
        HIP_TRY(c, hipMemsetAsync(p.vt_count, 0, sizeof(uint32_t), cur(c).stream.get()));
    }
    if (lit) {
        VctLightPixArgs la;
        memset(&la, 0, sizeof(la));
        la.lights = c->lights.table.get(); la.nlights = c->lights.n;
        la.width = c->cfg.width; la.height = c->cfg.height; la.tiles_x = vct_tiles_x(c);
        la.row0 = row0; la.row1 = row1;      // (a strided launch: every row of the range)
        for (int i = 0; i < 3; ++i) la.cam[i] = c->cam[i];
        la.shininess = c->cfg.shininess;
        la.show = c->show_mask;
        la.gbuf = cur(c).gb_current; la.emis = slot_emis; la.pix_gloss = pix_gloss;
        la.nclasses = c->gloss.n;
        for (int k = 0; k < c->gloss.n; ++k) la.class_shininess[k] = c->gloss.cls[k].shininess;
        la.lit = cur(c).lit.get();
        HIP_TRY(c, cur(c).lit_timer.begin(cur(c).stream.get(), c->time_traces));
        HIP_TRY(c, vct_launch_light_pixels(la, cur(c).stream.get()));
        HIP_TRY(c, cur(c).lit_timer.end(cur(c).stream.get()));
    }
    HIP_TRY(c, cur(c).march.begin(cur(c).stream.get(), c->time_traces));      // (vct_set_trace_timing)
    const hipEvent_t marks[3] = {cur(c).dr_ev[0].get(), cur(c).dr_ev[1].get(), cur(c).dr_ev[2].get()};
    HIP_TRY(c, vct_launch_trace(p, variant, cur(c).stream.get(), &c->last_march_form,       // an empty row range (a rank without rows) launches nothing
                                half_march && c->time_traces ? marks : nullptr));
    HIP_TRY(c, cur(c).march.end(cur(c).stream.get()));
    cur(c).last_trace_half = half_march;
    cur(c).last_row0 = row0;
    cur(c).last_row1 = row1;
    cur(c).last_row_stride = rstride;
    cur(c).last_was_screen_trace = true;
    cur(c).last_trace_compacted = compacting;
    return VCT_OK;
}

// The trace kernels fetch texels through typed-buffer loads and rely on the texture path converting a UNORM8 channel to
// exactly (float)c / 255.0f.  Every byte value in every channel position (1,024 texels) through that path against the
// library's exact decode; *bad_decode = channels that differ (0 on gfx950: tools/unorm_probe.hip).  And the same texels as
// two levels of a chain, through one resource over the chain with the levels' byte offsets in the loads' scalar offset
// operand (the CHAIN forms of the default trace kernel, vct_trace.hip ChainRef): *bad_offset = channels whose bits are not the
// zero-offset load's.
int vct_texel_buffer_selftest(vct_ctx* c, uint64_t* bad_decode, uint64_t* bad_offset) {
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t lead = 8u, n = 1024u;                // (a chain's smallest level in front of others holds 8 texels)
    std::vector<uint32_t> h(lead + 2u * n, 0xdeadbeefu);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = i & 255u, k = i >> 8;       // byte b in channel k, the other channels vary with it
        const uint32_t o0 = (b * 7u + 3u) & 255u, o1 = 255u - b, o2 = (b * 13u + 5u) & 255u;
        const uint32_t ch[4] = {o0, o1, o2, b};
        h[lead + i] = h[lead + n + i] =
            ch[(0 + 3 - k) & 3] | (ch[(1 + 3 - k) & 3] << 8) | (ch[(2 + 3 - k) & 3] << 16) | (ch[(3 + 3 - k) & 3] << 24);
    }
    VctBuf<uint32_t> d;
    HIP_TRY(c, d.alloc(h.size()));
    HIP_TRY(c, hipMemcpyAsync(d.get(), h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, cur(c).stream.get()));
    unsigned long long v[4] = {0, 0, 0, 0};
    PIPE_TRY(selftest_words(c, v, [&](unsigned long long* w, hipStream_t st) { return vct_launch_texel_buffer_selftest(d.get(), lead, n, w, st); }));
    *bad_decode = v[0];
    *bad_offset = v[2];
    if (v[0] || v[2]) {
        char msg[224];
        snprintf(msg, sizeof(msg), "texel buffer: %llu channel values differ from (float)c / 255.0f, e.g. texel 0x%08llx; %llu differ "
                 "between a load with a scalar offset and one without, e.g. texel 0x%08llx", v[0], v[1], v[2], v[3]);
        c->err = msg;
    }
    return VCT_OK;
}

extern "C" {

// the rows of the last screen trace again (vct_trace_resident, vct_gi_pass) -- at diffuse rate 2 the whole frame
static int launch_trace_last_rows(vct_ctx* c) {
    if (c->diffuse_rate == 2) return vct_launch_trace_rows(c, 0, vct_tiles_y(c));
    return vct_launch_trace_rows(c, cur(c).last_row0, cur(c).last_row1, nullptr, cur(c).last_row_stride, false);
}

static int bind_gbuffer(vct_ctx* c, const vct_gbuffer* gb) {
    if (!gb || !gb->planes) return vct_fail(c, VCT_ERR_INVALID, "vct_trace: null G-buffer");
    if (gb->width != c->cfg.width || gb->height != c->cfg.height)
        return vct_fail(c, VCT_ERR_INVALID, "vct_trace: G-buffer size differs from the context's frame");
    if (gb->layout != VCT_GB_LINEAR && gb->layout != VCT_GB_TILED) return vct_fail(c, VCT_ERR_INVALID, "vct_trace: unknown G-buffer layout");
    if (gb->layout == VCT_GB_TILED && gb->location == VCT_MEM_DEVICE) {
        cur(c).gb_current = gb->planes;     // zero-copy: trace reads the caller's HBM buffer
        return VCT_OK;
    }
    PIPE_TRY(vct_planes_set(c, cur(c).gb_tiled.get(), gb->planes, gb->layout, gb->location, VCT_GB_NPLANES, sizeof(float)));
    cur(c).gb_current = cur(c).gb_tiled.get();
    return VCT_OK;
}

// bytes [off, off + bytes) of the frame into the same range of the caller's `out` (host or device), on the slot's stream
static int copy_frame_out(vct_ctx* c, void* out, int32_t out_location, size_t off, size_t bytes) {
    HIP_TRY(c, hipMemcpyAsync((char*)out + off, (const char*)cur(c).frame_out() + off, bytes,
                              out_location == VCT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, cur(c).stream.get()));
    return VCT_OK;
}

static int trace_rows(vct_ctx* c, const vct_gbuffer* gb, int32_t row0, int32_t row1, void* out, int32_t out_location) {
    if (!vct_rows_in_frame(c, row0, row1)) return vct_fail(c, VCT_ERR_INVALID, "vct_trace_slab: tile-row range outside the frame");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(bind_gbuffer(c, gb));
    cur(c).have_gbuffer = true;
    PIPE_TRY(vct_launch_trace_rows(c, row0, row1));
    if (out) {
        const int y0 = row0 * VCT_TILE;
        const int y1 = row1 * VCT_TILE < c->cfg.height ? row1 * VCT_TILE : c->cfg.height;
        if (y1 > y0) {
            const size_t off = (size_t)y0 * c->cfg.width * 8, bytes = (size_t)(y1 - y0) * c->cfg.width * 8;
            PIPE_TRY(copy_frame_out(c, out, out_location, off, bytes));
        }
    }
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

int vct_trace_slab(vct_ctx* c, const vct_gbuffer* gb, int32_t row0, int32_t row1, void* out, int32_t out_location) {
    if (!c) return VCT_ERR_INVALID;
    if (c->diffuse_rate == 2) return vct_fail(c, VCT_ERR_INVALID, "vct_trace_slab: diffuse rate 2 traces whole frames only (vct_trace)");
    return trace_rows(c, gb, row0, row1, out, out_location);
}

int vct_trace(vct_ctx* c, const vct_gbuffer* gb, void* out, int32_t out_location) {
    if (!c) return VCT_ERR_INVALID;
    return trace_rows(c, gb, 0, vct_tiles_y(c), out, out_location);
}

int vct_trace_current(vct_ctx* c, void* out, int32_t out_location) {
    if (!c) return VCT_ERR_INVALID;
    if (!cur(c).have_gbuffer) return vct_fail(c, VCT_ERR_INVALID, "vct_trace_current: no G-buffer resident yet");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_launch_trace_rows(c, 0, vct_tiles_y(c)));
    if (out) PIPE_TRY(copy_frame_out(c, out, out_location, 0, (size_t)c->cfg.width * c->cfg.height * 8));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

int vct_trace_resident_rows(vct_ctx* c, int32_t row0, int32_t row1) {
    if (!c) return VCT_ERR_INVALID;
    if (c->diffuse_rate == 2) return vct_fail(c, VCT_ERR_INVALID, "vct_trace_resident_rows: diffuse rate 2 traces whole frames only (vct_trace_resident)");
    if (!cur(c).have_gbuffer) return vct_fail(c, VCT_ERR_INVALID, "vct_trace_resident_rows: no G-buffer resident yet");
    if (!vct_rows_in_frame(c, row0, row1)) return vct_fail(c, VCT_ERR_INVALID, "vct_trace_resident_rows: tile-row range outside the frame");
    HIP_TRY(c, hipSetDevice(c->device));
    return vct_launch_trace_rows(c, row0, row1);
}

int vct_trace_resident_strided(vct_ctx* c, int32_t row0, int32_t row1, int32_t stride) {
    if (!c) return VCT_ERR_INVALID;
    if (c->diffuse_rate == 2) return vct_fail(c, VCT_ERR_INVALID, "vct_trace_resident_strided: diffuse rate 2 traces whole frames only (vct_trace_resident)");
    if (!cur(c).have_gbuffer) return vct_fail(c, VCT_ERR_INVALID, "vct_trace_resident_strided: no G-buffer resident yet");
    if (!vct_rows_in_frame(c, row0, row1) || stride < 1)
        return vct_fail(c, VCT_ERR_INVALID, "vct_trace_resident_strided: tile-row range outside the frame or stride < 1");
    HIP_TRY(c, hipSetDevice(c->device));
    return vct_launch_trace_rows(c, row0, row1, nullptr, stride, false);
}

int vct_trace_resident(vct_ctx* c) {
    if (!c) return VCT_ERR_INVALID;
    if (!cur(c).have_gbuffer) return vct_fail(c, VCT_ERR_INVALID, "vct_trace_resident: no G-buffer resident yet");
    HIP_TRY(c, hipSetDevice(c->device));
    return launch_trace_last_rows(c);
}

int vct_gi_pass(vct_ctx* c, const float light_vp[16], const float view_proj[16], int32_t mode) {
    if (!c) return VCT_ERR_INVALID;
    if (!light_vp || !view_proj) return vct_fail(c, VCT_ERR_INVALID, "vct_gi_pass: null matrix");
    if (c->cfg.shadow_map_size <= 0) return vct_fail(c, VCT_ERR_INVALID, "vct_gi_pass: config.shadow_map_size <= 0");
    // A rank of a multi-GPU frame (vct_comm_init) runs the same pass on its slab: the G-buffer stream is scissored to
    // the rank's tile rows and the pass ends with vct_frame_step (slab trace + the frame's one gather) at the join.
    int row0 = 0, row1 = vct_tiles_y(c);
    const bool rank_ctx = vct_comm_rows(c, &row0, &row1);
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_pipeline_join(c));
    // VCT_GI_ONE_STREAM=1 (A/B): the six stages in sequence on the context's stream, no fork / join events
    static const bool one_stream = [] { const char* e = getenv("VCT_GI_ONE_STREAM"); return e && e[0] == '1'; }();
    if (one_stream) {
        int rc1 = vct_render_shadow_map(c, light_vp);
        if (rc1 == VCT_OK) rc1 = vct_voxelize(c, mode);
        if (rc1 == VCT_OK) rc1 = vct_inject_light(c);
        if (rc1 == VCT_OK) rc1 = vct_build_mips(c);
        if (rc1 == VCT_OK) rc1 = vct_render_gbuffer_rows_on(c, view_proj, row0, row1, cur(c).stream.get());
        if (rc1) return rc1;
        if (rank_ctx) return vct_frame_step(c);
        return launch_trace_last_rows(c);
    }
    VctForkJoin& fj = c->fork;
    if (!fj.aux) {
        hipStream_t aux = nullptr;
        if (c->reserved_cus > 0) {
            hipDeviceProp_t prop;
            HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
            HIP_TRY(c, vct_create_masked_stream(&aux, c->device, 0, prop.multiProcessorCount - c->reserved_cus));
        } else {
            bool ov = false;      // a stream that shares the context stream's hardware queue would run the two halves in sequence
            PIPE_TRY(vct_create_overlapping_stream(c, cur(c).stream.get(), &aux, &ov));
        }
        fj.aux.adopt(aux);
    }
    for (VctEvent* ev : {&fj.ev_fork, &fj.ev_shadow, &fj.ev_join})
        if (!*ev) HIP_TRY(c, ev->create(hipEventDisableTiming));
    // fork at once: the main draw's VISIBILITY raster needs nothing of this pass (it has its own lists and words);
    // only its shading kernel reads the shadow map (PCF term), so that alone waits for the shadow pass
    HIP_TRY(c, hipEventRecord(fj.ev_fork.get(), cur(c).stream.get()));                 // everything issued before this call is done
    HIP_TRY(c, hipStreamWaitEvent(fj.aux.get(), fj.ev_fork.get(), 0));
    int rc = vct_render_shadow_map(c, light_vp);                       // allocates / sizes the shadow map first
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(fj.ev_shadow.get(), cur(c).stream.get()));
    rc = vct_render_gbuffer_rows_on(c, view_proj, row0, row1, fj.aux.get(), fj.ev_shadow.get());
    // join before anything else can fail: later work on the context's stream must see the G-buffer
    const hipError_t ej = hipEventRecord(fj.ev_join.get(), fj.aux.get());
    if (rc == VCT_OK) rc = vct_voxelize(c, mode);
    if (rc == VCT_OK) rc = vct_inject_light(c);
    if (rc == VCT_OK) rc = vct_build_mips(c);
    if (ej == hipSuccess) HIP_TRY(c, hipStreamWaitEvent(cur(c).stream.get(), fj.ev_join.get(), 0));
    else HIP_TRY(c, ej);
    if (rc) return rc;
    if (rank_ctx) return vct_frame_step(c);
    return launch_trace_last_rows(c);
}

int vct_download_frame(vct_ctx* c, void* out) {
    if (!c || !out) return VCT_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(copy_frame_out(c, out, VCT_MEM_HOST, 0, (size_t)c->cfg.width * c->cfg.height * 8));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

int vct_set_frame_target(vct_ctx* c, void* dev) {
    if (!c) return VCT_ERR_INVALID;
    cur(c).frame_target = (uint16_t*)dev;
    return VCT_OK;
}

int vct_download_steps(vct_ctx* c, uint8_t* steps) {
    if (!c || !steps) return VCT_ERR_INVALID;
    if (!c->dbg_steps) return vct_fail(c, VCT_ERR_INVALID, "context created without debug_outputs");
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    HIP_TRY(c, hipMemcpy(steps, c->dbg_steps.get(), (size_t)c->cfg.width * c->cfg.height * 7, hipMemcpyDeviceToHost));
    return VCT_OK;
}

int vct_download_cones(vct_ctx* c, float* cones) {
    if (!c || !cones) return VCT_ERR_INVALID;
    if (!c->dbg_cones) return vct_fail(c, VCT_ERR_INVALID, "context created without debug_outputs");
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    HIP_TRY(c, hipMemcpy(cones, c->dbg_cones.get(), (size_t)c->cfg.width * c->cfg.height * 28 * sizeof(float), hipMemcpyDeviceToHost));
    return VCT_OK;
}

// executed steps per tile row of the last screen trace: sums of the waves' slots over the launched rows
static int row_steps(vct_ctx* c, std::vector<uint64_t>& rows) {
    const int tx = vct_tiles_x(c), ty = vct_tiles_y(c);
    rows.assign((size_t)ty, 0);
    const int r0 = cur(c).last_row0, r1 = cur(c).last_row1;
    if (r1 <= r0) return VCT_OK;
    const size_t per_row = (size_t)tx;
    std::vector<uint32_t> v(per_row * (size_t)(r1 - r0));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    HIP_TRY(c, hipMemcpy(v.data(), cur(c).tile_steps.get() + per_row * (size_t)r0, v.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int r = r0; r < r1; ++r) {
        if ((r - r0) % cur(c).last_row_stride) continue;          // an interleaved launch: the other rows belong to other ranks
        uint64_t sum = 0;
        const uint32_t* q = v.data() + per_row * (size_t)(r - r0);
        for (size_t i = 0; i < per_row; ++i) sum += q[i];
        rows[(size_t)r] = sum;
    }
    return VCT_OK;
}

int vct_set_trace_timing(vct_ctx* c, int32_t on) {
    if (!c) return VCT_ERR_INVALID;
    c->time_traces = on != 0;
    return VCT_OK;
}

int vct_get_stage_counts(vct_ctx* c, uint64_t out[8]) {
    if (!c || !out) return VCT_ERR_INVALID;
    memset(out, 0, 8 * sizeof(uint64_t));
    out[0] = (uint64_t)c->mesh.ntri;
    out[1] = c->vox.n_frags;
    // bits 0-7 division form of the last march launch: 0 none, 1 IEEE, 2 product, 3 x * r; bits 8-9 (screen traces) how its
    // typed loads reached a level: 1 a resource per level, 2 one per wave (include/vct.h)
    out[2] = (uint64_t)c->last_march_form;
    out[3] = c->vox.nslots;
    out[5] = (uint64_t)c->reserved_cus;          // compute units kept for the communication stream (VCT_COMM_RESERVED_CUS)
    out[6] = (uint64_t)c->raster_form.last_form;      // visibility form of the last main-draw pass: 1 direct, 2 tile-binned
    out[7] = (uint64_t)c->vox.n_items;           // work items of the voxelize pass (slots, heavy ones cut into chunks)
    if (c->vol.brick_prev) {
        HIP_TRY(c, hipSetDevice(c->device));
        const size_t nbricks = c->vol.nbricks();
        std::vector<uint32_t> flags(nbricks);
        HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
        HIP_TRY(c, hipMemcpy(flags.data(), c->vol.brick_prev.get(), nbricks * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint64_t n = 0;
        for (uint32_t f : flags) n += f != 0u;
        out[4] = n;
    }
    return VCT_OK;
}

int vct_last_step_count(vct_ctx* c, uint64_t* steps) {
    if (!c || !steps) return VCT_ERR_INVALID;
    if (!cur(c).march.have) return vct_fail(c, VCT_ERR_INVALID, "no trace has run");
    HIP_TRY(c, hipSetDevice(c->device));
    uint64_t sum = 0;
    if (cur(c).last_was_screen_trace) {
        std::vector<uint64_t> rows;
        PIPE_TRY(row_steps(c, rows));
        for (uint64_t r : rows) sum += r;
        if (cur(c).last_trace_half) {       // + the coarse and the fill march of a half-rate pass (the stream is idle by now)
            std::vector<unsigned long long> v(VCT_DR_COUNTERS);
            HIP_TRY(c, hipMemcpy(v.data(), cur(c).dr_ctr.get(), v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (unsigned long long w : v) sum += w;
        }
    } else {        // a bounce: its kernels add into the atomic bank
        HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
        unsigned long long v[VCT_STEP_COUNTERS];
        HIP_TRY(c, hipMemcpy(v, c->step_counter.get(), sizeof(v), hipMemcpyDeviceToHost));
        for (int i = 0; i < VCT_STEP_COUNTERS; ++i) sum += v[i];
    }
    *steps = sum;
    return VCT_OK;
}

int vct_last_row_steps(vct_ctx* c, uint64_t* rows, int32_t nrows) {
    if (!c || !rows) return VCT_ERR_INVALID;
    if (!cur(c).march.have || !cur(c).last_was_screen_trace)
        return vct_fail(c, VCT_ERR_INVALID, "vct_last_row_steps: the last march was not a screen trace");
    if (nrows != vct_tiles_y(c)) return vct_fail(c, VCT_ERR_INVALID, "vct_last_row_steps: nrows must be the frame's tile rows, ceil(height / 8)");
    if (c->diffuse_rate == 2 || cur(c).last_trace_half)
        return vct_fail(c, VCT_ERR_INVALID, "vct_last_row_steps: diffuse rate 2 keeps no per-row histogram (its marches are not per tile row)");
    // trace_variant 4 stores its step counts per VIRTUAL tile of the compaction list: only their total means anything
    if (cur(c).last_trace_compacted)
        return vct_fail(c, VCT_ERR_INVALID, "vct_last_row_steps: the last trace was compacted (config.trace_variant 4): no per-row histogram");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<uint64_t> v;
    PIPE_TRY(row_steps(c, v));
    memcpy(rows, v.data(), (size_t)nrows * sizeof(uint64_t));
    return VCT_OK;
}

int vct_last_trace_stats(vct_ctx* c, uint64_t out[32]) {
    if (!c || !out) return VCT_ERR_INVALID;
#if defined(VCT_STATS) && VCT_STATS
    if (!cur(c).march.have) return vct_fail(c, VCT_ERR_INVALID, "no trace has run");
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    HIP_TRY(c, hipMemcpy(out, c->stats.get(), 32 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VCT_OK;
#else
    return vct_fail(c, VCT_ERR_INVALID, "vct_last_trace_stats: this library was built without -DVCT_STATS=1 "
                                    "(tools/build_ab.sh stats \"-DVCT_STATS=1\")");
#endif
}

int vct_last_trace_ms(vct_ctx* c, float* ms) {
    if (!c || !ms) return VCT_ERR_INVALID;
    return vct_timer_ms(c, cur(c).march, ms, "no trace has run", "vct_last_trace_ms: the last trace was issued with timing off (vct_set_trace_timing)");
}

int vct_selftest_const_divide(vct_ctx* c, float d, uint64_t* mismatches) {
    if (!c || !mismatches) return VCT_ERR_INVALID;
    if (!divisor_ok(d)) return vct_fail(c, VCT_ERR_INVALID, "divisor outside the set the FMA division is proven for");
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned long long v[2] = {0, 0};
    PIPE_TRY(selftest_words(c, v, [&](unsigned long long* w, hipStream_t st) { return vct_launch_divide_selftest(d, w, st); }));
    *mismatches = v[0];
    if (v[0]) {      // not a failure of the call: leave one offending x readable for diagnosis
        char msg[96];
        snprintf(msg, sizeof(msg), "const divide by %.9g: %llu mismatches, e.g. x bits 0x%08llx", d, v[0], v[1]);
        c->err = msg;
    }
    return VCT_OK;
}

// vct_texel_buffer_selftest (above): both of its counts
int vct_selftest_texel_buffer(vct_ctx* c, uint64_t* mismatches) {
    if (!c || !mismatches) return VCT_ERR_INVALID;
    uint64_t decode = 0, offset = 0;
    PIPE_TRY(vct_texel_buffer_selftest(c, &decode, &offset));
    *mismatches = decode + offset;
    return VCT_OK;
}

int vct_selftest_area_divide(vct_ctx* c, uint64_t seed, uint64_t count, uint64_t* mismatches) {
    if (!c || !mismatches) return VCT_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned long long v[2] = {0, 0};
    PIPE_TRY(selftest_words(c, v, [&](unsigned long long* w, hipStream_t st) { return vct_launch_area_divide_selftest(seed, count, w, st); }));
    *mismatches = v[0];
    if (v[0]) {
        char msg[96];
        snprintf(msg, sizeof(msg), "area divide: %llu mismatches, e.g. sample %llu of seed %llu", v[0], v[1],
                 (unsigned long long)seed);
        c->err = msg;
    }
    return VCT_OK;
}

int vct_set_aov_outputs(vct_ctx* c, uint32_t which) {
    if (!c) return VCT_ERR_INVALID;
    if (which & ~(uint32_t)(VCT_AOV_INDIRECT_DIFFUSE | VCT_AOV_INDIRECT_SPECULAR | VCT_AOV_DIRECT))
        return vct_fail(c, VCT_ERR_INVALID, "vct_set_aov_outputs: unknown output bits");
    if (which) PIPE_TRY(vct_refuse_conflict(c, "vct_set_aov_outputs", VCT_FEAT_AOV, vct_rules_in_force(c).modes));
    if (which == c->aov_which) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));            // the buffers being replaced may still be written
    // every live slot's set, allocated here and never in a launch
    const size_t bytes = vct_aov_frames(which) * (size_t)c->cfg.width * c->cfg.height * 8;
    VctBuf<uint16_t> fresh[2];
    hipError_t e = hipSuccess;
    for (int k = 0; k < c->frames_in_flight && bytes && e == hipSuccess; ++k) {
        e = fresh[k].alloc(bytes / 2);
        if (e == hipSuccess) e = hipMemset(fresh[k].get(), 0, bytes);
    }
    if (e != hipSuccess)            // all or nothing: the old sets stay
        return vct_fail(c, e == hipErrorOutOfMemory ? VCT_ERR_NOMEM : VCT_ERR_DEVICE, std::string("vct_set_aov_outputs: ") + hipGetErrorString(e));
    for (int k = 0; k < c->frames_in_flight; ++k) c->slots[k].aov = std::move(fresh[k]);
    c->aov_which = which;
    return VCT_OK;
}

// the output `bit` of the selected slot: device address (null when the bit is not exactly one output that is on)
static uint16_t* aov_of(const vct_ctx* c, uint32_t bit) {
    if (bit == 0 || (bit & (bit - 1)) || !(c->aov_which & bit) || !cur(c).aov) return nullptr;
    return cur(c).aov.get() + vct_aov_frames(c->aov_which & (bit - 1)) * (size_t)c->cfg.width * c->cfg.height * 4;
}

int vct_download_aov(vct_ctx* c, uint32_t bit, void* out) {
    if (!c || !out) return VCT_ERR_INVALID;
    const uint16_t* src = aov_of(c, bit);
    if (!src) return vct_fail(c, VCT_ERR_INVALID, "vct_download_aov: not one output that vct_set_aov_outputs turned on");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, src, (size_t)c->cfg.width * c->cfg.height * 8, hipMemcpyDeviceToHost, cur(c).stream.get()));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    return VCT_OK;
}

int vct_get_aov_device(vct_ctx* c, uint32_t bit, void** p, size_t* bytes) {
    if (!c || !p) return VCT_ERR_INVALID;
    uint16_t* src = aov_of(c, bit);
    if (!src) return vct_fail(c, VCT_ERR_INVALID, "vct_get_aov_device: not one output that vct_set_aov_outputs turned on");
    *p = src;
    if (bytes) *bytes = (size_t)c->cfg.width * c->cfg.height * 8;
    return VCT_OK;
}

// ---- half-rate diffuse gather (include/vct.h) ---------------------------------------------------------------------------
int vct_set_diffuse_rate(vct_ctx* c, int32_t rate) {
    if (!c) return VCT_ERR_INVALID;
    if (rate != 1 && rate != 2) return vct_fail(c, VCT_ERR_INVALID, "vct_set_diffuse_rate: 1 or 2");
    if (rate == 2) PIPE_TRY(vct_refuse_conflict(c, "vct_set_diffuse_rate", VCT_FEAT_RATE2, vct_rules_in_force(c).modes));
    if (rate == c->diffuse_rate) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_synchronize(c));            // buffers about to go may still be read
    if (rate == 2) {
        // every live slot's set, allocated here and never in a launch; all or nothing
        hipError_t e = hipSuccess;
        for (int k = 0; k < c->frames_in_flight && e == hipSuccess; ++k) {
            e = c->slots[k].alloc_half_rate(c->cfg.width, c->cfg.height);
            if (e == hipSuccess) e = hipStreamSynchronize(c->slots[k].stream.get());
        }
        if (e != hipSuccess) {
            for (int k = 0; k < c->frames_in_flight; ++k) c->slots[k].free_half_rate();
            return vct_fail(c, e == hipErrorOutOfMemory ? VCT_ERR_NOMEM : VCT_ERR_DEVICE, std::string("vct_set_diffuse_rate: ") + hipGetErrorString(e));
        }
        const char* w = getenv("VCT_DIFFUSE_RATE_WAVES");      // A/B of the march's workgroup shape
        c->diffuse_rate_waves = w && w[0] == '2' ? 2 : 1;
    } else {
        for (int k = 0; k < c->frames_in_flight; ++k) c->slots[k].free_half_rate();
    }
    c->diffuse_rate = rate;
    return VCT_OK;
}

int vct_get_diffuse_rate(const vct_ctx* c, int32_t* rate, uint64_t* marched_pixels) {
    if (!c) return VCT_ERR_INVALID;
    if (rate) *rate = c->diffuse_rate;
    if (marched_pixels) {
        *marched_pixels = 0;
        if (cur(c).march.have && cur(c).last_trace_half && cur(c).dr_ctr) {
            std::vector<unsigned long long> v(VCT_DR_COUNTERS);
            hipError_t e = hipSetDevice(c->device);
            if (e == hipSuccess) e = hipStreamSynchronize(cur(c).stream.get());
            if (e == hipSuccess)
                e = hipMemcpy(v.data(), cur(c).dr_ctr.get() + VCT_DR_COUNTERS, v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            if (e != hipSuccess) return vct_fail(const_cast<vct_ctx*>(c), VCT_ERR_DEVICE, std::string("vct_get_diffuse_rate: ") + hipGetErrorString(e));
            for (unsigned long long w : v) *marched_pixels += w;
        }
    }
    return VCT_OK;
}

int vct_last_diffuse_rate_ms(vct_ctx* c, float ms[4]) {
    if (!c || !ms) return VCT_ERR_INVALID;
    if (!cur(c).march.have || !cur(c).last_trace_half || !cur(c).last_was_screen_trace)
        return vct_fail(c, VCT_ERR_INVALID, "vct_last_diffuse_rate_ms: the last trace was no rate-2 pass that marched the diffuse group");
    if (!cur(c).march.timed)
        return vct_fail(c, VCT_ERR_INVALID, "vct_last_diffuse_rate_ms: the last trace was issued with timing off (vct_set_trace_timing)");
    HIP_TRY(c, hipEventSynchronize(cur(c).march.last()));
    const hipEvent_t ev[5] = {cur(c).march.first(), cur(c).dr_ev[0].get(), cur(c).dr_ev[1].get(), cur(c).dr_ev[2].get(), cur(c).march.last()};
    for (int i = 0; i < 4; ++i) HIP_TRY(c, hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    return VCT_OK;
}

int vct_get_frame_device(vct_ctx* c, void** p, size_t* bytes) {
    if (!c || !p) return VCT_ERR_INVALID;
    *p = cur(c).frame_out();
    if (bytes) *bytes = (size_t)c->cfg.width * c->cfg.height * 8;
    return VCT_OK;
}

}  // extern "C"
