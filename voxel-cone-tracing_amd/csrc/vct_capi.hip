// vct_capi.hip -- the C ABI declared in include/vct.h: context, HBM ownership, launch sequencing.
//
// Counterpart of the reference's orchestrator struct (R/Voxel_Cone_Tracing.h:11-252): where that
// owns GL object names and issues draws, this owns HBM buffers and issues HIP kernels on one
// stream.  No CPU fallback exists: every entry point that computes launches a kernel or fails.
#include <map>
#include <mutex>
#include <utility>

#include "vct_ctx.h"

namespace {

std::string g_create_error;

bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// ---- frame slots (vct_ctx.h VctFrameSlot) ----------------------------------------------------------------------------
// Does a candidate stream run BESIDE the context's stream?  HIP spreads a process' streams over a few hardware queues
// (four by default) and two streams that share one execute in order -- a second frame slot on such a stream buys nothing
// (measured: tools/pipe_probe.py with five streams alive, 0.632 ms per step against 0.592).  A spin kernel on the base
// stream stamps its end, a stamp kernel issued on the candidate right behind it stamps its start: the streams overlap
// iff the stamp's start precedes the spin's end.
__global__ void k_spin_stamp(long long ticks, unsigned long long* out) {
    const long long t0 = (long long)wall_clock64();
    while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
    out[0] = wall_clock64();
}
__global__ void k_stamp(unsigned long long* out) { out[1] = wall_clock64(); }

int streams_overlap(vct_ctx* c, hipStream_t base, hipStream_t cand, bool* overlap) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000;
    HIP_TRY(c, hipMemsetAsync(c->stats.get(), 0, 2 * sizeof(unsigned long long), base));
    HIP_TRY(c, hipStreamSynchronize(base));
    hipLaunchKernelGGL(k_spin_stamp, dim3(1), dim3(1), 0, base, (long long)khz * 3 / 10, c->stats.get());      // 0.3 ms
    hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, cand, c->stats.get());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(base));
    HIP_TRY(c, hipStreamSynchronize(cand));
    unsigned long long v[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(v, c->stats.get(), sizeof(v), hipMemcpyDeviceToHost));
    *overlap = v[1] != 0ull && v[1] < v[0];
    return VCT_OK;
}

// A slot on `stream`, which it owns from here on: timing events, G-buffer, frame, per-tile step counts and the
// per-component outputs that are on, zeroed on that stream.  A failure leaves a partial slot for slot_release.
hipError_t slot_create(vct_ctx* c, VctFrameSlot& s, hipStream_t stream) {
    const size_t npix = (size_t)c->cfg.width * c->cfg.height, nt = (size_t)vct_tiles_x(c) * vct_tiles_y(c);
    const size_t aov_halves = vct_aov_frames(c->aov_which) * npix * 4;
    s.stream.adopt(stream);
    hipError_t e = s.march.create();      // (no frame loop allocates them)
    if (e == hipSuccess) e = s.gb_tiled.alloc(vct_gb_tiled_floats(c));
    if (e == hipSuccess) e = s.frame.alloc(npix * 4);
    if (e == hipSuccess) e = s.tile_steps.alloc(nt);
    if (e == hipSuccess) e = hipMemsetAsync(s.gb_tiled.get(), 0, vct_gb_tiled_floats(c) * sizeof(float), stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.frame.get(), 0, npix * 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.tile_steps.get(), 0, nt * sizeof(uint32_t), stream);
    if (e == hipSuccess && aov_halves) e = s.aov.alloc(aov_halves);
    if (e == hipSuccess && aov_halves) e = hipMemsetAsync(s.aov.get(), 0, aov_halves * 2, stream);
    if (e == hipSuccess && c->diffuse_rate == 2) e = s.alloc_half_rate(c->cfg.width, c->cfg.height);
    if (e == hipSuccess && vct_emission_table_attached(c)) e = vct_emission_planes(c, s);      // material emission is attached (either mesh's): every slot has planes
    if (e == hipSuccess && c->gloss.n) e = vct_gloss_plane(c, s);      // gloss classes are attached: every slot has a plane
    if (e == hipSuccess && c->lights.n) e = vct_lights_planes(c, s);      // local lights are attached: every slot has lit planes
    s.gb_current = s.gb_tiled.get();
    return e;
}
// Waits for the slot's stream (its kernels may still read the slot's buffers); the fresh slot that takes its place
// frees the memory (its raster scratch too), the events and the stream.
void slot_release(VctFrameSlot& s) {
    if (s.stream) (void)hipStreamSynchronize(s.stream.get());
    s = VctFrameSlot();
}

// everything a fresh context owns on its device: slot 0 on the context's stream, the zeroed chain, the march's tables; then the texel-path check
int create_resources(vct_ctx* c) {
    const vct_config* cfg = &c->cfg;
    const int dev = c->device;
    HIP_TRY(c, hipSetDevice(dev));
    hipStream_t stream = nullptr;
    // VCT_STREAM_PRIORITY = high | low: experiments with two contexts sharing a GPU (tools/overlap_probe.py)
    int lo = 0, hi = 0;
    const char* pr = getenv("VCT_STREAM_PRIORITY");
    // VCT_COMM_RESERVED_CUS = k: the context's streams leave the device's last k compute units alone; the multi-GPU
    // step's communication stream gets exactly those (vct_ctx.h vct_create_masked_stream)
    const char* rc_ = getenv("VCT_COMM_RESERVED_CUS");
    c->reserved_cus = rc_ ? atoi(rc_) : 0;
    hipDeviceProp_t prop;
    HIP_TRY(c, hipGetDeviceProperties(&prop, dev));
    if (c->reserved_cus < 0 || c->reserved_cus >= prop.multiProcessorCount) c->reserved_cus = 0;
    if (c->reserved_cus > 0)
        HIP_TRY(c, vct_create_masked_stream(&stream, dev, 0, prop.multiProcessorCount - c->reserved_cus));
    else if (pr && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess)
        HIP_TRY(c, hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, pr[0] == 'h' ? hi : lo));
    else
        HIP_TRY(c, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_TRY(c, slot_create(c, c->slots[0], stream));      // slot 0: the context's stream
    // VCT_RASTER_PATH=binned | direct: the tile-binned visibility (round 4) or the direct form of rounds 2-3 (one
    // device-scope atomicMin per covered pixel) for both raster passes -- same results.  Unset: chosen per scene by
    // measurement (vct_ctx.h VctRasterForm).
    const char* rp = getenv("VCT_RASTER_PATH");
    c->raster_form.mode = !rp ? 0 : (rp[0] == 'b' ? 2 : (rp[0] == 'd' ? 1 : 0));
    for (VctEvent& ev : c->raster_form.ev) HIP_TRY(c, ev.create());
    if (const char* fr = getenv("VCT_FOOTPRINT_RECORDS")) c->vol.want_cells = fr[0] == '1';     // vct_set_footprint_records
    // VCT_BIN_TEST_CAPS="records,entries": the binned kernels are told these (smaller) capacities, so that a test can
    // drive the overflow paths -- sub-triangles rasterised in place, the merge by atomicMin -- on a small scene
    if (const char* tc = getenv("VCT_BIN_TEST_CAPS")) {
        unsigned a = 0, b = 0;
        if (sscanf(tc, "%u,%u", &a, &b) == 2) { c->raster_form.bin_test_caps[0] = a; c->raster_form.bin_test_caps[1] = b; }
    }
    VctChain& vol = c->vol;
    vol.V = cfg->voxel_dim;
    vol.nlev = vct_ilog2(vol.V) + 1;
    vol.chain_texels = vct_chain_texels(vol.V);
    HIP_TRY(c, vol.chain.alloc(vol.chain_texels));
    HIP_TRY(c, hipMemsetAsync(vol.chain.get(), 0, vol.chain_texels * 4, cur(c).stream.get()));   // VCT.h:115-119
    const size_t npix = (size_t)cfg->width * cfg->height;
    if (cfg->anisotropic_mips) {
        const size_t n = 6 * (vol.chain_texels - vol.nvox());
        HIP_TRY(c, vol.aniso.alloc(n));
        HIP_TRY(c, hipMemsetAsync(vol.aniso.get(), 0, n * 4, cur(c).stream.get()));
    }
    HIP_TRY(c, c->step_counter.alloc(VCT_STEP_COUNTERS));
    HIP_TRY(c, hipMemsetAsync(c->step_counter.get(), 0, VCT_STEP_COUNTERS * sizeof(unsigned long long), cur(c).stream.get()));
    HIP_TRY(c, c->stats.alloc(32));
    HIP_TRY(c, hipMemsetAsync(c->stats.get(), 0, 32 * sizeof(unsigned long long), cur(c).stream.get()));
    HIP_TRY(c, c->steps_dev.alloc(2 * VCT_MAX_STEPS));
    {
        std::vector<uint32_t> lut(1024);
        for (uint32_t i = 0; i < 1024u; ++i) lut[i] = vct_spread3(i) << 2;
        HIP_TRY(c, c->spread_lut.alloc(lut.size()));
        HIP_TRY(c, hipMemcpy(c->spread_lut.get(), lut.data(), lut.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (cfg->debug_outputs) {
        HIP_TRY(c, c->dbg_steps.alloc(npix * 7));
        HIP_TRY(c, c->dbg_cones.alloc(npix * 28));
        HIP_TRY(c, hipMemsetAsync(c->dbg_steps.get(), 0, npix * 7, cur(c).stream.get()));
        HIP_TRY(c, hipMemsetAsync(c->dbg_cones.get(), 0, npix * 28 * sizeof(float), cur(c).stream.get()));
    }
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    // once per process and device: the texture path's UNORM8 conversion must be the exact decode the trace kernels count on
    // (it is on gfx950).  No other path is compiled in: a device where it is not fails here, loudly.
    // The same run checks the loads' scalar offset operand, which the CHAIN forms of the default trace kernel rest on
    // (vct_trace.hip ChainRef): a device that fails that part traces with a resource per level instead.  So does a chain with a level at
    // or beyond 4 GiB, and any chain under VCT_LEVEL_DESCRIPTORS=1 (tests: both forms on one small chain; same bits).
    static std::mutex lock;
    static std::map<int, std::pair<uint64_t, uint64_t>> verdict;      // channel values that differ: decode, offset read
    std::lock_guard<std::mutex> g(lock);
    auto it = verdict.find(c->device);
    if (it == verdict.end()) {
        uint64_t bad = 0, bad_offset = 0;
        PIPE_TRY(vct_texel_buffer_selftest(c, &bad, &bad_offset));
        it = verdict.emplace(c->device, std::make_pair(bad, bad_offset)).first;
    }
    if (it->second.first)
        return vct_fail(c, VCT_ERR_DEVICE, "this device's typed-buffer loads do not convert UNORM8 to exactly c / 255 (" +
                        std::to_string(it->second.first) + " of 4096 channel values differ)");
    const char* ld = getenv("VCT_LEVEL_DESCRIPTORS");
    c->chain_form = vct_chain_form_fits(cfg->voxel_dim) && it->second.second == 0 && !(ld && ld[0] == '1');
    c->err.clear();
    return VCT_OK;
}

}  // namespace

int vct_fail(vct_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

hipError_t VctFrameSlot::alloc_half_rate(int w, int h) {
    const size_t npix = (size_t)w * h, nquad = (size_t)((w + 1) / 2) * ((h + 1) / 2);
    hipError_t e = dr_ind.alloc(npix);
    if (e == hipSuccess) e = dr_coarse.alloc(nquad);
    if (e == hipSuccess) e = dr_anchor.alloc(nquad);
    if (e == hipSuccess) e = dr_list.alloc(npix);
    if (e == hipSuccess) e = dr_ctr.alloc(VCT_DR_CTR_WORDS);
    if (e == hipSuccess) e = hipMemsetAsync(dr_ind.get(), 0, npix * sizeof(float4), stream.get());
    if (e == hipSuccess) e = hipMemsetAsync(dr_coarse.get(), 0, nquad * sizeof(float4), stream.get());
    if (e == hipSuccess) e = hipMemsetAsync(dr_anchor.get(), 0xff, nquad, stream.get());
    if (e == hipSuccess) e = hipMemsetAsync(dr_list.get(), 0, npix * sizeof(uint32_t), stream.get());
    if (e == hipSuccess) e = hipMemsetAsync(dr_ctr.get(), 0, VCT_DR_CTR_WORDS * sizeof(unsigned long long), stream.get());
    for (VctEvent& ev : dr_ev)
        if (e == hipSuccess && !ev) e = ev.create();
    if (e != hipSuccess) free_half_rate();
    return e;
}

// A new stream that demonstrably runs beside `base`: candidates are created until one overlaps (the rejected ones stay
// alive during the search so that the runtime hands out other hardware queues), at most 8; if none does, the last
// candidate is returned with *overlaps = false (correct all the same, nothing gained).  VCT_STREAM_PROBE=0: the first
// stream the runtime hands out, unprobed (A/B runs).
int vct_create_overlapping_stream(vct_ctx* c, hipStream_t base, hipStream_t* out, bool* overlaps) {
    *out = nullptr;
    *overlaps = false;
    const char* pr = getenv("VCT_STREAM_PROBE");
    if (pr && pr[0] == '0') { HIP_TRY(c, hipStreamCreateWithFlags(out, hipStreamNonBlocking)); return VCT_OK; }
    VctStream rejected[8];      // (whatever is left in here goes with the scope)
    int nrej = 0;
    while (nrej < 8) {
        VctStream cand;
        const hipError_t e = cand.create(hipStreamNonBlocking);
        if (e != hipSuccess) return vct_fail(c, VCT_ERR_DEVICE, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e));
        PIPE_TRY(streams_overlap(c, base, cand.get(), overlaps));
        if (*overlaps) { *out = cand.release(); return VCT_OK; }
        rejected[nrej++] = std::move(cand);
    }
    *out = rejected[nrej - 1].release();
    return VCT_OK;
}

int vct_pipeline_join(vct_ctx* c) {
    if (c->frames_in_flight < 2) return VCT_OK;
    VctSlotOrder& x = c->xslot;
    x.note_producer();
    if (x.joined) return VCT_OK;      // (vct_ctx.h: nothing new can be on the other stream)
    HIP_TRY(c, hipEventRecord(x.ev.get(), other(c).stream.get()));
    HIP_TRY(c, hipStreamWaitEvent(cur(c).stream.get(), x.ev.get(), 0));
    x.joined = true;
    return VCT_OK;
}
int vct_pipeline_drain(vct_ctx* c) {
    if (c->frames_in_flight < 2) return VCT_OK;
    VctSlotOrder& x = c->xslot;
    x.note_producer();
    if (x.drained) return VCT_OK;
    HIP_TRY(c, hipStreamSynchronize(other(c).stream.get()));
    x.drained = x.joined = true;      // (a finished stream needs no GPU-side wait either)
    return VCT_OK;
}

int vct_staging_free(vct_ctx* c) {
    if (c->frames_in_flight > 1) HIP_TRY(c, hipStreamSynchronize(other(c).stream.get()));
    return VCT_OK;
}

int vct_timer_ms(vct_ctx* c, const VctTimer& t, float* ms, const char* never, const char* untimed) {
    hipError_t e = hipSuccess;
    switch (t.elapsed(ms, &e)) {
        case VctTimer::NEVER: return vct_fail(c, VCT_ERR_INVALID, never);
        case VctTimer::UNTIMED: return vct_fail(c, VCT_ERR_INVALID, untimed);
        case VctTimer::FAILED: return vct_fail(c, VCT_ERR_DEVICE, std::string("timing events: ") + hipGetErrorString(e));
        default: return VCT_OK;
    }
}

VctRulesInForce vct_rules_in_force(const vct_ctx* c) {
    VctRulesInForce r = {0u, 0u};
    if (c->show_mask != VCT_SHOW_ALL) r.features |= VCT_FEAT_MASK;
    if (c->aov_which) r.features |= VCT_FEAT_AOV;
    if (c->diffuse_rate == 2) r.features |= VCT_FEAT_RATE2;
    if (c->slots[0].emis || c->slots[1].emis) r.features |= VCT_FEAT_EMISSION;
    if (c->gloss.n) r.features |= VCT_FEAT_GLOSS;
    if (c->sky.attached) r.features |= VCT_FEAT_SKY;
    if (c->lights.n) r.features |= VCT_FEAT_LIGHTS;
    if (c->frames_in_flight > 1) r.features |= VCT_FEAT_TWO_FRAMES;
    if (c->cfg.trace_variant != 0) r.modes |= VCT_MODE_VARIANT;
    if (c->cfg.anisotropic_mips) r.modes |= VCT_MODE_ANISO;
    if (c->vol.want_cells) r.modes |= VCT_MODE_CELLS;
    if (c->comm) r.modes |= VCT_MODE_COMM;
    if (c->cfg.debug_outputs) r.modes |= VCT_MODE_DEBUG;
    if (c->cfg.trace_variant == 4) r.modes |= VCT_MODE_VARIANT4;
#if defined(VCT_STATS) && VCT_STATS
    r.modes |= VCT_MODE_STATS;
#endif
    return r;
}

int vct_refuse_conflict(vct_ctx* c, const char* who, unsigned features, unsigned modes) {
    const VctConflict hit = vct_rule_conflict(features, modes);
    if (!hit) return VCT_OK;
    const VctRuleText& f = kVctFeatureText[vct_rule_bit_index(hit.feature)];
    const VctRuleText& m = kVctModeText[vct_rule_bit_index(hit.mode)];
    std::string msg = std::string(who) + ": " + f.name + " and " + m.name + " do not go together (" + f.lift;
    if (m.lift) msg += std::string(", or ") + m.lift;
    return vct_fail(c, VCT_ERR_INVALID, msg + " lifts it)");
}

hipError_t vct_create_masked_stream(hipStream_t* s, int device, int first_cu, int last_cu) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return e;
    const int ncu = prop.multiProcessorCount;
    std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
    for (int cu = first_cu < 0 ? 0 : first_cu; cu < last_cu && cu < ncu; ++cu) mask[(size_t)cu / 32] |= 1u << (cu % 32);
    return hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data());
}
extern "C" {

int vct_default_config(vct_config* cfg) {
    if (!cfg) return VCT_ERR_INVALID;
    memset(cfg, 0, sizeof(*cfg));
    cfg->abi_version = VCT_ABI_VERSION;
    cfg->device = -1;
    cfg->voxel_dim = 128;            // VCT.h:16
    cfg->grid_world_size = 150.0f;   // VCT.h:17
    cfg->width = 1280;               // VCT.h:24
    cfg->height = 720;               // VCT.h:25
    cfg->shadow_map_size = 4096;     // VCT.h:35
    cfg->model_scale = 0.05f;        // VCT.h:183
    cfg->ambient_factor = 0.1f;      // VCT.h:53
    cfg->shininess = 20.0f;          // Mesh.h:86
    cfg->max_distance = 75.0f;       // trace.fs:43
    cfg->max_alpha = 0.95f;          // trace.fs:44
    cfg->tan_diffuse = 0.577f;       // trace.fs:198
    cfg->tan_specular = 0.07f;       // trace.fs:218
    cfg->wrap_repeat = 1;
    cfg->texture_mipmaps = 1;        // Model.h:168,172: glGenerateMipmap + LINEAR_MIPMAP_LINEAR
    return VCT_OK;
}

size_t vct_chain_texels(int32_t V) {
    return is_pow2(V) ? (size_t)vct_level_offset(V, vct_ilog2(V) + 1) : 0;
}

int vct_create(const vct_config* cfg, vct_ctx** out) {
    if (!cfg || !out) return vct_fail(nullptr, VCT_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->abi_version != VCT_ABI_VERSION) return vct_fail(nullptr, VCT_ERR_INVALID, "vct_config.abi_version mismatch");
    if (!is_pow2(cfg->voxel_dim) || cfg->voxel_dim < 8 || cfg->voxel_dim > VCT_MAX_VOXEL_DIM)
        return vct_fail(nullptr, VCT_ERR_INVALID, "voxel_dim must be a power of two in [8,1024]");
    if (cfg->width <= 0 || cfg->height <= 0 || !(cfg->grid_world_size > 0.0f))
        return vct_fail(nullptr, VCT_ERR_INVALID, "bad frame size or grid size");
    // the checks of the setters (vct_set_cone_apertures, vct_set_trace_variant) for the same fields
    if (!(cfg->tan_diffuse > 0.0f) || !(cfg->tan_specular > 0.0f)) return vct_fail(nullptr, VCT_ERR_INVALID, "aperture must be > 0");
    if (cfg->trace_variant < 0 || cfg->trace_variant > 4) return vct_fail(nullptr, VCT_ERR_INVALID, "trace_variant: 0 .. 4");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return vct_fail(nullptr, VCT_ERR_NO_DEVICE, "no HIP device: this library has no CPU path (MI355X / gfx950 required)");
    vct_ctx* c = new vct_ctx();
    c->cfg = *cfg;
    int dev = cfg->device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) { delete c; return vct_fail(nullptr, VCT_ERR_INVALID, "device ordinal out of range"); }
    c->device = dev;
    c->cfg.device = dev;
    const int rc = create_resources(c);
    if (rc) { const std::string m = c->err; vct_destroy(c); return vct_fail(nullptr, rc, m); }
    *out = c;
    return VCT_OK;
}

void vct_destroy(vct_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    vct_comm_release(c);
    // every stream that can still read a buffer is waited for before the context's members free their memory
    for (VctFrameSlot& s : c->slots)
        if (s.stream) (void)hipStreamSynchronize(s.stream.get());
    if (c->fork.aux) (void)hipStreamSynchronize(c->fork.aux.get());
    delete c;
}

const char* vct_last_error(const vct_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int vct_get_config(const vct_ctx* c, vct_config* cfg) {
    if (!c || !cfg) return VCT_ERR_INVALID;
    *cfg = c->cfg;
    return VCT_OK;
}

int vct_set_camera_position(vct_ctx* c, const float pos[3]) {
    if (!c || !pos) return VCT_ERR_INVALID;
    memcpy(c->cam, pos, 12);
    return VCT_OK;
}

int vct_set_light_direction(vct_ctx* c, const float dir[3]) {
    if (!c || !dir) return VCT_ERR_INVALID;
    memcpy(c->light, dir, 12);
    return VCT_OK;
}

int vct_set_ambient_factor(vct_ctx* c, float a) {
    if (!c) return VCT_ERR_INVALID;
    c->cfg.ambient_factor = a;
    return VCT_OK;
}

int vct_set_cone_apertures(vct_ctx* c, float td, float ts) {
    if (!c) return VCT_ERR_INVALID;
    if (!(td > 0.0f) || !(ts > 0.0f)) return vct_fail(c, VCT_ERR_INVALID, "aperture must be > 0");
    c->cfg.tan_diffuse = td;
    c->cfg.tan_specular = ts;
    c->steps_dirty = true;
    return VCT_OK;
}

int vct_set_trace_variant(vct_ctx* c, int32_t variant) {
    if (!c) return VCT_ERR_INVALID;
    if (variant < 0 || variant > 4) return vct_fail(c, VCT_ERR_INVALID, "vct_set_trace_variant: 0 .. 4");
    PIPE_TRY(vct_refuse_conflict(c, "vct_set_trace_variant", vct_rules_in_force(c).features,
                                 (variant != 0 ? VCT_MODE_VARIANT : 0u) | (variant == 4 ? VCT_MODE_VARIANT4 : 0u)));
    c->cfg.trace_variant = variant;
    return VCT_OK;
}

int vct_synchronize(vct_ctx* c) {
    if (!c) return VCT_ERR_INVALID;
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    if (c->frames_in_flight > 1) HIP_TRY(c, hipStreamSynchronize(other(c).stream.get()));      // every frame in flight
    return VCT_OK;
}

// ---- two frames in flight (vct_ctx.h VctFrameSlot) ---------------------------------------------------------------------
int vct_set_frames_in_flight(vct_ctx* c, int32_t n) {
    if (!c) return VCT_ERR_INVALID;
    if (n != 1 && n != 2) return vct_fail(c, VCT_ERR_INVALID, "vct_set_frames_in_flight: 1 or 2");
    if (n == c->frames_in_flight) return VCT_OK;
    if (n == 2) PIPE_TRY(vct_refuse_conflict(c, "vct_set_frames_in_flight", VCT_FEAT_TWO_FRAMES, vct_rules_in_force(c).modes));
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->comm) PIPE_TRY(vct_comm_sync(c));      // (deadline-bounded: a frame step in flight may wait for a peer)
    PIPE_TRY(vct_synchronize(c));
    if (n == 1) {
        // back to one frame: slot 0 selected first, then slot 1 released with its raster scratch
        c->cur_slot = 0;
        slot_release(c->slots[1]);
        c->frames_in_flight = 1;
        c->xslot.reset();
        return VCT_OK;
    }
    // a second slot: its own stream, timing events, G-buffer, frame and per-tile step counts (190 MB + 17 MB at 1080p)
    // on a stream that demonstrably runs beside the context's stream (create_overlapping_stream)
    hipStream_t stream = nullptr;
    PIPE_TRY(vct_create_overlapping_stream(c, c->slots[0].stream.get(), &stream, &c->xslot.streams_overlap));
    hipError_t e = slot_create(c, c->slots[1], stream);
    if (e == hipSuccess && !c->xslot.ev) e = c->xslot.ev.create(hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        slot_release(c->slots[1]);
        return vct_fail(c, e == hipErrorOutOfMemory ? VCT_ERR_NOMEM : VCT_ERR_DEVICE, std::string("vct_set_frames_in_flight: ") + hipGetErrorString(e));
    }
    c->frames_in_flight = 2;
    c->xslot.reset();
    return VCT_OK;
}

int vct_get_frames_in_flight(const vct_ctx* c, int32_t* n, int32_t* selected, int32_t* streams_overlap_out) {
    if (!c) return VCT_ERR_INVALID;
    if (n) *n = c->frames_in_flight;
    if (selected) *selected = c->cur_slot;
    if (streams_overlap_out) *streams_overlap_out = (c->frames_in_flight > 1 && c->xslot.streams_overlap) ? 1 : 0;
    return VCT_OK;
}

int vct_select_frame_slot(vct_ctx* c, int32_t slot) {
    if (!c) return VCT_ERR_INVALID;
    if (slot < 0 || slot >= c->frames_in_flight)
        return vct_fail(c, VCT_ERR_INVALID, "vct_select_frame_slot: slot outside [0, frames in flight)");
    if (slot == c->cur_slot) return VCT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    bool waited = false;
    if (c->xslot.produced) {      // shared state was written on this slot's stream: the other stream's next work follows it
        HIP_TRY(c, hipEventRecord(c->xslot.ev.get(), cur(c).stream.get()));
        HIP_TRY(c, hipStreamWaitEvent(c->slots[slot].stream.get(), c->xslot.ev.get(), 0));
        c->xslot.produced = false;
        waited = true;
    }
    c->cur_slot = slot;
    // the stream left behind may hold work the next producer must follow -- unless the wait above already put the selected
    // stream behind all of it (the stream left behind receives nothing more until it is selected again)
    c->xslot.joined = waited;
    c->xslot.drained = false;
    return VCT_OK;
}

int vct_get_stream(vct_ctx* c, void** s) {
    if (!c || !s) return VCT_ERR_INVALID;
    *s = (void*)cur(c).stream.get();
    return VCT_OK;
}

// ---- lighting components (include/vct.h) -------------------------------------------------------------------------------
int vct_set_lighting_components(vct_ctx* c, uint32_t mask) {
    if (!c) return VCT_ERR_INVALID;
    if (mask & ~(uint32_t)VCT_SHOW_ALL) return vct_fail(c, VCT_ERR_INVALID, "vct_set_lighting_components: bits above VCT_SHOW_ALL");
    if (mask != VCT_SHOW_ALL) PIPE_TRY(vct_refuse_conflict(c, "vct_set_lighting_components", VCT_FEAT_MASK, vct_rules_in_force(c).modes));
    c->show_mask = mask;
    return VCT_OK;
}

int vct_get_lighting_components(const vct_ctx* c, uint32_t* mask) {
    if (!c || !mask) return VCT_ERR_INVALID;
    *mask = c->show_mask;
    return VCT_OK;
}

}  // extern "C"
