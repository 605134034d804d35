// vct_api_query.hip -- the C ABI's point queries: vct_gather_points, vct_cone_points, their counts and timing.
#include <hipcub/hipcub.hpp>

#include "vct_ctx.h"
#include "vct_query_check.h"

static_assert(sizeof(vct_gather_point) == 48 && sizeof(vct_cone_point) == 36, "point records are packed floats");
static_assert(VCT_QUERY_KIND_GATHER == VCT_QUERY_GATHER && VCT_QUERY_KIND_CONE == VCT_QUERY_CONE, "one numbering of the kinds");

namespace {

// The buffers of the slot's VctPointQuery a query of these sizes needs.  They only grow; growing frees the old buffer,
// which an earlier device-located query of this slot may still read or write, so the slot's stream is waited for first.
int reserve_buffers(vct_ctx* c, VctPointQuery& Q, const VctQuerySizes& sz, bool host, bool sort, size_t n, size_t sort_bytes) {
    const bool grow = !Q.ctr ||
                      (host && (sz.pts_floats > Q.pts.size() || sz.out_floats > Q.out.size() || sz.cones_floats > Q.out_cones.size() ||
                                sz.steps_bytes > Q.out_steps.size())) ||
                      (sort && (2 * n > Q.keys.size() || 2 * n > Q.index.size() || sort_bytes > Q.sort_tmp.size()));
    if (!grow) return VCT_OK;
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    if (!Q.ctr) HIP_TRY(c, Q.ctr.alloc(VCT_DR_COUNTERS));
    if (host) {
        HIP_TRY(c, Q.pts.reserve(sz.pts_floats));
        HIP_TRY(c, Q.out.reserve(sz.out_floats));
        HIP_TRY(c, Q.out_cones.reserve(sz.cones_floats));
        HIP_TRY(c, Q.out_steps.reserve(sz.steps_bytes));
    }
    if (sort) {
        HIP_TRY(c, Q.keys.reserve(2 * n));
        HIP_TRY(c, Q.index.reserve(2 * n));
        HIP_TRY(c, Q.sort_tmp.reserve(sort_bytes));
    }
    return VCT_OK;
}

int run_query(vct_ctx* c, const char* who, int kind, const void* pts, int32_t n, int32_t location, int32_t aperture, float* out,
              float* out_cones, uint8_t* out_steps, uint32_t flags) {
    if (!c) return VCT_ERR_INVALID;
    auto refuse = [&](const char* why) { return vct_fail(c, VCT_ERR_INVALID, std::string(who) + ": " + why); };
    // VCT_APERTURE_GLOSS(k), k < nclasses (include/vct.h "per-material gloss"): class k's step table in the specular
    // table's place -- wave-uniform as before, one query has one aperture.  From here on it counts as aperture 1.
    int gloss_class = -1;
    if (kind == VCT_QUERY_CONE && aperture >= 2) {
        if (aperture - 2 >= c->gloss.n) return refuse("aperture is neither 0 (diffuse), 1 (specular) nor VCT_APERTURE_GLOSS(k) of an attached class");
        gloss_class = aperture - 2;
        aperture = 1;
    }
    if (const char* why = vct_query_check_args(kind, pts, n, location, aperture, out, false, 0, flags)) return refuse(why);
    if (n > 0 && out_cones && ((uintptr_t)out_cones & 3u)) return refuse("points and outputs need 4-byte alignment");
    if (c->cfg.anisotropic_mips)
        return refuse("config.anisotropic_mips: point queries read the isotropic chain only (out of scope)");
    if (n == 0) return VCT_OK;
    if (!c->vol.mips_valid) return refuse("level 0 changed since the last vct_build_mips (call it first)");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_refresh_steps(c));
    const bool specular = kind == VCT_QUERY_CONE && aperture == 1;
    if (const char* why = vct_query_check_args(kind, pts, n, location, aperture, out, out_steps != nullptr,
                                               gloss_class >= 0 ? c->gloss.nsteps[gloss_class] : (specular ? c->n_specular : c->n_diffuse), flags))
        return refuse(why);

    VctPointQuery& Q = cur(c).query;
    hipStream_t s = cur(c).stream.get();
    const bool host = location == VCT_MEM_HOST, sort = (flags & VCT_QUERY_SORT_CELLS) != 0u;
    const VctQuerySizes sz = vct_query_sizes(kind, n, out_cones != nullptr, out_steps != nullptr);
    size_t sort_bytes = 0;
    if (sort)      // (a null temporary storage: the size query, nothing is launched)
        HIP_TRY(c, (hipcub::DeviceRadixSort::SortPairs<uint32_t, uint32_t>(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, 0,
                                                                           VCT_QUERY_KEY_BITS, s)));
    PIPE_TRY(reserve_buffers(c, Q, sz, host, sort, (size_t)n, sort_bytes));

    VctTraceParams p;
    vct_fill_march_params(c, p, c->vol.active());
    p.cells_biased = nullptr;      // same bits without the footprint records
    p.sky = c->sky.dev();          // sky light: the SKY forms of k_query_march (include/vct.h "sky light")
    if (gloss_class >= 0) { p.steps_specular = &c->gloss.table.get()->steps[gloss_class][0]; p.n_specular = c->gloss.nsteps[gloss_class]; }
    VctQueryArgs q;
    memset(&q, 0, sizeof(q));
    q.n = (uint32_t)n;
    q.specular = specular ? 1 : 0;
    q.ctr = Q.ctr.get();
    if (host) {
        HIP_TRY(c, hipMemcpyAsync(Q.pts.get(), pts, sz.pts_floats * sizeof(float), hipMemcpyHostToDevice, s));
        q.pts = Q.pts.get();
        q.out = Q.out.get();
        q.out_cones = out_cones ? Q.out_cones.get() : nullptr;
        q.out_steps = out_steps ? Q.out_steps.get() : nullptr;
    } else {
        q.pts = (const float*)pts;
        q.out = out;
        q.out_cones = out_cones;
        q.out_steps = out_steps;
    }
    HIP_TRY(c, hipMemsetAsync(Q.ctr.get(), 0, VCT_DR_COUNTERS * sizeof(unsigned long long), s));
    if (sort) {
        // (key, index) pairs, sorted by key into the second half of each buffer; the radix sort is stable, so points with
        // equal keys keep the caller's order
        uint32_t* keys = Q.keys.get();
        uint32_t* index = Q.index.get();
        HIP_TRY(c, vct_launch_query_keys(p, q, kind, keys, index, s));
        size_t bytes = Q.sort_tmp.size();
        HIP_TRY(c, (hipcub::DeviceRadixSort::SortPairs<uint32_t, uint32_t>(Q.sort_tmp.get(), bytes, keys, keys + n, index, index + n, n, 0,
                                                                           VCT_QUERY_KEY_BITS, s)));
        q.index = index + n;
    }
    HIP_TRY(c, Q.timer.begin(s, c->time_traces));
    HIP_TRY(c, vct_launch_query(p, q, kind, s));
    HIP_TRY(c, Q.timer.end(s));
    c->last_march_form = c->fast_div ? 2 : 1;
    Q.sorted = sort;
    Q.n = (uint64_t)n;
    Q.kind = kind;
    if (host) {
        HIP_TRY(c, hipMemcpyAsync(out, Q.out.get(), sz.out_floats * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out_cones) HIP_TRY(c, hipMemcpyAsync(out_cones, Q.out_cones.get(), sz.cones_floats * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out_steps) HIP_TRY(c, hipMemcpyAsync(out_steps, Q.out_steps.get(), sz.steps_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    return VCT_OK;
}

}  // namespace

extern "C" {

int vct_gather_points(vct_ctx* c, const vct_gather_point* pts, int32_t n, int32_t location, float* out_gather, float* out_cones,
                      uint8_t* out_steps, uint32_t flags) {
    return run_query(c, "vct_gather_points", VCT_QUERY_GATHER, pts, n, location, 0, out_gather, out_cones, out_steps, flags);
}

int vct_cone_points(vct_ctx* c, const vct_cone_point* pts, int32_t n, int32_t location, int32_t aperture, float* out_cone,
                    uint8_t* out_steps, uint32_t flags) {
    return run_query(c, "vct_cone_points", VCT_QUERY_CONE, pts, n, location, aperture, out_cone, nullptr, out_steps, flags);
}

int vct_last_point_query(vct_ctx* c, uint64_t out[4]) {
    if (!c || !out) return VCT_ERR_INVALID;
    const VctPointQuery& Q = cur(c).query;
    if (!Q.timer.have) return vct_fail(c, VCT_ERR_INVALID, "vct_last_point_query: no point query has run on this frame slot");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(cur(c).stream.get()));
    unsigned long long v[VCT_DR_COUNTERS];
    HIP_TRY(c, hipMemcpy(v, Q.ctr.get(), sizeof(v), hipMemcpyDeviceToHost));
    uint64_t sum = 0;
    for (unsigned long long w : v) sum += w;
    out[0] = Q.n;
    out[1] = sum;
    out[2] = (uint64_t)Q.kind;
    out[3] = Q.sorted ? 1u : 0u;
    return VCT_OK;
}

int vct_last_point_query_ms(vct_ctx* c, float* ms) {
    if (!c || !ms) return VCT_ERR_INVALID;
    return vct_timer_ms(c, cur(c).query.timer, ms, "vct_last_point_query_ms: no point query has run on this frame slot",
                        "vct_last_point_query_ms: the last query was issued with timing off (vct_set_trace_timing)");
}

}  // extern "C"
