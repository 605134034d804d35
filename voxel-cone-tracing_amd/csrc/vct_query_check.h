// vct_query_check.h -- argument checks and buffer-size arithmetic of the point queries (vct_api_query.hip), free of any
// HIP call so that a host program can run them under the sanitizers (tests/point_query_check_main.cpp).
#ifndef VCT_QUERY_CHECK_H_
#define VCT_QUERY_CHECK_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/vct.h"

#define VCT_QUERY_KIND_GATHER 0
#define VCT_QUERY_KIND_CONE 1

// What is wrong with the arguments of vct_gather_points / vct_cone_points, or null.  `out`: out_gather / out_cone.
// nsteps: march steps of the aperture's table (step counts travel as uint8).
static inline const char* vct_query_check_args(int kind, const void* pts, int32_t n, int32_t location, int32_t aperture,
                                               const void* out, bool want_steps, int nsteps, uint32_t flags) {
    if (n < 0) return "n < 0";
    if (n > VCT_POINT_QUERY_MAX) return "n > VCT_POINT_QUERY_MAX";
    if (location != VCT_MEM_HOST && location != VCT_MEM_DEVICE) return "location is neither VCT_MEM_HOST nor VCT_MEM_DEVICE";
    if (kind == VCT_QUERY_KIND_CONE && aperture != 0 && aperture != 1) return "aperture is neither 0 (diffuse) nor 1 (specular)";
    if (flags & ~(uint32_t)VCT_QUERY_SORT_CELLS) return "unknown flag bits";
    if (n > 0 && !pts) return "null points";
    if (n > 0 && !out) return "null output";
    if (n > 0 && (((uintptr_t)pts | (uintptr_t)out) & 3u)) return "points and outputs need 4-byte alignment";
    if (n > 0 && want_steps && nsteps > 255) return "step counts are uint8: this aperture needs more than 255 steps";
    return nullptr;
}

// element counts of the buffers of a query of n points (0 where an output is not wanted)
struct VctQuerySizes {
    size_t pts_floats, out_floats, cones_floats, steps_bytes;
};
static inline VctQuerySizes vct_query_sizes(int kind, int32_t n, bool want_cones, bool want_steps) {
    VctQuerySizes s;
    const size_t m = n > 0 ? (size_t)n : 0;
    const bool gather = kind == VCT_QUERY_KIND_GATHER;
    s.pts_floats = m * (gather ? sizeof(vct_gather_point) : sizeof(vct_cone_point)) / sizeof(float);
    s.out_floats = m * 4;
    s.cones_floats = gather && want_cones ? m * 24 : 0;
    s.steps_bytes = want_steps ? m * (gather ? 6 : 1) : 0;
    return s;
}

// workgroups (one wave each) of the march over n points: one per 64 points, at most `cap`
static inline uint32_t vct_query_items(uint32_t n) { return (n + 63u) >> 6; }

#endif
