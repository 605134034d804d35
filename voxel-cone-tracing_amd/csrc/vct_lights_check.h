// vct_lights_check.h -- the table check of vct_set_lights (vct_api_lights.hip) and the folding of a light into what the
// device sees (include/vct.h "local lights"), free of any HIP call so that a host program can run them under the
// sanitizers.  Build with -ffp-contract=off.
#ifndef VCT_LIGHTS_CHECK_H_
#define VCT_LIGHTS_CHECK_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vct.h"

// One light as the kernels read it: 64 B, one scalar load of sixteen dwords at a wave-uniform index.
struct VctLightDev {
    float pos[3], R2;          // position; radius^2
    float color[3], S2;        // colour; source_radius^2
    float axis[3], cos_outer;  // unit(direction) (SPOT; zeros for a point light); cosine of the outer half angle
    float inv_cone;            // 1 / (cos_inner - cos_outer)
    uint32_t flags;
    float pad[2];
};

#define VCT_LIGHTS_OK 0
#define VCT_LIGHTS_BAD (-1)

static inline bool vct_light_finite(float v) { return v == v && !isinf(v); }

// why light `l` is refused, or NULL: it is inside the contract
static inline const char* vct_light_fault(const vct_light* l) {
    const float f[14] = {l->position[0], l->position[1], l->position[2], l->radius, l->color[0], l->color[1], l->color[2],
                         l->source_radius, l->direction[0], l->direction[1], l->direction[2], l->cos_outer, l->cos_inner, 0.0f};
    for (int i = 0; i < 13; ++i)
        if (!vct_light_finite(f[i])) return "a field is not finite";
    if (l->flags & ~(uint32_t)VCT_LIGHT_SPOT) return "unknown flag bits";
    if (!(l->radius > 0.0f)) return "radius <= 0";
    if (!(l->source_radius > 0.0f)) return "source_radius <= 0";
    if (l->color[0] < 0.0f || l->color[1] < 0.0f || l->color[2] < 0.0f) return "a negative colour";
    if (l->flags & VCT_LIGHT_SPOT) {
        const float len = sqrtf((l->direction[0] * l->direction[0] + l->direction[1] * l->direction[1]) + l->direction[2] * l->direction[2]);
        if (!(len > 0.0f) || !vct_light_finite(len)) return "a spot's axis has zero or non-finite length";
        if (!(-1.0f <= l->cos_outer && l->cos_outer < l->cos_inner && l->cos_inner <= 1.0f)) return "a spot needs -1 <= cos_outer < cos_inner <= 1";
    }
    return NULL;
}

// lights: [n].  VCT_LIGHTS_BAD: *bad_index names the first light outside the contract and *why says how
static inline int vct_lights_check(const vct_light* lights, int32_t n, int32_t* bad_index, const char** why) {
    for (int32_t i = 0; i < n; ++i) {
        const char* w = vct_light_fault(&lights[i]);
        if (w) {
            if (bad_index) *bad_index = i;
            if (why) *why = w;
            return VCT_LIGHTS_BAD;
        }
    }
    return VCT_LIGHTS_OK;
}

// a checked light -> the device's form
static inline void vct_light_fold(const vct_light* l, VctLightDev* d) {
    for (int k = 0; k < 3; ++k) { d->pos[k] = l->position[k]; d->color[k] = l->color[k]; d->axis[k] = 0.0f; }
    d->R2 = l->radius * l->radius;
    d->S2 = l->source_radius * l->source_radius;
    d->cos_outer = 0.0f;
    d->inv_cone = 0.0f;
    d->flags = l->flags;
    d->pad[0] = d->pad[1] = 0.0f;
    if (l->flags & VCT_LIGHT_SPOT) {
        const float* v = l->direction;
        const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);      // the import's unit(v)
        const float r = 1.0f / len;
        for (int k = 0; k < 3; ++k) d->axis[k] = len > 0.0f ? v[k] * r : 0.0f;
        d->cos_outer = l->cos_outer;
        d->inv_cone = 1.0f / (l->cos_inner - l->cos_outer);
    }
}

#endif
