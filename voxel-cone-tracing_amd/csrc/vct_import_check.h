// vct_import_check.h -- the descriptor check of vct_import_gbuffer (vct_api_import.hip), the element sizes of its input
// formats and the per-pixel arithmetic of include/vct.h "G-buffer import" (decode, position, tangent frame, colours),
// free of any HIP call so that a host program can run them under the sanitizers (tests/import_check_main.cpp).
// k_gbuffer_import (vct_raster.hip) calls vct_import_pixel itself: one copy of the arithmetic, host and device.
// Build with -ffp-contract=off: every multiply, add and compare below happens in the written order.
#ifndef VCT_IMPORT_CHECK_H_
#define VCT_IMPORT_CHECK_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vct.h"

#if defined(__HIPCC__)
#define VCT_IMPORT_FN __host__ __device__ __forceinline__
#else
#define VCT_IMPORT_FN static inline
#endif

#define VCT_IMPORT_FLAGS_ALL (VCT_IMPORT_FLIP_Y | VCT_IMPORT_DEPTH_ZERO_TO_ONE | VCT_IMPORT_OPAQUE)
#define VCT_IMPORT_NPLANES 23

// verdicts of vct_import_check_desc: 0, or which rule of the header's list the descriptor breaks
enum {
    VCT_IMPORT_OK = 0,
    VCT_IMPORT_BAD_NULL,              // in, or a required pointer (position, normal, albedo)
    VCT_IMPORT_BAD_FORMAT,            // a format outside its enum (specular_format counts only with a specular buffer)
    VCT_IMPORT_BAD_LOCATION,
    VCT_IMPORT_BAD_FLAGS,             // a bit outside VCT_IMPORT_FLAGS_ALL
    VCT_IMPORT_BAD_MATRIX,            // DEPTH_F32 and a non-finite element of inv_view_proj
    VCT_IMPORT_BAD_NORMAL_SCALE,      // not finite, or <= 0
    VCT_IMPORT_BAD_SPECULAR_CONSTANT, // no specular buffer and a non-finite constant
    VCT_IMPORT_BAD_ROWS               // tile rows outside [0, tile_rows], or row0 > row1
};

VCT_IMPORT_FN bool vct_import_finite(float v) { return v == v && v - v == 0.0f; }

// bytes of one element; 0: unknown format
VCT_IMPORT_FN size_t vct_import_position_bytes(int32_t f) {
    return f == VCT_IMPORT_POSITION_F32X3 ? 12 : (f == VCT_IMPORT_POSITION_F32X4 ? 16 : (f == VCT_IMPORT_DEPTH_F32 ? 4 : 0));
}
VCT_IMPORT_FN size_t vct_import_normal_bytes(int32_t f) {
    return f == VCT_IMPORT_NORMAL_F32X3 ? 12 : (f == VCT_IMPORT_NORMAL_F16X4 ? 8 : (f == VCT_IMPORT_NORMAL_OCT_SNORM16X2 ? 4 : 0));
}
VCT_IMPORT_FN size_t vct_import_color_bytes(int32_t f) {
    return f == VCT_IMPORT_COLOR_UNORM8X4 ? 4 : (f == VCT_IMPORT_COLOR_F16X4 ? 8 : (f == VCT_IMPORT_COLOR_F32X4 ? 16 : 0));
}
// bytes of a tightly packed w x h input of `elem`-byte elements (w, h <= 2^15 each by the config check: no overflow)
VCT_IMPORT_FN size_t vct_import_buffer_bytes(size_t elem, int32_t w, int32_t h) { return elem * (size_t)w * (size_t)h; }

// Everything vct_import_gbuffer refuses before it touches anything; tile_rows = ceil(height / 8).
VCT_IMPORT_FN int vct_import_check_desc(const vct_gbuffer_import* in, int32_t tile_rows, int32_t row0, int32_t row1) {
    if (!in || !in->position || !in->normal || !in->albedo) return VCT_IMPORT_BAD_NULL;
    if (!vct_import_position_bytes(in->position_format) || !vct_import_normal_bytes(in->normal_format) ||
        !vct_import_color_bytes(in->albedo_format) || (in->specular && !vct_import_color_bytes(in->specular_format)))
        return VCT_IMPORT_BAD_FORMAT;
    if (in->location != VCT_MEM_HOST && in->location != VCT_MEM_DEVICE) return VCT_IMPORT_BAD_LOCATION;
    if (in->flags & ~VCT_IMPORT_FLAGS_ALL) return VCT_IMPORT_BAD_FLAGS;
    if (in->position_format == VCT_IMPORT_DEPTH_F32)
        for (int i = 0; i < 16; ++i)
            if (!vct_import_finite(in->inv_view_proj[i])) return VCT_IMPORT_BAD_MATRIX;
    if (!vct_import_finite(in->normal_scale) || !(in->normal_scale > 0.0f)) return VCT_IMPORT_BAD_NORMAL_SCALE;
    if (!in->specular)
        for (int i = 0; i < 3; ++i)
            if (!vct_import_finite(in->specular_constant[i])) return VCT_IMPORT_BAD_SPECULAR_CONSTANT;
    if (row0 < 0 || row1 > tile_rows || row0 > row1) return VCT_IMPORT_BAD_ROWS;
    return VCT_IMPORT_OK;
}

// ---- decode ----
// Inputs need the alignment of their scalar only, so wider elements are read through packed types (memcpy semantics).
struct __attribute__((packed, aligned(4))) VctImportF3 { float v[3]; };
struct __attribute__((packed, aligned(4))) VctImportF4 { float v[4]; };
struct __attribute__((packed, aligned(2))) VctImportH4 { uint16_t v[4]; };
struct __attribute__((packed, aligned(2))) VctImportS2 { int16_t v[2]; };

VCT_IMPORT_FN float vct_import_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// IEEE binary16 -> binary32, exact: every half value (subnormals, infinities, NaN payloads) has one fp32 image
VCT_IMPORT_FN float vct_import_half(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    if (e == 0x1fu) return vct_import_bits(sign | 0x7f800000u | (m << 13));
    if (e != 0u) return vct_import_bits(sign | ((e + 112u) << 23) | (m << 13));
    // zero or subnormal: m * 2^-24, exact in fp32 (m < 2^10; the product only changes the exponent)
    const float v = (float)m * 5.9604644775390625e-08f;
    return sign ? -v : v;
}
VCT_IMPORT_FN float vct_import_snorm16(int16_t s) { return (float)(s < -32767 ? -32767 : (int)s) / 32767.0f; }

VCT_IMPORT_FN void vct_import_oct(float ex, float ey, float v[3]) {
    v[0] = ex; v[1] = ey; v[2] = (1.0f - fabsf(ex)) - fabsf(ey);
    if (v[2] < 0.0f) {
        v[0] = (1.0f - fabsf(ey)) * (ex >= 0.0f ? 1.0f : -1.0f);
        v[1] = (1.0f - fabsf(ex)) * (ey >= 0.0f ? 1.0f : -1.0f);
    }
}

// element e of a normal target, undecoded length
VCT_IMPORT_FN void vct_import_read_normal(const void* buf, int32_t fmt, size_t e, float v[3]) {
    if (fmt == VCT_IMPORT_NORMAL_F32X3) {
        const VctImportF3 r = ((const VctImportF3*)buf)[e];
        v[0] = r.v[0]; v[1] = r.v[1]; v[2] = r.v[2];
    } else if (fmt == VCT_IMPORT_NORMAL_F16X4) {
        const VctImportH4 r = ((const VctImportH4*)buf)[e];
        v[0] = vct_import_half(r.v[0]); v[1] = vct_import_half(r.v[1]); v[2] = vct_import_half(r.v[2]);
    } else {
        const VctImportS2 r = ((const VctImportS2*)buf)[e];
        vct_import_oct(vct_import_snorm16(r.v[0]), vct_import_snorm16(r.v[1]), v);
    }
}

// element e of a colour target as four floats
VCT_IMPORT_FN void vct_import_read_color(const void* buf, int32_t fmt, size_t e, float c[4]) {
    if (fmt == VCT_IMPORT_COLOR_UNORM8X4) {
        const uint32_t r = ((const uint32_t*)buf)[e];      // bytes r, g, b, a in memory order (little endian)
        for (int k = 0; k < 4; ++k) c[k] = (float)((r >> (8 * k)) & 0xffu) / 255.0f;
    } else if (fmt == VCT_IMPORT_COLOR_F16X4) {
        const VctImportH4 r = ((const VctImportH4*)buf)[e];
        for (int k = 0; k < 4; ++k) c[k] = vct_import_half(r.v[k]);
    } else {
        const VctImportF4 r = ((const VctImportF4*)buf)[e];
        for (int k = 0; k < 4; ++k) c[k] = r.v[k];
    }
}

// unit(v) of the header: the shade kernel's normalisation of the bump normal
VCT_IMPORT_FN void vct_import_unit(const float v[3], float out[3]) {
    const float l = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const float il = 1.0f / l;
    for (int k = 0; k < 3; ++k) out[k] = l > 0.0f ? v[k] * il : 0.0f;
}

// u = unit(n), then the tangent t and bitangent b of the header's construction (vcth_frame_from_normal's, in fp32)
VCT_IMPORT_FN void vct_import_frame(const float n[3], float u[3], float t[3], float b[3]) {
    vct_import_unit(n, u);
    const float ax = fabsf(u[0]), ay = fabsf(u[1]), az = fabsf(u[2]);
    float k[3];
    if (ay >= ax && ay >= az) { k[0] = 0.0f; k[1] = -u[2]; k[2] = u[1]; }
    else { k[0] = u[2]; k[1] = 0.0f; k[2] = -u[0]; }
    vct_import_unit(k, t);
    b[0] = u[1] * t[2] - u[2] * t[1];
    b[1] = u[2] * t[0] - u[0] * t[2];
    b[2] = u[0] * t[1] - u[1] * t[0];
}

// ---- corner normals of the dynamic mesh (include/vct.h "dynamic mesh", Normals) ----
// n' = C n with C the cofactor matrix of the top-left 3 x 3 of the row-major 3 x 4 matrix m: with A_r its rows,
// C_0 = A_1 x A_2, C_1 = A_2 x A_0, C_2 = A_0 x A_1, each component a * b - c * d in the face normal's component order,
// then n'_r = ((C_r.x * n.x + C_r.y * n.y) + C_r.z * n.z).  No division: cross(A a, A b) = C cross(a, b) for any A.
VCT_IMPORT_FN void vct_import_cofactor(const float m[12], float c[9]) {
    for (int r = 0; r < 3; ++r) {
        const float* a = m + 4 * ((r + 1) % 3);
        const float* b = m + 4 * ((r + 2) % 3);
        c[3 * r] = a[1] * b[2] - a[2] * b[1];
        c[3 * r + 1] = a[2] * b[0] - a[0] * b[2];
        c[3 * r + 2] = a[0] * b[1] - a[1] * b[0];
    }
}
VCT_IMPORT_FN void vct_import_cofactor_normal(const float c[9], const float n[3], float out[3]) {
    for (int r = 0; r < 3; ++r) out[r] = (c[3 * r] * n[0] + c[3 * r + 1] * n[1]) + c[3 * r + 2] * n[2];
}

// The frame of a corner with moved normal n' on a face with frame (uf, tf, bf): u = unit(n'), accepted where
// uf . u > 0 (NaN, zero, an overflowing length and a normal 90 degrees or more from the face all fail that one test);
// t = unit(tf - u * (u . tf)), the face's tangent re-orthogonalised, never a fresh axis choice per corner; b = u x t.
// Returns whether the corner took a frame of its own; false: (u, t, b) is the face frame.
VCT_IMPORT_FN bool vct_import_corner_frame(const float n[3], const float uf[3], const float tf[3], const float bf[3], float u[3],
                                           float t[3], float b[3]) {
    float uc[3], k[3], tc[3];
    vct_import_unit(n, uc);
    const float df = (uc[0] * uf[0] + uc[1] * uf[1]) + uc[2] * uf[2];
    bool own = df > 0.0f;
    const float d = (uc[0] * tf[0] + uc[1] * tf[1]) + uc[2] * tf[2];
    for (int i = 0; i < 3; ++i) k[i] = tf[i] - uc[i] * d;
    vct_import_unit(k, tc);
    own = own && !(tc[0] == 0.0f && tc[1] == 0.0f && tc[2] == 0.0f);
    for (int i = 0; i < 3; ++i) { u[i] = own ? uc[i] : uf[i]; t[i] = own ? tc[i] : tf[i]; }
    const float cb[3] = {uc[1] * tc[2] - uc[2] * tc[1], uc[2] * tc[0] - uc[0] * tc[2], uc[0] * tc[1] - uc[1] * tc[0]};
    for (int i = 0; i < 3; ++i) b[i] = own ? cb[i] : bf[i];
    return own;
}

// The 23 planes of frame pixel (x, y), row 0 at the bottom, of a w x h frame.  Returns whether the pixel has a surface
// (none: every plane is +0).  Plane 22 is the given shadow value, or 25 * 0.111f where the descriptor has none -- the
// kernel with a shadow map replaces that by the PCF value.
VCT_IMPORT_FN bool vct_import_pixel(const vct_gbuffer_import& d, int32_t w, int32_t h, int32_t x, int32_t y, float g[VCT_IMPORT_NPLANES]) {
    for (int k = 0; k < VCT_IMPORT_NPLANES; ++k) g[k] = 0.0f;
    const size_t e = (size_t)((d.flags & VCT_IMPORT_FLIP_Y) ? h - 1 - y : y) * (size_t)w + (size_t)x;
    float P[3];
    if (d.position_format == VCT_IMPORT_DEPTH_F32) {
        const float depth = ((const float*)d.position)[e];
        if (depth == d.depth_clear || depth != depth) return false;
        const float nx = (2.0f * ((float)x + 0.5f)) / (float)w - 1.0f;
        const float ny = (2.0f * ((float)y + 0.5f)) / (float)h - 1.0f;
        const float nz = (d.flags & VCT_IMPORT_DEPTH_ZERO_TO_ONE) ? depth : 2.0f * depth - 1.0f;
        const float* m = d.inv_view_proj;
        float r[4];
        for (int i = 0; i < 4; ++i) r[i] = ((m[i] * nx + m[4 + i] * ny) + m[8 + i] * nz) + m[12 + i];
        for (int i = 0; i < 3; ++i) P[i] = r[i] / r[3];
    } else if (d.position_format == VCT_IMPORT_POSITION_F32X4) {
        const VctImportF4 r = ((const VctImportF4*)d.position)[e];
        if (r.v[3] == 0.0f) return false;
        P[0] = r.v[0]; P[1] = r.v[1]; P[2] = r.v[2];
    } else {
        const VctImportF3 r = ((const VctImportF3*)d.position)[e];
        P[0] = r.v[0]; P[1] = r.v[1]; P[2] = r.v[2];
    }
    float n[3], u[3], t[3], b[3];
    vct_import_read_normal(d.normal, d.normal_format, e, n);
    vct_import_frame(n, u, t, b);
    for (int k = 0; k < 3; ++k) {
        g[k] = P[k];
        g[3 + k] = u[k] * d.normal_scale;
        g[6 + k] = t[k] * d.normal_scale;
        g[9 + k] = b[k] * d.normal_scale;
        g[12 + k] = u[k];
    }
    if (d.shading_normal) {
        float sn[3], su[3];
        vct_import_read_normal(d.shading_normal, d.normal_format, e, sn);
        vct_import_unit(sn, su);
        for (int k = 0; k < 3; ++k) g[12 + k] = su[k];
    }
    float c[4];
    vct_import_read_color(d.albedo, d.albedo_format, e, c);
    g[15] = c[0]; g[16] = c[1]; g[17] = c[2];
    g[18] = (d.flags & VCT_IMPORT_OPAQUE) ? 1.0f : c[3];
    if (d.specular) {
        vct_import_read_color(d.specular, d.specular_format, e, c);
        g[19] = c[0]; g[20] = c[1]; g[21] = c[2];
    } else {
        g[19] = d.specular_constant[0]; g[20] = d.specular_constant[1]; g[21] = d.specular_constant[2];
    }
    g[22] = d.shadow ? d.shadow[e] : 25.0f * 0.111f;
    return true;
}

#endif
