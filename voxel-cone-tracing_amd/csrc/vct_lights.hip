// vct_lights.hip -- local lights (include/vct.h "local lights"): point and spot lights added to radiance level 0 and to
// the frame's lit planes.  Two kernels, neither of which any march or composite kernel knows about:
//   k_light_voxels  behind vct_inject_light's resolve, one wave per 8^3 brick of the voxelizer's slots: the direct
//                   diffuse term of every light into the texels of the occupied voxels, in place;
//   k_light_pixels  in front of every launch that composites a G-buffer, one wave per 8x8 tile, lane = pixel: the
//                   direct diffuse and specular terms (+ the slot's pixel-emission planes) into the lit planes, which
//                   that launch takes as its pixel-emission planes.
// Both read the folded light table (vct_lights_check.h VctLightDev, 64 B per light) through the constant address space
// at wave-uniform indices -- one scalar load of sixteen dwords per light, as the march reads its step table -- and skip
// a light wave-uniformly when it reaches nothing of the brick / tile: an unreached point's term is exactly +0, and
// x + (+0) = x for every sum that started from +0 and has only taken non-negative or NaN terms, so the bits are those
// of the plain loop over all lights.
// The arithmetic is the header's, operation for operation: plain fp32 operators under -ffp-contract=off (nothing fused),
// IEEE divide and square root, fmaxf / fminf as maxNum / minNum.  tests/lights_ref.py restates it in numpy.
#include "../../include/vct.h"
#include "vct_internal.h"
#include "vct_lights_check.h"

namespace {

typedef const __attribute__((address_space(4))) VctLightDev* LightTable;

struct Light {      // one table entry in scalar registers
    float px, py, pz, R2, cr, cg, cb, S2, ax, ay, az, cos_outer, inv_cone;
    uint32_t flags;
};
__device__ __forceinline__ Light load_light(LightTable t, int j) {
    Light L;
    L.px = t[j].pos[0]; L.py = t[j].pos[1]; L.pz = t[j].pos[2]; L.R2 = t[j].R2;
    L.cr = t[j].color[0]; L.cg = t[j].color[1]; L.cb = t[j].color[2]; L.S2 = t[j].S2;
    L.ax = t[j].axis[0]; L.ay = t[j].axis[1]; L.az = t[j].axis[2]; L.cos_outer = t[j].cos_outer;
    L.inv_cone = t[j].inv_cone; L.flags = t[j].flags;
    return L;
}

struct V3 { float x, y, z; };
__device__ __forceinline__ float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// IEEE-correct divide and square root (hipcc's default; the __fsqrt_rn intrinsic is the 1-ulp native one)
__device__ __forceinline__ float sqrt_rn(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ V3 normalize3(V3 a) {
    const float l = sqrt_rn(dot3(a, a));
    return {a.x / l, a.y / l, a.z / l};
}

// d = position - P, r2 = dot(d, d); returns `in`
__device__ __forceinline__ bool light_reach(const Light& L, V3 P, V3& d, float& r2) {
    d = {L.px - P.x, L.py - P.y, L.pz - P.z};
    r2 = dot3(d, d);
    return r2 < L.R2;
}
// l and att * spot of a light whose d and r2 are known
__device__ __forceinline__ float light_term(const Light& L, V3 d, float r2, V3& l) {
    const float len = sqrt_rn(r2);
    l = {d.x / len, d.y / len, d.z / len};
    const float q = r2 / L.R2;
    const float w = fmaxf(1.0f - q * q, 0.0f);
    const float att = (w * w) / fmaxf(r2, L.S2);
    float spot = 1.0f;
    if (L.flags & VCT_LIGHT_SPOT) {      // wave-uniform
        const float c = dot3(V3{L.ax, L.ay, L.az}, l) * -1.0f;
        const float t = fminf(fmaxf((c - L.cos_outer) * L.inv_cone, 0.0f), 1.0f);
        spot = t * t;
    }
    return att * spot;
}

// Smallest |p - x| the subtraction p - x can return for x in [lo, hi] (lo <= hi): fl(p - x) does not increase with x, so
// every such difference lies in [fl(p - hi), fl(p - lo)].
__device__ __forceinline__ float axis_gap(float p, float lo, float hi) {
    const float a = p - hi, b = p - lo;
    return a > 0.0f ? a : (b < 0.0f ? b * -1.0f : 0.0f);
}

// centre of voxel i along one axis, as vct_bounce forms it
__device__ __forceinline__ float voxel_centre(int i, float fV, float G) { return (((float)i + 0.5f) / fV - 0.5f) * G; }

#define VCT_LIGHT_WAVES 4

__global__ void __launch_bounds__(64 * VCT_LIGHT_WAVES)
k_light_voxels(const VctLightVoxArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * VCT_LIGHT_WAVES;
    const LightTable tab = (LightTable)a.lights;
    const float fV = (float)a.V;
    for (uint32_t sl = blockIdx.x * VCT_LIGHT_WAVES + wave; sl < a.nslots; sl += nwaves) {
        const uint32_t b = a.slot_brick[sl];
        if (a.brick_prev[b] == 0u) continue;        // the resolve wrote nothing of this pass here
        // The cull, lane j for light j.  The brick's voxel centres lie in the box [lo, hi] of its first and last voxel
        // (voxel_centre does not decrease with i).  With g the per-axis gaps, r2_min = (gx*gx + gy*gy) + gz*gz in the
        // same operation order is <= the r2 of every voxel of the brick (each rounded operation is monotonic in the
        // magnitudes it takes), so r2_min < R2 false proves `in` false for the whole brick.
        const int bx = (int)vct_compact3(b) * 8, by = (int)vct_compact3(b >> 1) * 8, bz = (int)vct_compact3(b >> 2) * 8;
        bool reach = false;
        if (lane < a.nlights) {
            const VctLightDev* L = a.lights + lane;
            const float gx = axis_gap(L->pos[0], voxel_centre(bx, fV, a.G), voxel_centre(bx + 7, fV, a.G));
            const float gy = axis_gap(L->pos[1], voxel_centre(by, fV, a.G), voxel_centre(by + 7, fV, a.G));
            const float gz = axis_gap(L->pos[2], voxel_centre(bz, fV, a.G), voxel_centre(bz + 7, fV, a.G));
            reach = (gx * gx + gy * gy) + gz * gz < L->R2;
        }
        const unsigned long long reached = __builtin_amdgcn_ballot_w64(reach);
        if (reached == 0ull) continue;              // no light reaches the brick: nothing of it is read
        const size_t pool = (size_t)sl * 512;
        uint32_t* __restrict__ l0 = a.level0 + (size_t)b * 512;
        for (uint32_t it = 0; it < 8u; ++it) {
            const uint32_t v = it * 64u + (uint32_t)lane;
            const uint32_t aq = a.attr_albedo[pool + v];
            const bool occ = (aq >> 24) == 255u;
            if (__builtin_amdgcn_ballot_w64(occ) == 0ull) continue;
            const uint32_t nq = a.attr_normal[pool + v], src = l0[v];
            const uint32_t mi = b * 512u + v;       // the voxel's Morton index (V <= 1024: below 2^30)
            const V3 P = {voxel_centre((int)vct_compact3(mi), fV, a.G), voxel_centre((int)vct_compact3(mi >> 1), fV, a.G),
                          voxel_centre((int)vct_compact3(mi >> 2), fV, a.G)};
            const V3 n = normalize3(V3{(float)((int)(nq & 0xffu) - 128), (float)((int)((nq >> 8) & 0xffu) - 128),
                                       (float)((int)((nq >> 16) & 0xffu) - 128)});
            float sr = 0.0f, sg = 0.0f, sb = 0.0f;
            for (unsigned long long m = reached; m != 0ull; m &= m - 1ull) {
                const Light L = load_light(tab, __ffsll((long long)m) - 1);
                V3 d, l;
                float r2;
                const bool in = light_reach(L, P, d, r2);
                const float as = light_term(L, d, r2, l);
                const float nl = fmaxf(dot3(n, l), 0.0f);
                const float k = in ? as * nl : 0.0f;
                sr = sr + L.cr * k; sg = sg + L.cg * k; sb = sb + L.cb * k;
            }
            if (occ) {
                const uint32_t r = vct_float_to_unorm8(vct_unorm8_to_float(src & 0xffu) + vct_unorm8_to_float(aq & 0xffu) * sr);
                const uint32_t g = vct_float_to_unorm8(vct_unorm8_to_float((src >> 8) & 0xffu) + vct_unorm8_to_float((aq >> 8) & 0xffu) * sg);
                const uint32_t bl = vct_float_to_unorm8(vct_unorm8_to_float((src >> 16) & 0xffu) + vct_unorm8_to_float((aq >> 16) & 0xffu) * sb);
                l0[v] = r | (g << 8) | (bl << 16) | (src & 0xff000000u);
            }
        }
    }
}

__global__ void __launch_bounds__(64 * VCT_LIGHT_WAVES)
k_light_pixels(const VctLightPixArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ntiles = (a.row1 - a.row0) * a.tiles_x;
    const int ti = (int)blockIdx.x * VCT_LIGHT_WAVES + wave;
    if (ti >= ntiles) return;
    const int tile = a.row0 * a.tiles_x + ti;       // frame-wide tile index: the tiled buffers' own order
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x = tx * VCT_TILE + (lane & 7), y = ty * VCT_TILE + (lane >> 3);
    const float* __restrict__ gb = a.gbuf + (size_t)tile * (VCT_GB_NPLANES * VCT_TILE_PIX) + lane;
    const bool live = x < a.width && y < a.height && !(gb[18 * VCT_TILE_PIX] < 0.5f);      // the composite's discard
    const V3 P = {gb[0], gb[VCT_TILE_PIX], gb[2 * VCT_TILE_PIX]};
    const V3 N = {gb[12 * VCT_TILE_PIX], gb[13 * VCT_TILE_PIX], gb[14 * VCT_TILE_PIX]};
    const float alb_r = gb[15 * VCT_TILE_PIX], alb_g = gb[16 * VCT_TILE_PIX], alb_b = gb[17 * VCT_TILE_PIX];
    const float spc_r = gb[19 * VCT_TILE_PIX], spc_g = gb[20 * VCT_TILE_PIX], spc_b = gb[21 * VCT_TILE_PIX];
    const V3 Ev = normalize3(V3{a.cam[0] - P.x, a.cam[1] - P.y, a.cam[2] - P.z});
    float shin = a.shininess;
    if (a.pix_gloss) {      // the lane's class under the gloss plane's clamp rule: never an index before the clamp
        const int byte = (int)a.pix_gloss[(size_t)tile * VCT_TILE_PIX + lane];
        const int cls = byte < a.nclasses ? byte : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) shin = cls == k ? a.class_shininess[k] : shin;
    }
    const LightTable tab = (LightTable)a.lights;
    // (A first cull of the table against the box of the tile's live positions, as k_light_voxels culls against its brick,
    // was measured and left out: 0.156 -> 0.143 ms with 64 lights on the atrium at 1080p, nothing below that -- a tile's
    // pixels span too much of the scene for the box to drop many lights, and the time is the terms of those that reach.)
    float dr = 0.0f, dg = 0.0f, db = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
    for (int j = 0; j < a.nlights; ++j) {
        const Light L = load_light(tab, j);
        V3 d, l;
        float r2;
        const bool in = light_reach(L, P, d, r2);
        if (__builtin_amdgcn_ballot_w64(in && live) == 0ull) continue;      // no live pixel in range: +0 to every sum
        const float as = light_term(L, d, r2, l);
        const float ndl = dot3(N, l);
        const float kd = in ? as * fmaxf(ndl, 0.0f) : 0.0f;
        dr = dr + L.cr * kd; dg = dg + L.cg * kd; db = db + L.cb * kd;
        const float two_ndl = 2.0f * ndl;
        const V3 R = {two_ndl * N.x - l.x, two_ndl * N.y - l.y, two_ndl * N.z - l.z};
        const float sp = powf(fmaxf(dot3(Ev, R), 0.0f), shin);
        const float ks = in ? as * sp : 0.0f;
        sr = sr + L.cr * ks; sg = sg + L.cg * ks; sb = sb + L.cb * ks;
    }
    const bool s_dd = (a.show & VCT_SHOW_DIFFUSE) != 0u, s_ds = (a.show & VCT_SHOW_SPECULAR) != 0u;
    float o0 = (s_dd ? dr * alb_r : 0.0f) + (s_ds ? sr * spc_r : 0.0f);
    float o1 = (s_dd ? dg * alb_g : 0.0f) + (s_ds ? sg * spc_g : 0.0f);
    float o2 = (s_dd ? db * alb_b : 0.0f) + (s_ds ? sb * spc_b : 0.0f);
    const size_t off = (size_t)tile * (VCT_EMIS_NPLANES * VCT_TILE_PIX) + lane;
    if (a.emis) {
        const float* __restrict__ em = a.emis + off;
        o0 = em[0] + o0; o1 = em[VCT_TILE_PIX] + o1; o2 = em[2 * VCT_TILE_PIX] + o2;
    }
    float* __restrict__ out = a.lit + off;
    out[0] = live ? o0 : 0.0f;
    out[VCT_TILE_PIX] = live ? o1 : 0.0f;
    out[2 * VCT_TILE_PIX] = live ? o2 : 0.0f;
}

}  // namespace

hipError_t vct_launch_light_voxels(const VctLightVoxArgs& a, hipStream_t s) {
    if (a.nslots == 0u || a.nlights <= 0) return hipSuccess;
    const uint32_t blocks = (a.nslots + VCT_LIGHT_WAVES - 1u) / VCT_LIGHT_WAVES;
    hipLaunchKernelGGL(k_light_voxels, dim3(blocks < 8192u ? blocks : 8192u), dim3(64 * VCT_LIGHT_WAVES), 0, s, a);
    return hipGetLastError();
}

hipError_t vct_launch_light_pixels(const VctLightPixArgs& a, hipStream_t s) {
    const int ntiles = (a.row1 - a.row0) * a.tiles_x;
    if (ntiles <= 0 || a.nlights <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_light_pixels, dim3((ntiles + VCT_LIGHT_WAVES - 1) / VCT_LIGHT_WAVES), dim3(64 * VCT_LIGHT_WAVES), 0, s, a);
    return hipGetLastError();
}
