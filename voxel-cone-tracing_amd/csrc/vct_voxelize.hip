// vct_voxelize.hip -- triangle voxelization + light injection into level 0 of the brick chain.
//
// Replaces the reference's voxelization draw (VCT.h:213-245): S/Voxelization.vs:15-22 (world
// position, shadow coordinate), S/Voxelization.gs:22-51 (dominant axis), S/Voxelization.fs:18-89
// (PCF, voxel index, imageStore of albedo*shadow).  fp32 operation order mirrors the scalar oracle
// (compile with -ffp-contract=off).  Two modes:
//
// North-star mode: conservative triangle / voxel-box overlap (Schwarz & Seidel 2010) instead of pixel-centre raster,
// and the exact, order-independent rounded mean of the fragments of a voxel instead of the racy last-writer imageStore.
//   plan      Which voxels a triangle overlaps depends only on geometry, V and G, so the fragment list is built ONCE when
//             the triangles are uploaded (k_vox_plan / k_vox_plan_big: entries (triangle, Morton voxel)).
//   sort      Counting sort of the list by 8^3 brick; every brick the mesh can touch gets a SLOT (k_frag_mark,
//             k_assign_slots, k_frag_count, k_frag_scatter, k_slot_bricks).
//   constants What a fragment contributes apart from the light -- its barycentrics on its triangle and its albedo (the
//             mip-mapped diffuse fetch of vox.fs:56; scenes with textures only) -- is stored per sorted fragment
//             (k_frag_geom), and the quantised face normals per triangle (k_tri_nrm).
//   LDS pass  A voxelize pass -- e.g. after the light moved -- is one workgroup per work item = up to VCT_VOX_CHUNK
//             fragments of one slot (k_voxelize_bricks): its threads read their fragments' stored values, transform the
//             triangle's vertices by the light matrix, run the 25-tap PCF and add unorm8(albedo * shadow) into the
//             brick's 512 accumulators IN LDS (64-bit ds_add of sumR|sumG, sumB|count); the same workgroup resolves the
//             rounded means and writes the brick's 2 KiB of texels into the slot's place in a STAGING pool -- coalesced,
//             once, no global atomics.  Only the chunks of a slot above VCT_VOX_CHUNK meet in HBM accumulators, resolved
//             by k_vox_resolve_multi.  All fragments of a brick lie within 8 voxels of each other, so their 25-tap shadow
//             windows overlap: coherent fetches.
//   resolve   vct_inject_light's sparse resolve (k_resolve_sparse) copies the staged slots of touched bricks into level 0
//             and clears bricks that are no longer covered: vct_voxelize evaluates the light, vct_inject_light makes it
//             visible.
// Reference mode: the shaders as written (k_voxelize_reference*), last writer by atomicMax into per-slot words in HBM,
// unpacked by the same sparse resolve.
//
// Both modes share the triangle front end (load_world_tri, shadow_coords, dominant_axis), the material (material_colour,
// load_material, interp_uv, quad_duv, frag_albedo) and the fragment value (shadow_factor, lit_rgb8): DESIGN.md 3.2.
#include <type_traits>

#include "vct_internal.h"

namespace {

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 sub3(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot3(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ F3 cross3(F3 a, F3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float comp(F3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }

__device__ __forceinline__ F3 xform_point(const float* m, F3 p) {
    return {m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12],
            m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
            m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]};
}

// [GL] bilinear, clamp-to-edge depth fetch (VCT.h:93-96)
__device__ __forceinline__ float shadow_tex(const uint32_t* __restrict__ words, uint32_t eb, int S, float u, float v) {
    const float fS = (float)S;
    const float x = u * fS - 0.5f, y = v * fS - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    const float a = x - fx, b = y - fy;
    const float top = (float)(S - 1);
    auto cl = [&](float f) -> int {
        if (!(f > 0.0f)) return 0;
        if (f >= top) return S - 1;
        return (int)f;
    };
    const int i0 = cl(fx), i1 = cl(fx + 1.0f), j0 = cl(fy), j1 = cl(fy + 1.0f);
    const float d00 = vct_shadow_depth(words[(size_t)j0 * S + i0], eb), d10 = vct_shadow_depth(words[(size_t)j0 * S + i1], eb);
    const float d01 = vct_shadow_depth(words[(size_t)j1 * S + i0], eb), d11 = vct_shadow_depth(words[(size_t)j1 * S + i1], eb);
    const float a0 = 1.0f - a, b0 = 1.0f - b;
    float acc = (a0 * b0) * d00;
    acc = fmaf(a * b0, d10, acc);
    acc = fmaf(a0 * b, d01, acc);
    acc = fmaf(a * b, d11, acc);
    return acc;
}

// One axis of the 5 PCF taps (offsets -2..2): floor of the texel coordinate and filter fraction, each computed exactly
// as shadow_tex() does for that tap.
struct TapAxis { float f[5], a[5]; };
__device__ __forceinline__ void tap_axis(float coord, float inv, float fS, TapAxis& t) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float u = coord + inv * (float)(k - 2);
        const float x = u * fS - 0.5f;
        t.f[k] = floorf(x);
        t.a[k] = x - t.f[k];
    }
}
// The window of the five taps of an axis is six CONSECUTIVE, UNCLAMPED texels when the floors step by exactly one
// (fp rounding at a texel boundary can make them step by 0 or 2) and the first / last lie inside the map: then
// shadow_tex()'s clamped indices are (int)f[k] and (int)f[k] + 1 for every tap -- without computing the ten clamped
// conversions of each axis (round 4: ~85 of the PCF's instructions).
__device__ __forceinline__ bool tap_axis_regular(const TapAxis& t, float top) {
    bool ok = t.f[0] >= 0.0f && t.f[4] + 1.0f <= top;
#pragma unroll
    for (int k = 0; k < 4; ++k) ok = ok && t.f[k + 1] == t.f[k] + 1.0f;
    return ok;
}

// vox.fs:18-52 (count of passing taps; caller divides by 25).  The 25 bilinear taps sit one texel
// apart, so they normally share a 6x6 texel window: when that window is six consecutive unclamped texels on both axes
// (checked per lane) it is loaded once (6 x 2 wide loads instead of 100 single ones) and each tap is evaluated from
// registers with its own exact weights; lanes whose window is irregular (fp rounding at a texel boundary, the rim of
// the map) take the tap-by-tap path.  Same bits either way.  (A clamped window used to have a path of its own -- 36
// single loads, i.e. 72 address registers, which set the register peak of the whole voxelize kernel: 158 VGPRs, 3 waves
// per SIMD, for a case only the rim of the map ever sees.)
__device__ __forceinline__ int pcf25(const uint32_t* __restrict__ words, uint32_t eb, int S, F3 c, float bias,
                                     const uint2* __restrict__ tiles = nullptr) {
    const float inv = __fdiv_rn(1.0f, (float)S);
    const float fS = (float)S, top = (float)(S - 1);
    TapAxis X, Y;
    tap_axis(c.x, inv, fS, X);
    tap_axis(c.y, inv, fS, Y);
    const float cur = c.z - bias;
    int count = 0;
    if (tap_axis_regular(X, top) && tap_axis_regular(Y, top)) {
        const uint32_t row0 = (uint32_t)(int)Y.f[0];
        const uint32_t col0 = (uint32_t)(int)X.f[0];
        // Round 5: first the depth bounds of the map tile the window starts in (ONE 8-byte load from a table the fragments of
        // a brick share, instead of twelve wide unaligned ones): a fragment away from every shadow boundary never fetches
        // a window.
        if (tiles) {
            const int v = vct_pcf_tile_verdict(tiles, S, col0, row0, cur);
            if (v >= 0) return v;
        }
        // One pass over the window: decode in place and take the smallest / largest decoded word on the way (the decode is
        // monotonic, so these are the window's depth bounds: vct_internal.h "PCF short cut").  A window the shadow boundary
        // does not cross ends here; the others evaluate the 25 taps from the same registers.  (The first form of the short
        // cut took the bounds on the raw words and loaded the window a second time: one more round trip in a kernel that
        // waits on memory two thirds of its time.)
        float d[6][6];
        uint32_t wmin = 0xffffffffu, wmax = 0u;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const VctWords6 w = *reinterpret_cast<const VctWords6*>(words + ((row0 + (uint32_t)j) * (uint32_t)S + col0));
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const uint32_t v = min(w.v[i] - eb, VCT_SHADOW_ONE);      // = vct_shadow_depth()
                d[j][i] = __uint_as_float(v);
                wmin = min(wmin, v); wmax = max(wmax, v);
            }
        }
        {
            const float lo = __uint_as_float(wmin) * 0.999998f, hi = __uint_as_float(wmax) * 1.000002f;
            if (cur <= lo) return 25;
            if (cur > hi) return 0;
        }
#pragma unroll
        for (int x = 0; x < 5; ++x)
#pragma unroll
            for (int y = 0; y < 5; ++y) {
                const float a = X.a[x], b = Y.a[y];
                const float a0 = 1.0f - a, b0 = 1.0f - b;
                float acc = (a0 * b0) * d[y][x];
                acc = fmaf(a * b0, d[y][x + 1], acc);
                acc = fmaf(a0 * b, d[y + 1][x], acc);
                acc = fmaf(a * b, d[y + 1][x + 1], acc);
                if (cur <= acc) ++count;
            }
    } else {
        for (int x = -2; x <= 2; ++x)
            for (int y = -2; y <= 2; ++y) {
                const float ox = inv * (float)x, oy = inv * (float)y;
                const float closest = shadow_tex(words, eb, S, c.x + ox, c.y + oy);
                if (cur <= closest) ++count;
            }
    }
    return count;
}

// vox.fs:46: the PCF factor of a fragment with barycentrics (b0, b1, b2) on a triangle whose vertices have the shadow
// coordinates dc; 1 without a shadow map
__device__ __forceinline__ float shadow_factor(const VctVoxParams& p, const F3 dc[3], float b0, float b1, float b2) {
    if (!p.shadow) return 1.0f;
    const F3 c = {b0 * dc[0].x + b1 * dc[1].x + b2 * dc[2].x,
                  b0 * dc[0].y + b1 * dc[1].y + b2 * dc[2].y,
                  b0 * dc[0].z + b1 * dc[1].z + b2 * dc[2].z};
    return __fdiv_rn((float)pcf25(p.shadow, p.shadow_ebase, p.shadow_size, c, 0.002f, p.shadow_tiles), 25.0f);
}
// vox.fs:88: unorm8(albedo * shadow), a channel per word
struct Rgb8 { uint32_t r, g, b; };
__device__ __forceinline__ Rgb8 lit_rgb8(const float alb[3], float sh) {
    return {vct_float_to_unorm8(alb[0] * sh), vct_float_to_unorm8(alb[1] * sh), vct_float_to_unorm8(alb[2] * sh)};
}

// ---- the triangle front end of both modes -------------------------------------------------------------------------
// vox.vs:21: world-space vertices (the record as three wide loads, not nine)
__device__ __forceinline__ void load_world_tri(const VctVoxParams& p, int t, F3 w[3]) {
    const VctTri9 rec = *reinterpret_cast<const VctTri9*>(p.pos + (size_t)t * 9);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* q = rec.v + 3 * k;
        w[k] = {q[0] * p.model_scale, q[1] * p.model_scale, q[2] * p.model_scale};
    }
}
// vox.vs:18-19: the vertices in the light's clip space, as shadow-map coordinates
__device__ __forceinline__ void shadow_coords(const VctVoxParams& p, const F3 w[3], F3 dc[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const F3 d = xform_point(p.light_vp, w[k]);
        dc[k] = {d.x * 0.5f + 0.5f, d.y * 0.5f + 0.5f, d.z * 0.5f + 0.5f};
    }
}
// vox.gs:24-39: 1 / 2 / 3 = the face normal is longest along x / y / z
__device__ __forceinline__ int dominant_axis(const F3 w[3]) {
    const F3 e1 = sub3(w[0], w[1]), e2 = sub3(w[2], w[0]);
    const F3 nn = cross3(e1, e2);
    const float len = __builtin_sqrtf(dot3(nn, nn));
    const float nx = fabsf(__fdiv_rn(nn.x, len)), ny = fabsf(__fdiv_rn(nn.y, len)),
                nz = fabsf(__fdiv_rn(nn.z, len));
    if (nx >= ny && nx >= nz) return 1;
    if (ny >= nx && ny >= nz) return 2;
    return 3;
}

// What a fragment's albedo comes from: the material's colour, or its diffuse texture at the triangle's coordinates
struct TriMaterial {
    float alb[3];
    float uv[3][2];     // TexCoord per vertex (vox.vs:17)
    int tex;            // diffuse texture of the triangle's material or -1 (flat colour)
};
__device__ __forceinline__ void material_colour(const VctVoxParams& p, int t, float alb[3]) {
    const float* c = p.albedo + 4 * (size_t)p.material[t];
    alb[0] = c[0]; alb[1] = c[1]; alb[2] = c[2];
}
__device__ __forceinline__ void load_material(const VctVoxParams& p, int t, TriMaterial& r) {
    material_colour(p, t, r.alb);
    r.tex = vct_tex_of(p.tex, p.material[t], 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.uv[k][0] = r.tex >= 0 ? p.tex.uv[(size_t)t * 6 + 2 * k] : 0.0f;
        r.uv[k][1] = r.tex >= 0 ? p.tex.uv[(size_t)t * 6 + 2 * k + 1] : 0.0f;
    }
}
// the texture coordinate at barycentrics (c0, c1, c2)
struct UV { float u, v; };
__device__ __forceinline__ UV interp_uv(const TriMaterial& r, float c0, float c1, float c2) {
    return {c0 * r.uv[0][0] + c1 * r.uv[1][0] + c2 * r.uv[2][0], c0 * r.uv[0][1] + c1 * r.uv[1][1] + c2 * r.uv[2][1]};
}
// texture() derivatives: the differences of the coordinate between the fragment (m) and its neighbours along the two
// raster axes (x, y), on this triangle (mip-mapped textures; oracle/vct_oracle.h vcto_scene)
__device__ __forceinline__ void quad_duv(UV m, UV x, UV y, float duv[4]) {
    duv[0] = x.u - m.u; duv[1] = x.v - m.v; duv[2] = y.u - m.u; duv[3] = y.v - m.v;
}
// vox.fs:56: the fragment's albedo -- texture(DiffuseTexture, uv) with uv interpolated by the fragment's
// barycentrics, or the flat material colour when the material has no diffuse texture
__device__ __forceinline__ void frag_albedo(const VctVoxParams& p, const TriMaterial& r, float b0, float b1, float b2,
                                            const float duv[4], float alb[3]) {
    alb[0] = r.alb[0]; alb[1] = r.alb[1]; alb[2] = r.alb[2];
    if (r.tex >= 0) {
        const UV q = interp_uv(r, b0, b1, b2);
        const float4 c = vct_tex_sample_lod(p.tex, r.tex, q.u, q.v, duv[0], duv[1], duv[2], duv[3]);
        alb[0] = c.x; alb[1] = c.y; alb[2] = c.z;
    }
}

struct TriSetup : TriMaterial {
    F3 g[3];     // voxel-space vertices
    F3 dc[3];    // shadow coordinates
    F3 n;
    float d1, d2;
    float ne[3][3][2];
    float de[3][3];
    int lo[3], hi[3];
    int ua, ub;
    float area;         // twice the signed area of the in-plane triangle
    bool valid;
};
// the vertices in the plane the triangle is projected to (perpendicular to its dominant axis)
struct InPlane { float x[3], y[3]; };
__device__ __forceinline__ InPlane in_plane(const TriSetup& r) {
    return {{comp(r.g[0], r.ua), comp(r.g[1], r.ua), comp(r.g[2], r.ua)},
            {comp(r.g[0], r.ub), comp(r.g[1], r.ub), comp(r.g[2], r.ub)}};
}

__device__ __forceinline__ void setup_tri(const VctVoxParams& p, int t, TriSetup& r) {
    F3 w[3];
    const float fV = (float)p.V;
    load_world_tri(p, t, w);
    shadow_coords(p, w, r.dc);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        r.g[k] = {(__fdiv_rn(w[k].x, p.G) + 0.5f) * fV, (__fdiv_rn(w[k].y, p.G) + 0.5f) * fV,
                  (__fdiv_rn(w[k].z, p.G) + 0.5f) * fV};
    const int axis = dominant_axis(w);

    const F3 e[3] = {sub3(r.g[1], r.g[0]), sub3(r.g[2], r.g[1]), sub3(r.g[0], r.g[2])};
    r.n = cross3(e[0], e[1]);
    r.valid = !((r.n.x == 0.0f && r.n.y == 0.0f && r.n.z == 0.0f) || r.n.x != r.n.x ||
                r.n.y != r.n.y || r.n.z != r.n.z);
    const F3 cp = {r.n.x > 0.0f ? 1.0f : 0.0f, r.n.y > 0.0f ? 1.0f : 0.0f, r.n.z > 0.0f ? 1.0f : 0.0f};
    r.d1 = dot3(r.n, sub3(cp, r.g[0]));
    r.d2 = dot3(r.n, sub3(sub3(F3{1.0f, 1.0f, 1.0f}, cp), r.g[0]));
    const float nsel[3] = {r.n.z, r.n.x, r.n.y};
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const int a0 = pl, a1 = (pl + 1) % 3;    // xy, yz, zx
        const float sg = nsel[pl] >= 0.0f ? 1.0f : -1.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float ea = comp(e[i], a0), eb = comp(e[i], a1);
            const float na = -eb * sg, nb = ea * sg;
            r.ne[pl][i][0] = na;
            r.ne[pl][i][1] = nb;
            const float va = comp(r.g[i], a0), vb = comp(r.g[i], a1);
            r.de[pl][i] = -(na * va + nb * vb) + fmaxf(0.0f, na) + fmaxf(0.0f, nb);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float mn = fminf(fminf(comp(r.g[0], a), comp(r.g[1], a)), comp(r.g[2], a));
        const float mx = fmaxf(fmaxf(comp(r.g[0], a), comp(r.g[1], a)), comp(r.g[2], a));
        r.lo[a] = max((int)floorf(mn), 0);
        r.hi[a] = min((int)floorf(mx), p.V - 1);
    }
    r.ua = axis == 1 ? 1 : 0;
    r.ub = axis == 3 ? 1 : 2;
    const InPlane a = in_plane(r);
    r.area = (a.x[1] - a.x[0]) * (a.y[2] - a.y[0]) - (a.x[2] - a.x[0]) * (a.y[1] - a.y[0]);
    load_material(p, t, r);
}

__device__ __forceinline__ bool overlap(const TriSetup& c, int i, int j, int k) {
    const F3 pp = {(float)i, (float)j, (float)k};
    const float np = dot3(c.n, pp);
    if ((np + c.d1) * (np + c.d2) > 0.0f) return false;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const float pa = comp(pp, pl), pb = comp(pp, (pl + 1) % 3);
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (c.ne[pl][e][0] * pa + c.ne[pl][e][1] * pb + c.de[pl][e] < 0.0f) return false;
    }
    return true;
}

// the centre of voxel (i, j, k) in that plane
struct PlanePoint { float x, y; };
__device__ __forceinline__ PlanePoint voxel_centre(const TriSetup& r, int i, int j, int k) {
    const F3 ctr = {(float)i + 0.5f, (float)j + 0.5f, (float)k + 0.5f};
    return {comp(ctr, r.ua), comp(ctr, r.ub)};
}
// (no reference code for this mode) the UNCLAMPED barycentrics of in-plane point q, from area cross products
__device__ __forceinline__ void area_bary(const TriSetup& r, PlanePoint q, float& c0, float& c1) {
    const InPlane a = in_plane(r);
    c0 = __fdiv_rn((a.x[1] - q.x) * (a.y[2] - q.y) - (a.x[2] - q.x) * (a.y[1] - q.y), r.area);
    c1 = __fdiv_rn((a.x[2] - q.x) * (a.y[0] - q.y) - (a.x[0] - q.x) * (a.y[2] - q.y), r.area);
}
// The barycentrics of the conservative fragment of triangle set-up `r` at voxel (i, j, k) (vox.fs has none: the oracle's
// north-star mode evaluates the triangle at the voxel centre projected along the dominant axis, clamped into the
// triangle), and -- for mip-mapped textures -- the differences of the texture coordinate one voxel further along each
// in-plane axis.  Pure geometry (triangle, V, G, texture coordinates): evaluated ONCE per mesh by k_frag_geom and stored
// per fragment; the voxelize pass reads them back (round 4: the pass used to re-derive the whole triangle set-up --
// nine IEEE divisions, the dominant axis, the in-plane area -- for every fragment, ~300 of its ~1,200 instructions).
__device__ __forceinline__ void frag_bary(const TriSetup& r, int i, int j, int k, float& b0, float& b1) {
    area_bary(r, voxel_centre(r, i, j, k), b0, b1);
    b0 = fminf(fmaxf(b0, 0.0f), 1.0f);
    b1 = fminf(fmaxf(b1, 0.0f), 1.0f);
    const float sum = b0 + b1;
    if (sum > 1.0f) { b0 = __fdiv_rn(b0, sum); b1 = __fdiv_rn(b1, sum); }
}
__device__ __forceinline__ void frag_duv(const TriSetup& r, int i, int j, int k, float duv[4]) {
    const PlanePoint c = voxel_centre(r, i, j, k);
    auto uv_at = [&](float qx, float qy) {
        float c0, c1;
        area_bary(r, {qx, qy}, c0, c1);
        return interp_uv(r, c0, c1, 1.0f - c0 - c1);
    };
    quad_duv(uv_at(c.x, c.y), uv_at(c.x + 1.0f, c.y), uv_at(c.x, c.y + 1.0f), duv);
}

// What a voxelize pass still needs of a fragment's triangle: the shadow coordinates of its vertices (they follow the
// light) and, in a scene without textures, the material's colour (FALB = false; with textures every fragment's albedo
// comes from frag_alb).
struct PassTri {
    F3 dc[3];
    float alb[3];
    uint32_t nrm[3];    // biased quantised face normal (voxel attributes)
};
template <bool ATTR, bool FALB>
__device__ __forceinline__ void setup_pass(const VctVoxParams& p, int t, PassTri& r) {
    if (p.shadow) {       // (the positions are not touched without a shadow map)
        F3 w[3];
        load_world_tri(p, t, w);
        shadow_coords(p, w, r.dc);
    }
    if (!FALB) material_colour(p, t, r.alb);
    if (ATTR) {
#pragma unroll
        for (int k = 0; k < 3; ++k) r.nrm[k] = p.tri_qnrm[(size_t)t * 3 + k];
    }
}

// One conservative fragment of triangle `r` with barycentrics (b0, b1) and albedo alb: the vox.fs:88 value
// unorm8(albedo * PCF / 25) and, for the second bounce, the fragment's albedo (unorm8) -- vox.fs:18-56.
struct FragValue { Rgb8 lit, alb; };
__device__ __forceinline__ FragValue frag_eval(const VctVoxParams& p, const PassTri& r, float b0, float b1, const float alb[3]) {
    const float b2 = fmaxf(1.0f - b0 - b1, 0.0f);
    const float sh = shadow_factor(p, r.dc, b0, b1, b2);
    return {lit_rgb8(alb, sh), lit_rgb8(alb, 1.0f)};       // (x * 1.0f is x, bit for bit)
}

__device__ __forceinline__ uint32_t resolve_voxel(ulonglong2 a) {
    const uint32_t c = (uint32_t)(a.y >> 32);
    if (!c) return 0u;
    const uint32_t h = c >> 1;
    const uint32_t r = ((uint32_t)a.x + h) / c, g = ((uint32_t)(a.x >> 32) + h) / c,
                   b = ((uint32_t)a.y + h) / c;
    return r | (g << 8) | (b << 16) | 0xff000000u;      // vox.fs:88: a = 1
}

#define VCT_VOX_BIG 4096

__device__ __forceinline__ long long tri_candidates(const TriSetup& r) {
    if (!r.valid) return 0;
    const int nx = r.hi[0] - r.lo[0] + 1, ny = r.hi[1] - r.lo[1] + 1, nz = r.hi[2] - r.lo[2] + 1;
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    return (long long)nx * ny * nz;
}

// Builds the fragment list: one entry (triangle, Morton index of the voxel) per voxel a triangle OVERLAPS.  The overlap
// test is pure geometry (triangle, V, G), so it runs here, once per uploaded mesh, and a voxelize pass spends its threads
// on fragments only.  (Round 2 listed every voxel of the clipped bounding box and tested in the pass: fine for the
// wall-and-floor atrium, but an oblique triangle overlaps a thin diagonal slice of its box -- the Bistro-class street's
// randomly oriented foliage cards at 1024^3: 753 M candidates for ~1/5 as many fragments.)  WRITE = false: only totals
// (plan[0] = fragments of the small triangles, plan[1] = big triangles, listed in big_list: bounding box > VCT_VOX_BIG
// voxels, enumerated by a workgroup each, k_vox_plan_big); WRITE = true: the entries.  Entry order is
// irrelevant (integer accumulation), so workgroups claim ranges with one atomic each.
template <class F>
__device__ __forceinline__ void for_each_overlap(const TriSetup& r, F f) {      // f(i, j, k) per overlapped voxel of the box
    for (int k = r.lo[2]; k <= r.hi[2]; ++k)
        for (int j = r.lo[1]; j <= r.hi[1]; ++j)
            for (int i = r.lo[0]; i <= r.hi[0]; ++i)
                if (overlap(r, i, j, k)) f(i, j, k);
}
template <bool WRITE>
__global__ void __launch_bounds__(256)
k_vox_plan(const VctVoxParams p, uint32_t* plan, uint2* frags, int32_t* big_list) {
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t block_base;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t chunks = 0;
    bool big = false;
    TriSetup r;
    if (t < p.ntri) {
        setup_tri(p, t, r);
        const long long cnt = tri_candidates(r);
        if (cnt > VCT_VOX_BIG) big = true;
        else if (cnt > 0) for_each_overlap(r, [&](int, int, int) { ++chunks; });
    }
    // workgroup exclusive scan of `chunks`
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = chunks;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) wave_base += wave_tot[w];
        total += wave_tot[w];
    }
    if (threadIdx.x == 0) {
        block_base = total ? atomicAdd(&plan[0], total) : 0u;
        if (block_base + total < block_base) plan[3] = 1u;      // the 32-bit counter wrapped: the caller rejects the mesh
    }
    __syncthreads();
    if (big && !WRITE) big_list[atomicAdd(&plan[1], 1u)] = t;      // (capacity ntri: the count pass lists them)
    if (WRITE && chunks) {
        uint32_t at = block_base + wave_base + incl - chunks;
        for_each_overlap(r, [&](int i, int j, int k) {
            frags[at++] = make_uint2((uint32_t)t, vct_morton3((uint32_t)i, (uint32_t)j, (uint32_t)k));
        });
    }
}

// fragments of the big triangles, one workgroup per triangle striding its bounding box.  WRITE = false: plan[2] += count;
// WRITE = true: entries appended at plan[2] (the caller starts it behind the small triangles' entries).
template <bool WRITE>
__global__ void __launch_bounds__(256)
k_vox_plan_big(const VctVoxParams p, const int32_t* __restrict__ big_list, int n_big, uint32_t* plan, uint2* frags) {
    const int lane = threadIdx.x & 63;
    for (int b = blockIdx.x; b < n_big; b += gridDim.x) {
        const int t = big_list[b];
        TriSetup r;
        setup_tri(p, t, r);
        const int nx = r.hi[0] - r.lo[0] + 1, ny = r.hi[1] - r.lo[1] + 1, nz = r.hi[2] - r.lo[2] + 1;
        const long long cnt = (long long)nx * ny * nz;
        for (long long v0 = 0; v0 < cnt; v0 += blockDim.x) {         // wave-uniform trip count: ballots below
            const long long v = v0 + threadIdx.x;
            bool hit = false;
            int i = 0, j = 0, k = 0;
            if (v < cnt) {
                i = r.lo[0] + (int)(v % nx);
                j = r.lo[1] + (int)((v / nx) % ny);
                k = r.lo[2] + (int)(v / ((long long)nx * ny));
                hit = overlap(r, i, j, k);
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
            if (m == 0ull) continue;
            uint32_t base = 0u;
            const int leader = (int)__ffsll((long long)m) - 1;
            if (lane == leader) {
                base = atomicAdd(&plan[2], (uint32_t)__popcll(m));      // one atomic per wave
                if (base + (uint32_t)__popcll(m) < base) plan[3] = 1u;  // wrapped (see k_vox_plan)
            }
            base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
            if (WRITE && hit)
                frags[base + __popcll(m & ((1ull << lane) - 1ull))] =
                    make_uint2((uint32_t)t, vct_morton3((uint32_t)i, (uint32_t)j, (uint32_t)k));
        }
    }
}

// counting sort of the fragment list by brick: marks, per-slot counts, scatter
__global__ void __launch_bounds__(256)
k_frag_mark(const uint2* __restrict__ frags, uint32_t n, uint32_t* __restrict__ mark) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) mark[frags[i].y >> 9] = 1u;
}
__global__ void __launch_bounds__(256)
k_frag_count(const uint2* __restrict__ frags, uint32_t n, const uint32_t* __restrict__ brick_slot, uint32_t* __restrict__ count) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        atomicAdd(&count[brick_slot[frags[i].y >> 9]], 1u);
}
__global__ void __launch_bounds__(256)
k_frag_scatter(const uint2* __restrict__ frags, uint32_t n, const uint32_t* __restrict__ brick_slot,
               const uint32_t* __restrict__ first, uint32_t* __restrict__ cursor, uint32_t* __restrict__ sorted,
               uint32_t* __restrict__ slot_brick) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint2 e = frags[i];
        const uint32_t brick = e.y >> 9, slot = brick_slot[brick];
        const uint32_t at = first[slot] + atomicAdd(&cursor[slot], 1u);
        sorted[at] = (e.x << 9) | (e.y & 511u);          // (triangle, voxel inside the brick): 23 + 9 bits
        slot_brick[slot] = brick;                          // benign race: every writer stores the same value
    }
}

// Per sorted fragment, the values of the pass that do not depend on the light: its barycentrics (BARY: geometry only,
// once per mesh) and its albedo (ALB: vox.fs:56 texture(DiffuseTexture, uv) -- mip-mapped -- or the material's colour;
// once per change of the textures / texture coordinates; only scenes with textures store it).  One workgroup per slot
// (the sorted list does not name a fragment's brick).
struct __attribute__((packed, aligned(4))) VctF3 { float v[3]; };
template <bool BARY, bool ALB>
__global__ void __launch_bounds__(256)
k_frag_geom(const VctVoxParams p, float2* __restrict__ bary, VctF3* __restrict__ falb) {
    for (uint32_t slot = blockIdx.x; slot < p.nslots; slot += gridDim.x) {
        const uint32_t first = p.slot_first[slot], n = p.slot_first[slot + 1] - first;
        const uint32_t bm = p.slot_brick[slot] << 9;
        for (uint32_t f = threadIdx.x; f < n; f += blockDim.x) {
            const uint32_t e = p.frag_sorted[first + f];
            const uint32_t vox = bm | (e & 511u);
            const int t = (int)(e >> 9);
            TriSetup r;
            setup_tri(p, t, r);
            const int i = (int)vct_compact3(vox), j = (int)vct_compact3(vox >> 1), k = (int)vct_compact3(vox >> 2);
            float b0, b1;
            frag_bary(r, i, j, k, b0, b1);
            if (BARY) bary[first + f] = make_float2(b0, b1);
            if (ALB) {
                const float b2 = fmaxf(1.0f - b0 - b1, 0.0f);
                float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (r.tex >= 0 && p.tex.mips) frag_duv(r, i, j, k, d);
                VctF3 o;
                frag_albedo(p, r, b0, b1, b2, d, o.v);
                falb[first + f] = o;
            }
        }
    }
}

// front-face unit normal n = normalize(cross(v1-v0, v2-v0)) of every triangle, quantised floor(n*127+.5)+128 (the voxel
// attribute of the second bounce): geometry only, once per mesh
__global__ void __launch_bounds__(256)
k_tri_nrm(const VctVoxParams p, uint32_t* __restrict__ tri_nrm) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.ntri) return;
    F3 w[3];
    load_world_tri(p, t, w);
    const F3 fn = cross3(sub3(w[1], w[0]), sub3(w[2], w[0]));
    const float fl = __builtin_sqrtf(dot3(fn, fn));
    const float fc[3] = {__fdiv_rn(fn.x, fl), __fdiv_rn(fn.y, fl), __fdiv_rn(fn.z, fl)};
#pragma unroll
    for (int k = 0; k < 3; ++k) tri_nrm[(size_t)t * 3 + k] = (uint32_t)((int)floorf(fc[k] * 127.0f + 0.5f) + 128);
}

// ---- the voxelize pass: one workgroup per work item = up to VCT_VOX_CHUNK fragments of one brick slot ------------
// acc in LDS: [512][2] u64 (sumR | sumG << 32, sumB | count << 32), + [512][3] for the voxel attributes.
// A slot of one chunk (most) is resolved from LDS by its workgroup.  The chunks of a heavier slot add their non-empty
// LDS sums to the slot's accumulators in HBM (acc2 / acc2_attr; integer sums: any order gives the same bits); a SECOND
// small launch, k_vox_resolve_multi, turns those sums into texels and re-zeroes them for the next pass.  (A "last
// chunk resolves" variant with an arrival counter needs a device-scope release / acquire per workgroup -- a write-back
// and invalidate of the XCD's L2 on this GPU -- and ran 4x slower.)
__device__ __forceinline__ void resolve_attr(uint32_t c, unsigned long long q0, unsigned long long q1, unsigned long long q2,
                                             uint32_t& alb, uint32_t& nrm) {
    alb = 0u; nrm = 0u;
    if (c) {
        const uint32_t h = c >> 1;
        alb = (((uint32_t)q0 + h) / c) | ((((uint32_t)(q0 >> 32) + h) / c) << 8) |
              ((((uint32_t)q1 + h) / c) << 16) | 0xff000000u;
        nrm = (((uint32_t)(q1 >> 32) + h) / c) | ((((uint32_t)q2 + h) / c) << 8) |
              ((((uint32_t)(q2 >> 32) + h) / c) << 16) | 0xff000000u;
    }
}

// (4 waves per SIMD: the kernel waits on memory more than it computes; unbounded, hipcc takes 132-134 VGPRs and loses one)
#ifndef VCT_VOX_MIN_BLOCKS
#define VCT_VOX_MIN_BLOCKS 4
#endif
// Threads per work item: 256, or 128 for meshes of many work items (VCT_VOX_SMALL_BLOCK_ITEMS).  The kernel takes its
// stride from blockDim; with half the threads an item runs twice the iterations but twice as many items are resident
// (8 instead of 4 per CU at the same 4 waves per SIMD), which hides the dependent round trips at the head and tail of an
// item better once there are several generations of items anyway.  Street: 1024^3 (40 k items) 0.459 -> 0.408 ms,
// 512^3 0.221 -> 0.205; with few items it loses (street 256^3 0.127 -> 0.145, atrium 0.035 -> 0.048: 2.5 k items are
// one generation of 128-thread workgroups).  512 threads lose everywhere (0.56 / 0.25 / 0.134 / 0.042).
#ifndef VCT_VOX_SMALL_BLOCK_ITEMS
#define VCT_VOX_SMALL_BLOCK_ITEMS 8192u
#endif
#ifndef VCT_VOX_TINY_BLOCK_ITEMS
#define VCT_VOX_TINY_BLOCK_ITEMS 32768u     // from here on one wave per item
#endif
template <bool ATTR, bool FALB>
__global__ void __launch_bounds__(256, VCT_VOX_MIN_BLOCKS)
k_voxelize_bricks(const VctVoxParams p) {
    __shared__ unsigned long long acc[512 * 2];
    __shared__ unsigned long long acc_attr[ATTR ? 512 * 3 : 1];
    const VctF3* __restrict__ falb = reinterpret_cast<const VctF3*>(p.frag_alb);
    for (uint32_t it = blockIdx.x; it < p.nitems; it += gridDim.x) {
        // (slot, first fragment, fragments, index among the multi-chunk slots or ~0: the slot's only chunk): everything
        // the workgroup needs to start on its fragments in ONE scalar load
        const uint4 w = p.items[it];
        const uint32_t slot = w.x, first = w.y, n = w.z, mi = w.w;
        uint32_t* __restrict__ out = p.stage + (size_t)slot * 512;
        if (n == 0u) {                    // a brick only the reference-mode voxelizer can touch: nothing of this mode
            for (uint32_t v = threadIdx.x; v < 512u; v += blockDim.x) {
                out[v] = 0u;
                if (ATTR) { p.stage_albedo[(size_t)slot * 512 + v] = 0u; p.stage_normal[(size_t)slot * 512 + v] = 0u; }
            }
            continue;
        }
        // the first fragment's list entry and light-independent values are requested before the accumulators are zeroed;
        // inside the loop the next fragment's are requested before the current one is evaluated (the kernel waits on
        // memory two thirds of its time at 4 waves per SIMD: every dependent round trip taken off a fragment counts)
        uint32_t f = threadIdx.x;
        uint32_t e = 0u;
        float2 bb = make_float2(0.0f, 0.0f);
        VctF3 fa = {{0.0f, 0.0f, 0.0f}};
        if (f < n) {
            e = p.frag_sorted[first + f];
            bb = p.frag_bary[first + f];
            if (FALB) fa = falb[first + f];
        }
        for (uint32_t v = threadIdx.x; v < 512u * 2u; v += blockDim.x) acc[v] = 0ull;
        if (ATTR) for (uint32_t v = threadIdx.x; v < 512u * 3u; v += blockDim.x) acc_attr[v] = 0ull;
        __syncthreads();
        while (f < n) {
            const uint32_t fn = f + blockDim.x;
            uint32_t e_next = 0u;
            float2 bb_next = bb;
            VctF3 fa_next = fa;
            if (fn < n) {
                e_next = p.frag_sorted[first + fn];
                bb_next = p.frag_bary[first + fn];
                if (FALB) fa_next = falb[first + fn];
            }
            const uint32_t local = e & 511u;
            PassTri r;
            setup_pass<ATTR, FALB>(p, (int)(e >> 9), r);
            const FragValue fv = frag_eval(p, r, bb.x, bb.y, FALB ? fa.v : r.alb);
            atomicAdd(&acc[2 * local], (unsigned long long)fv.lit.r | ((unsigned long long)fv.lit.g << 32));       // ds_add_u64
            atomicAdd(&acc[2 * local + 1], (unsigned long long)fv.lit.b | (1ull << 32));
            if (ATTR) {
                atomicAdd(&acc_attr[3 * local], (unsigned long long)fv.alb.r | ((unsigned long long)fv.alb.g << 32));
                atomicAdd(&acc_attr[3 * local + 1], (unsigned long long)fv.alb.b | ((unsigned long long)r.nrm[0] << 32));
                atomicAdd(&acc_attr[3 * local + 2], (unsigned long long)r.nrm[1] | ((unsigned long long)r.nrm[2] << 32));
            }
            f = fn; e = e_next; bb = bb_next; fa = fa_next;
        }
        __syncthreads();
        if (mi == 0xffffffffu) {
            for (uint32_t v = threadIdx.x; v < 512u; v += blockDim.x) {
                const ulonglong2 a = make_ulonglong2(acc[2 * v], acc[2 * v + 1]);
                out[v] = resolve_voxel(a);
                if (ATTR) {
                    uint32_t alb, nrm;
                    resolve_attr((uint32_t)(a.y >> 32), acc_attr[3 * v], acc_attr[3 * v + 1], acc_attr[3 * v + 2], alb, nrm);
                    p.stage_albedo[(size_t)slot * 512 + v] = alb;
                    p.stage_normal[(size_t)slot * 512 + v] = nrm;
                }
            }
            if (threadIdx.x == 0) p.brick_flags[p.slot_brick[slot]] = 1u;
        } else {
            unsigned long long* __restrict__ g = p.acc2 + (size_t)mi * 1024;
            unsigned long long* __restrict__ ga = ATTR ? p.acc2_attr + (size_t)mi * 1536 : nullptr;
            for (uint32_t v = threadIdx.x; v < 512u; v += blockDim.x) {
                const unsigned long long a1 = acc[2 * v + 1];
                if ((a1 >> 32) == 0ull) continue;                    // no fragment of this chunk in the voxel
                atomicAdd(&g[2 * v], acc[2 * v]);
                atomicAdd(&g[2 * v + 1], a1);
                if (ATTR) {
                    atomicAdd(&ga[3 * v], acc_attr[3 * v]);
                    atomicAdd(&ga[3 * v + 1], acc_attr[3 * v + 1]);
                    atomicAdd(&ga[3 * v + 2], acc_attr[3 * v + 2]);
                }
            }
            // (k_vox_resolve_multi, the next launch, turns the sums into texels: a "last chunk resolves" scheme needs a
            // device-scope release / acquire pair per workgroup, which on this GPU is a write-back and an invalidate of the
            // XCD's L2 -- measured: the pass four times slower)
        }
        __syncthreads();           // the accumulators are re-zeroed for the next work item of this workgroup
    }
}

// the multi-chunk slots of the pass: sums -> texels (+ attributes), accumulators back to zero
template <bool ATTR>
__global__ void __launch_bounds__(256)
k_vox_resolve_multi(const VctVoxParams p, const uint32_t* __restrict__ multi_slot, uint32_t nmulti) {
    for (uint32_t mi = blockIdx.x; mi < nmulti; mi += gridDim.x) {
        const uint32_t slot = multi_slot[mi];
        unsigned long long* __restrict__ g = p.acc2 + (size_t)mi * 1024;
        unsigned long long* __restrict__ ga = ATTR ? p.acc2_attr + (size_t)mi * 1536 : nullptr;
        for (uint32_t v = threadIdx.x; v < 512u; v += blockDim.x) {
            const ulonglong2 a = make_ulonglong2(g[2 * v], g[2 * v + 1]);
            p.stage[(size_t)slot * 512 + v] = resolve_voxel(a);
            const bool any = (a.y >> 32) != 0ull;
            if (any) { g[2 * v] = 0ull; g[2 * v + 1] = 0ull; }
            if (ATTR) {
                uint32_t alb = 0u, nrm = 0u;
                if (any) {
                    resolve_attr((uint32_t)(a.y >> 32), ga[3 * v], ga[3 * v + 1], ga[3 * v + 2], alb, nrm);
                    ga[3 * v] = 0ull; ga[3 * v + 1] = 0ull; ga[3 * v + 2] = 0ull;
                }
                p.stage_albedo[(size_t)slot * 512 + v] = alb;
                p.stage_normal[(size_t)slot * 512 + v] = nrm;
            }
        }
        if (threadIdx.x == 0) p.brick_flags[p.slot_brick[slot]] = 1u;
    }
}

// ---- reference mode (S/Voxelization.vs/.gs/.fs as written): dominant-axis projection, V x V raster
// at pixel centres with the top-left rule, voxel index from (x, y, V*depth) (vox.fs:58-86), value
// = unorm8(albedo * PCF/25), a = 1, and "imageStore: last writer wins".  The reference's store order
// is a race; the deterministic reading the oracle uses -- the last triangle in submission order
// wins -- is an order-independent 64-bit atomicMax on (triangle + 1) << 32 | rgb.
struct RefSetup : TriMaterial {
    float wx[3], wy[3], wz[3];
    F3 dc[3];
    float area, sgn;
    int x0, x1, y0, y1, axis;
    bool ok;
};

__device__ __forceinline__ void ref_setup(const VctVoxParams& p, int t, RefSetup& r) {
    F3 w[3];
    const float fV = (float)p.V;
    load_world_tri(p, t, w);
    shadow_coords(p, w, r.dc);
    r.axis = dominant_axis(w);
    const float* proj = p.proj + 16 * (r.axis - 1);
    for (int k = 0; k < 3; ++k) {
        const F3 ndc = xform_point(proj, w[k]);                                       // vox.gs:47 (w = 1)
        r.wx[k] = (ndc.x * 0.5f + 0.5f) * fV;
        r.wy[k] = (ndc.y * 0.5f + 0.5f) * fV;
        r.wz[k] = ndc.z * 0.5f + 0.5f;
    }
    const float area = (r.wx[1] - r.wx[0]) * (r.wy[2] - r.wy[0]) - (r.wx[2] - r.wx[0]) * (r.wy[1] - r.wy[0]);
    r.ok = !(area == 0.0f || area != area);
    r.sgn = area > 0.0f ? 1.0f : -1.0f;
    r.area = area * r.sgn;
    r.x0 = max((int)floorf(fminf(fminf(r.wx[0], r.wx[1]), r.wx[2])), 0);
    r.x1 = min((int)floorf(fmaxf(fmaxf(r.wx[0], r.wx[1]), r.wx[2])), p.V - 1);
    r.y0 = max((int)floorf(fminf(fminf(r.wy[0], r.wy[1]), r.wy[2])), 0);
    r.y1 = min((int)floorf(fmaxf(fmaxf(r.wy[0], r.wy[1]), r.wy[2])), p.V - 1);
    load_material(p, t, r);
}

__device__ __forceinline__ void ref_fragment(const VctVoxParams& p, const RefSetup& r, int t, int px, int py) {
    const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
    float e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;            // edge opposite vertex k
        const float dx = (r.wx[b] - r.wx[a]) * r.sgn, dy = (r.wy[b] - r.wy[a]) * r.sgn;
        e[k] = dx * (cy - r.wy[a]) - dy * (cx - r.wx[a]);
        const bool top_left = (dy > 0.0f) || (dy == 0.0f && dx < 0.0f);              // [GL] fill rule
        if (e[k] < 0.0f || (e[k] == 0.0f && !top_left)) return;
    }
    const float l0 = __fdiv_rn(e[0], r.area), l1 = __fdiv_rn(e[1], r.area), l2 = 1.0f - l0 - l1;
    const float fz = l0 * r.wz[0] + l1 * r.wz[1] + l2 * r.wz[2];
    const int V = p.V;
    const int ix = (int)cx, iy = (int)cy, iz = (int)((float)V * fz);                  // vox.fs:58
    int vx, vy, vz;
    if (r.axis == 1) { vx = V - 1 - iz; vz = V - 1 - ix; vy = iy; }                   // vox.fs:70-75
    else if (r.axis == 2) { vz = V - 1 - iy; vy = V - 1 - iz; vx = ix; }              // :76-81
    else { vx = ix; vy = iy; vz = V - 1 - iz; }                                       // :82-86
    if (vx < 0 || vy < 0 || vz < 0 || vx >= V || vy >= V || vz >= V) return;          // [GL] store dropped
    const uint32_t vox = vct_morton3((uint32_t)vx, (uint32_t)vy, (uint32_t)vz);
    if (p.mark_only) { p.brick_mark[vox >> 9] = 1u; return; }
    const float sh = shadow_factor(p, r.dc, l0, l1, l2);
    float alb[3];
    float duv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r.tex >= 0 && p.tex.mips) {
        // the neighbouring pixel centres of the fragment's 2x2 quad; unclamped barycentrics from the signed edge functions
        auto uv_at = [&](int qx, int qy) {
            const float nx = (float)qx + 0.5f, ny = (float)qy + 0.5f;
            float f[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int a = (k + 1) % 3, b = (k + 2) % 3;
                const float dx = (r.wx[b] - r.wx[a]) * r.sgn, dy = (r.wy[b] - r.wy[a]) * r.sgn;
                f[k] = dx * (ny - r.wy[a]) - dy * (nx - r.wx[a]);
            }
            const float c0 = __fdiv_rn(f[0], r.area), c1 = __fdiv_rn(f[1], r.area);
            return interp_uv(r, c0, c1, 1.0f - c0 - c1);
        };
        quad_duv(uv_at(px, py), uv_at(px ^ 1, py), uv_at(px, py ^ 1), duv);
    }
    frag_albedo(p, r, l0, l1, l2, duv, alb);                                          // vox.fs:56
    const Rgb8 c = lit_rgb8(alb, sh);
    atomicMax(p.acc + 2 * ((size_t)p.brick_slot[vox >> 9] * 512 + (vox & 511u)),
              ((unsigned long long)(uint32_t)(t + 1) << 32) | c.r | (c.g << 8) | (c.b << 16));
    p.brick_flags[vox >> 9] = 1u;
}

#define VCT_REF_SMALL 64

__global__ void __launch_bounds__(256)
k_voxelize_reference(const VctVoxParams p, int32_t* big_list, int32_t* big_count) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.ntri) return;
    RefSetup r;
    ref_setup(p, t, r);
    if (!r.ok || r.x1 < r.x0 || r.y1 < r.y0) return;
    if ((long long)(r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1) > VCT_REF_SMALL) {
        big_list[atomicAdd(big_count, 1)] = t;
        return;
    }
    for (int py = r.y0; py <= r.y1; ++py)
        for (int px = r.x0; px <= r.x1; ++px) ref_fragment(p, r, t, px, py);
}

__global__ void __launch_bounds__(256)
k_voxelize_reference_big(const VctVoxParams p, const int32_t* big_list, const int32_t* big_count) {
    const int nbig = *big_count;
    for (int b = blockIdx.x; b < nbig; b += gridDim.x) {
        const int t = big_list[b];
        RefSetup r;
        ref_setup(p, t, r);
        const int bw = r.x1 - r.x0 + 1;
        const long long box = (long long)bw * (r.y1 - r.y0 + 1);
        for (long long i = threadIdx.x; i < box; i += blockDim.x)
            ref_fragment(p, r, t, r.x0 + (int)(i % bw), r.y0 + (int)(i / bw));
    }
}

// Per-byte saturating add of two RGBA8 words (emissive materials: staged texel + emission-pool texel).  Even and odd
// bytes are added apart, each in a 16-bit field, so a byte's carry lands in the gap above it instead of in its
// neighbour; a field whose bit 8 is set overflowed and its byte becomes 255.
__device__ __forceinline__ uint32_t add_sat_rgba8(uint32_t a, uint32_t b) {
    const uint32_t even = (a & 0x00ff00ffu) + (b & 0x00ff00ffu);
    const uint32_t odd = ((a >> 8) & 0x00ff00ffu) + ((b >> 8) & 0x00ff00ffu);
    const uint32_t even_s = (even | (((even >> 8) & 0x00010001u) * 0xffu)) & 0x00ff00ffu;
    const uint32_t odd_s = (odd | (((odd >> 8) & 0x00010001u) * 0xffu)) & 0x00ff00ffu;
    return even_s | (odd_s << 8);
}

// A pass's result -> RGBA8 level 0 (Morton) for the bricks that were touched in this pass or in the previous one (all
// bricks if `dense`), one wave per 8^3 brick.  Three cases: the mesh has no slot for the brick (level 0 is empty there);
// north-star mode: the brick's staged texels (+ voxel attributes) are copied -- plus, with emissive materials, the
// emission pool's brick per byte with saturation (a.emis, wave-uniform: one more coalesced 2 KiB read); reference mode: the last writer's colour
// is unpacked from the slot's words, which go back to zero.
__global__ void __launch_bounds__(256)
k_resolve_sparse(const VctResolveArgs a, uint32_t nbricks, int dense, int scan64) {
    const int lane = threadIdx.x & 63;
    const uint32_t waves = (gridDim.x * blockDim.x) >> 6;
    // The flags are read 64 bricks at a time, one brick per lane, and the wave then serves the flagged ones one after the
    // other (round 3: one brick per wave iteration made the scan of a 1024^3 grid's 2 M bricks -- 36 k of them touched --
    // 64 dependent round trips per wave: 0.20 ms).  A wave's 64 bricks are spread over the whole grid
    // (lane * nchunks + chunk): touched bricks cluster in Morton order and would otherwise all fall to a few waves.
    // Only worth it for the largest grids: with few bricks per wave (256^3: one, 512^3: eight) the per-brick scan is a
    // handful of round trips and keeps every wave busy with at most a brick or two, while 64 bricks per wave would put a
    // dozen touched bricks in a row on a few waves (measured: 0.012 -> 0.046 ms at 256^3, 0.20 -> 0.086 ms at 1024^3).
    // group = bricks a wave looks at per iteration: 64 lanes' worth, or 1.
    const uint32_t group = scan64 ? 64u : 1u;
    const uint32_t nchunks = (nbricks + group - 1u) / group;
    for (uint32_t c = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; c < nchunks; c += waves) {
      const uint32_t mine = scan64 ? (uint32_t)lane * nchunks + c : c;
      const bool in = mine < nbricks && (scan64 || lane == 0);
      const uint32_t now_l = in ? a.flags[mine] : 0u, before_l = in ? a.prev[mine] : 0u;
      for (unsigned long long todo = __builtin_amdgcn_ballot_w64(in && (dense || (now_l | before_l) != 0u)); todo != 0ull;
           todo &= todo - 1ull) {
        const int src = (int)__ffsll((long long)todo) - 1;
        const uint32_t b = scan64 ? (uint32_t)src * nchunks + c : c;
        const uint32_t now = (uint32_t)__builtin_amdgcn_readlane((int)now_l, src);
        uint32_t* l0 = a.level0 + (size_t)b * 512;
        const uint32_t slot = a.brick_slot[b];
        if (slot == VCT_NO_SLOT) {        // no fragment of this mesh can land here: level 0 is empty
            for (uint32_t v = lane; v < 512u; v += 64) l0[v] = 0u;
            if (lane == 0) { a.prev[b] = 0u; a.flags[b] = 0u; }
            continue;
        }
        if (a.stage) {        // north-star mode: k_voxelize_bricks already resolved the brick into its staging slot
            for (uint32_t v = lane; v < 512u; v += 64) {
                const size_t vox = (size_t)slot * 512 + v;
                l0[v] = a.emis ? add_sat_rgba8(a.stage[vox], a.emis[vox]) : a.stage[vox];
                if (a.stage_albedo) { a.attr_albedo[vox] = a.stage_albedo[vox]; a.attr_normal[vox] = a.stage_normal[vox]; }
            }
        } else {              // reference mode: (triangle + 1) << 32 | rgb of the last triangle that stored here
            ulonglong2* w = reinterpret_cast<ulonglong2*>(a.acc) + (size_t)slot * 512;
            for (uint32_t v = lane; v < 512u; v += 64) {
                const unsigned long long last = w[v].x;
                l0[v] = last ? ((uint32_t)last & 0xffffffu) | 0xff000000u : 0u;
                if (last) w[v] = make_ulonglong2(0ull, 0ull);
            }
        }
        if (lane == 0) { a.prev[b] = now; a.flags[b] = 0u; }
      }
    }
}

__global__ void __launch_bounds__(256)
k_assign_slots(const uint32_t* __restrict__ mark, uint32_t* __restrict__ slot, uint32_t* __restrict__ count,
               uint32_t nbricks) {
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < nbricks; b += gridDim.x * blockDim.x)
        slot[b] = mark[b] ? atomicAdd(count, 1u) : VCT_NO_SLOT;
}

// slot -> brick for EVERY slot (k_frag_scatter only names the bricks that hold a conservative fragment; a slot the
// mark-only run of the reference-mode voxelizer created would keep pointing at brick 0 -- the slot-driven loops of the
// second bounce then visited brick 0 once per such slot: found by the fuzzer as an over-count of cone steps)
__global__ void __launch_bounds__(256)
k_slot_bricks(const uint32_t* __restrict__ slot, uint32_t nbricks, uint32_t* __restrict__ slot_brick) {
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < nbricks; b += gridDim.x * blockDim.x) {
        const uint32_t s = slot[b];
        if (s != VCT_NO_SLOT) slot_brick[s] = b;
    }
}

__global__ void __launch_bounds__(256)
k_unpool(const uint32_t* __restrict__ pooled, const uint32_t* __restrict__ brick_slot, uint32_t* __restrict__ dense,
         uint32_t nbricks) {
    const int lane = threadIdx.x & 63;
    const uint32_t waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; b < nbricks; b += waves) {
        const uint32_t slot = brick_slot[b];
        for (uint32_t v = lane; v < 512u; v += 64)
            dense[(size_t)b * 512 + v] = slot == VCT_NO_SLOT ? 0u : pooled[(size_t)slot * 512 + v];
    }
}

// ---- the dynamic mesh (include/vct.h "dynamic mesh") ----------------------------------------------
// A small mesh whose positions change every frame is voxelized by itself in every pass, with none of the plan above: no
// fragment list, no sort, nothing the host reads.  Two launches per triangle class (a thread per triangle; a workgroup
// per triangle whose box exceeds VCT_VOX_BIG voxels):
//   slots      every brick an overlapped voxel lies in is claimed in the [V^3/512] table with one atomicCAS; the winner
//              draws a slot number and stores slot -> brick and brick -> slot.  Nobody waits inside the kernel: a loser
//              needs nothing of the winner before the next launch.  Slot numbers are racy, nothing indexed by brick is.
//   fragments  (a launch later: the table is complete) every overlapped voxel's fragment -- frag_bary, frag_eval, the
//              face normal of k_tri_nrm, operation for operation what the static pass evaluates -- is added to the slot's
//              accumulators in HBM with 64-bit integer atomics, packed like acc2 / acc2_attr: any order gives the same
//              sums.  If the pass claimed more bricks than the layer has slots the launch does nothing (a wave-uniform
//              test of the counter word): the whole layer is left out, never "some" bricks.
// k_dyn_merge, behind the static resolve, turns the sums into texels with resolve_voxel / resolve_attr.
__device__ __forceinline__ bool dyn_in_contract(const VctVoxParams& p, const VctDynArgs& d, int t) {
    const VctTri9 rec = *reinterpret_cast<const VctTri9*>(p.pos + (size_t)t * 9);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && fabsf(rec.v[k] * p.model_scale) <= d.vertex_limit;      // false for NaN and infinities
    return ok;
}
__device__ __forceinline__ void dyn_claim(const VctDynArgs& d, uint32_t brick) {
    if (__hip_atomic_load(&d.brick_slot[brick], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != VCT_NO_SLOT) return;
    if (atomicCAS(&d.brick_slot[brick], VCT_NO_SLOT, VCT_DYN_CLAIMED) != VCT_NO_SLOT) return;
    const uint32_t s = atomicAdd(&d.words[VCT_DYN_W_NEED], 1u);
    if (s < d.max_bricks) {       // (beyond the capacity the entry stays VCT_DYN_CLAIMED: the count goes on, k_dyn_merge sweeps the table)
        d.slot_brick[s] = brick;
        __hip_atomic_store(&d.brick_slot[brick], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// what the fragments of a triangle share: shadow coordinates and colour as setup_pass gives them, the quantised face
// normal as k_tri_nrm stores it
template <bool ATTR>
__device__ __forceinline__ void dyn_pass_tri(const VctVoxParams& p, int t, const TriSetup& r, PassTri& q) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { q.dc[k] = r.dc[k]; q.alb[k] = r.alb[k]; q.nrm[k] = 0u; }
    if (ATTR) {
        F3 w[3];
        load_world_tri(p, t, w);
        const F3 fn = cross3(sub3(w[1], w[0]), sub3(w[2], w[0]));
        const float fl = __builtin_sqrtf(dot3(fn, fn));
        const float fc[3] = {__fdiv_rn(fn.x, fl), __fdiv_rn(fn.y, fl), __fdiv_rn(fn.z, fl)};
#pragma unroll
        for (int k = 0; k < 3; ++k) q.nrm[k] = (uint32_t)((int)floorf(fc[k] * 127.0f + 0.5f) + 128);
    }
}
template <bool ATTR>
__device__ __forceinline__ void dyn_fragment(const VctVoxParams& p, const VctDynArgs& d, const TriSetup& r, const PassTri& q,
                                             int i, int j, int k) {
    float b0, b1;
    frag_bary(r, i, j, k, b0, b1);
    const FragValue fv = frag_eval(p, q, b0, b1, q.alb);
    const uint32_t vox = vct_morton3((uint32_t)i, (uint32_t)j, (uint32_t)k);
    const uint32_t slot = d.brick_slot[vox >> 9];
    if (slot >= d.max_bricks) return;       // (cannot happen in a pass within capacity; never write outside the pools)
    const size_t at = (size_t)slot * 512 + (vox & 511u);
    atomicAdd(&d.acc[2 * at], (unsigned long long)fv.lit.r | ((unsigned long long)fv.lit.g << 32));
    atomicAdd(&d.acc[2 * at + 1], (unsigned long long)fv.lit.b | (1ull << 32));
    if (ATTR) {
        atomicAdd(&d.acc_attr[3 * at], (unsigned long long)fv.alb.r | ((unsigned long long)fv.alb.g << 32));
        atomicAdd(&d.acc_attr[3 * at + 1], (unsigned long long)fv.alb.b | ((unsigned long long)q.nrm[0] << 32));
        atomicAdd(&d.acc_attr[3 * at + 2], (unsigned long long)q.nrm[1] | ((unsigned long long)q.nrm[2] << 32));
    }
}
// Emission of the dynamic mesh (vct_set_dynamic_emission).  Only the EMIS instantiations take the table and the sums: the
// argument block of the others is VctDynArgs / VctDynMergeArgs as it was.  A triangle's emission is constant, so its
// three bytes unorm8(emission[material] * 1.0f) -- the static emission pool's fragment value -- are formed once per
// triangle; a fragment adds them to two words per voxel beside `acc` (r | g << 32, b; the count is acc's: 255 * 2^20
// fragments stay below 2^32 per channel).  A zero half issues no atomic: adding 0 changes nothing, so a mover with one
// glowing material pays for that material's fragments alone.
struct DynEmisArgs : VctDynArgs { VctDynEmisArgs e; };
struct DynEmisMergeArgs : VctDynMergeArgs { unsigned long long* acc_emis; };
template <bool EMIS> using DynArgs = std::conditional_t<EMIS, DynEmisArgs, VctDynArgs>;
template <bool EMIS> using DynMergeArgs = std::conditional_t<EMIS, DynEmisMergeArgs, VctDynMergeArgs>;
struct DynEmisTri { unsigned long long rg, b; };
__device__ __forceinline__ DynEmisTri dyn_emis_tri(const VctVoxParams& p, const VctDynEmisArgs& e, int t) {
    const float* c = e.emission + 4 * (size_t)p.material[t];
    const float em[3] = {c[0], c[1], c[2]};
    const Rgb8 v = lit_rgb8(em, 1.0f);
    return {(unsigned long long)v.r | ((unsigned long long)v.g << 32), (unsigned long long)v.b};
}
__device__ __forceinline__ void dyn_emis_fragment(const VctDynArgs& d, const VctDynEmisArgs& e, const DynEmisTri& q, int i, int j, int k) {
    if (!(q.rg | q.b)) return;
    const uint32_t vox = vct_morton3((uint32_t)i, (uint32_t)j, (uint32_t)k);
    const uint32_t slot = d.brick_slot[vox >> 9];
    if (slot >= d.max_bricks) return;       // (as dyn_fragment: never write outside the sums)
    const size_t at = (size_t)slot * 512 + (vox & 511u);
    if (q.rg) atomicAdd(&e.acc_emis[2 * at], q.rg);
    if (q.b) atomicAdd(&e.acc_emis[2 * at + 1], q.b);
}
// one add per wave of the lanes' values to a counter word
__device__ __forceinline__ void dyn_wave_add(uint32_t* word, uint32_t mine) {
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(word, mine);
}

template <bool FRAGS, bool ATTR, bool EMIS = false>
__global__ void __launch_bounds__(256)
k_dyn_tris(const VctVoxParams p, const DynArgs<EMIS> d) {
    if (FRAGS && d.words[VCT_DYN_W_NEED] > d.max_bricks) return;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nfrag = 0u, skipped = 0u;
    if (t < p.ntri) {
        if (!dyn_in_contract(p, d, t)) skipped = 1u;
        else {
            TriSetup r;
            setup_tri(p, t, r);
            const long long cnt = tri_candidates(r);
            if (cnt > VCT_VOX_BIG) {
                if (!FRAGS) d.big_list[atomicAdd(&d.words[VCT_DYN_W_NBIG], 1u)] = t;      // (capacity ntri)
            } else if (cnt > 0) {
                if (!FRAGS) {
                    uint32_t last = VCT_NO_SLOT;
                    for_each_overlap(r, [&](int i, int j, int k) {
                        ++nfrag;
                        const uint32_t brick = vct_morton3((uint32_t)i, (uint32_t)j, (uint32_t)k) >> 9;
                        if (brick != last) { dyn_claim(d, brick); last = brick; }
                    });
                } else {
                    PassTri q;
                    dyn_pass_tri<ATTR>(p, t, r, q);
                    if constexpr (EMIS) {
                        const DynEmisTri qe = dyn_emis_tri(p, d.e, t);
                        for_each_overlap(r, [&](int i, int j, int k) {
                            dyn_fragment<ATTR>(p, d, r, q, i, j, k);
                            dyn_emis_fragment(d, d.e, qe, i, j, k);
                        });
                    } else {
                        for_each_overlap(r, [&](int i, int j, int k) { dyn_fragment<ATTR>(p, d, r, q, i, j, k); });
                    }
                }
            }
        }
    }
    if (!FRAGS) {
        dyn_wave_add(&d.words[VCT_DYN_W_FRAGS], nfrag);
        dyn_wave_add(&d.words[VCT_DYN_W_SKIPPED], skipped);
    }
}

// the big triangles, a workgroup striding the box of each (as k_vox_plan_big): one huge triangle does not wait on a lane
template <bool FRAGS, bool ATTR, bool EMIS = false>
__global__ void __launch_bounds__(256)
k_dyn_big(const VctVoxParams p, const DynArgs<EMIS> d) {
    if (FRAGS && d.words[VCT_DYN_W_NEED] > d.max_bricks) return;
    const int n_big = min((int)d.words[VCT_DYN_W_NBIG], p.ntri);
    for (int b = blockIdx.x; b < n_big; b += gridDim.x) {
        const int t = d.big_list[b];
        TriSetup r;
        setup_tri(p, t, r);
        PassTri q;
        if (FRAGS) dyn_pass_tri<ATTR>(p, t, r, q);
        DynEmisTri qe = {0ull, 0ull};
        if constexpr (EMIS) qe = dyn_emis_tri(p, d.e, t);
        const int nx = r.hi[0] - r.lo[0] + 1, ny = r.hi[1] - r.lo[1] + 1, nz = r.hi[2] - r.lo[2] + 1;
        const long long cnt = (long long)nx * ny * nz;
        uint32_t nfrag = 0u;
        for (long long v = threadIdx.x; v < cnt; v += blockDim.x) {
            const int i = r.lo[0] + (int)(v % nx);
            const int j = r.lo[1] + (int)((v / nx) % ny);
            const int k = r.lo[2] + (int)(v / ((long long)nx * ny));
            if (!overlap(r, i, j, k)) continue;
            if (!FRAGS) {
                ++nfrag;
                dyn_claim(d, vct_morton3((uint32_t)i, (uint32_t)j, (uint32_t)k) >> 9);
            } else {
                dyn_fragment<ATTR>(p, d, r, q, i, j, k);
                if constexpr (EMIS) dyn_emis_fragment(d, d.e, qe, i, j, k);
            }
        }
        if (!FRAGS) dyn_wave_add(&d.words[VCT_DYN_W_FRAGS], nfrag);
    }
}

// Behind the static resolve (and the static light kernel), one wave per slot of the dynamic layer: the rounded means of
// the slot's sums; texels with a fragment go into level 0 (the dynamic mesh wins per voxel), the brick's texels and
// attributes into the layer's own pools (what k_light_voxels and the downloads read); accumulators and table entry go
// back to zero / VCT_NO_SLOT and brick_prev is raised, so that the next static resolve restores or clears the brick and
// the sparse mip build reduces it.  A slot that held a brick in the last resolved pass and holds none now gets empty
// pools and brick 0 in the resolved list: k_light_voxels, launched over every slot, finds no occupied voxel there.
// A pass beyond the capacity added nothing to the accumulators; its table -- claimed entries without a slot among
// them -- is swept.  discard: only the accumulators and the table, for a pass that is never resolved.
// EMIS (the pass was voxelized with an emission table): the texel is D' = D + DEm per byte with saturation, DEm the
// rounded mean of the emission sums over acc's count; it goes to level 0 and to pool_rad alike, and the emission words
// go back to zero wherever acc's do, in the discard form too.
template <bool ATTR, bool EMIS = false>
__global__ void __launch_bounds__(256)
k_dyn_merge(const DynMergeArgs<EMIS> a) {
    const int lane = threadIdx.x & 63;
    const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
    const uint32_t need = a.d.words[VCT_DYN_W_NEED];
    const bool left_out = need > a.d.max_bricks;
    const uint32_t used = left_out ? 0u : need;
    const uint32_t* before = a.d.words + VCT_DYN_W_STATS + 8 * (1 - a.set);
    const uint32_t top = a.discard ? used : max(used, min(before[1], a.d.max_bricks));
    if (left_out)
        for (uint32_t b = gtid; b < a.nbricks; b += nthreads) a.d.brick_slot[b] = VCT_NO_SLOT;
    for (uint32_t sl = gtid >> 6; sl < top; sl += nthreads >> 6) {
        const size_t pool = (size_t)sl * 512;
        if (sl >= used) {
            for (uint32_t v = lane; v < 512u; v += 64) {
                a.pool_rad[pool + v] = 0u;
                if (ATTR) { a.pool_alb[pool + v] = 0u; a.pool_nrm[pool + v] = 0u; }
            }
            if (lane == 0) a.res_brick[sl] = 0u;
            continue;
        }
        const uint32_t b = a.d.slot_brick[sl];
        if (b >= a.nbricks) continue;
        for (uint32_t v = lane; v < 512u; v += 64) {
            unsigned long long* g = a.d.acc + 2 * (pool + v);
            const ulonglong2 s = make_ulonglong2(g[0], g[1]);
            const uint32_t c = (uint32_t)(s.y >> 32);
            if (c) { g[0] = 0ull; g[1] = 0ull; }
            uint32_t emis = 0u;
            if constexpr (EMIS) {
                if (c) {
                    unsigned long long* ge = a.acc_emis + 2 * (pool + v);
                    const unsigned long long e0 = ge[0], e1 = ge[1];
                    if (e0 | e1) {
                        ge[0] = 0ull; ge[1] = 0ull;
                        emis = resolve_voxel(make_ulonglong2(e0, (e1 & 0xffffffffull) | ((unsigned long long)c << 32))) & 0x00ffffffu;
                    }
                }
            }
            if (!a.discard) {
                const uint32_t texel = EMIS ? add_sat_rgba8(resolve_voxel(s), emis) : resolve_voxel(s);
                a.pool_rad[pool + v] = texel;
                if (c) a.level0[(size_t)b * 512 + v] = texel;
            }
            if (ATTR) {
                unsigned long long* ga = a.d.acc_attr + 3 * (pool + v);
                uint32_t alb = 0u, nrm = 0u;
                if (c) {
                    resolve_attr(c, ga[0], ga[1], ga[2], alb, nrm);
                    ga[0] = 0ull; ga[1] = 0ull; ga[2] = 0ull;
                }
                if (!a.discard) { a.pool_alb[pool + v] = alb; a.pool_nrm[pool + v] = nrm; }
            }
        }
        if (lane == 0) {
            a.d.brick_slot[b] = VCT_NO_SLOT;
            if (!a.discard) { a.brick_prev[b] = 1u; a.res_brick[sl] = b; }
        }
    }
    if (!a.discard && gtid == 0u) {
        uint32_t* now = a.d.words + VCT_DYN_W_STATS + 8 * a.set;
        now[0] = need; now[1] = used; now[2] = a.d.words[VCT_DYN_W_FRAGS]; now[3] = a.d.words[VCT_DYN_W_SKIPPED];
        now[4] = left_out ? 1u : 0u;
    }
}

// the layer's pooled texels or attributes of the last resolved pass into a zeroed dense Morton volume (downloads)
__global__ void __launch_bounds__(256)
k_dyn_unpool(const uint32_t* __restrict__ pool, const uint32_t* __restrict__ res_brick, const uint32_t* __restrict__ words,
             int set, uint32_t max_bricks, uint32_t nbricks, uint32_t* __restrict__ dense) {
    const int lane = threadIdx.x & 63;
    const uint32_t used = min(words[VCT_DYN_W_STATS + 8 * set + 1], max_bricks);
    const uint32_t waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t sl = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; sl < used; sl += waves) {
        const uint32_t b = res_brick[sl];
        if (b >= nbricks) continue;
        for (uint32_t v = lane; v < 512u; v += 64) dense[(size_t)b * 512 + v] = pool[(size_t)sl * 512 + v];
    }
}

}  // namespace

// blocks of a grid-stride launch over n units of work: n, at most cap, at least one
static unsigned capped_grid(size_t n, size_t cap) { return (unsigned)(n < cap ? (n ? n : 1) : cap); }

hipError_t vct_launch_assign_slots(const uint32_t* mark, uint32_t* slot, uint32_t* count, uint32_t nbricks, hipStream_t s) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_assign_slots, dim3(capped_grid((nbricks + 255) / 256, 4096)), dim3(256), 0, s, mark, slot, count, nbricks);
    return hipGetLastError();
}

hipError_t vct_launch_slot_bricks(const uint32_t* slot, uint32_t nbricks, uint32_t* slot_brick, hipStream_t s) {
    hipLaunchKernelGGL(k_slot_bricks, dim3(capped_grid((nbricks + 255) / 256, 4096)), dim3(256), 0, s, slot, nbricks, slot_brick);
    return hipGetLastError();
}

hipError_t vct_launch_unpool(const uint32_t* pooled, const uint32_t* brick_slot, uint32_t* dense, uint32_t nbricks, hipStream_t s) {
    hipLaunchKernelGGL(k_unpool, dim3(capped_grid(((size_t)nbricks + 3) / 4, 256 * 32)), dim3(256), 0, s, pooled, brick_slot, dense, nbricks);
    return hipGetLastError();
}

hipError_t vct_launch_vox_plan(const VctVoxParams& p, uint32_t* plan, uint2* frags,
                               int32_t* big_list, bool write, hipStream_t s) {
    if (p.ntri <= 0) return hipSuccess;
    const dim3 grid((p.ntri + 255) / 256), block(256);
    if (write) hipLaunchKernelGGL(k_vox_plan<true>, grid, block, 0, s, p, plan, frags, big_list);
    else hipLaunchKernelGGL(k_vox_plan<false>, grid, block, 0, s, p, plan, frags, big_list);
    return hipGetLastError();
}

hipError_t vct_launch_vox_plan_big(const VctVoxParams& p, const int32_t* big_list, int n_big, uint32_t* plan, uint2* frags,
                                   bool write, hipStream_t s) {
    if (n_big <= 0) return hipSuccess;
    const dim3 grid(capped_grid((size_t)n_big, 256 * 8)), block(256);
    if (write) hipLaunchKernelGGL(k_vox_plan_big<true>, grid, block, 0, s, p, big_list, n_big, plan, frags);
    else hipLaunchKernelGGL(k_vox_plan_big<false>, grid, block, 0, s, p, big_list, n_big, plan, frags);
    return hipGetLastError();
}

static unsigned frag_blocks(uint32_t n) { return capped_grid(((size_t)n + 255) / 256, 256 * 32); }
hipError_t vct_launch_frag_mark(const uint2* frags, uint32_t n, uint32_t* mark, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_frag_mark, dim3(frag_blocks(n)), dim3(256), 0, s, frags, n, mark);
    return hipGetLastError();
}
hipError_t vct_launch_frag_count(const uint2* frags, uint32_t n, const uint32_t* brick_slot, uint32_t* count, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_frag_count, dim3(frag_blocks(n)), dim3(256), 0, s, frags, n, brick_slot, count);
    return hipGetLastError();
}
hipError_t vct_launch_frag_scatter(const uint2* frags, uint32_t n, const uint32_t* brick_slot, const uint32_t* first,
                                   uint32_t* cursor, uint32_t* sorted, uint32_t* slot_brick, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_frag_scatter, dim3(frag_blocks(n)), dim3(256), 0, s, frags, n, brick_slot, first, cursor, sorted,
                       slot_brick);
    return hipGetLastError();
}

hipError_t vct_launch_frag_geom(const VctVoxParams& p, float2* bary, float* falb, hipStream_t s) {
    if (p.nslots == 0u || (!bary && !falb)) return hipSuccess;
    const dim3 grid(capped_grid(p.nslots, 256 * 64)), block(256);
    VctF3* fa = reinterpret_cast<VctF3*>(falb);
    if (bary && falb) hipLaunchKernelGGL((k_frag_geom<true, true>), grid, block, 0, s, p, bary, fa);
    else if (bary) hipLaunchKernelGGL((k_frag_geom<true, false>), grid, block, 0, s, p, bary, fa);
    else hipLaunchKernelGGL((k_frag_geom<false, true>), grid, block, 0, s, p, bary, fa);
    return hipGetLastError();
}

hipError_t vct_launch_tri_nrm(const VctVoxParams& p, uint32_t* tri_nrm, hipStream_t s) {
    if (p.ntri <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tri_nrm, dim3((p.ntri + 255) / 256), dim3(256), 0, s, p, tri_nrm);
    return hipGetLastError();
}

hipError_t vct_launch_voxelize_reference(const VctVoxParams& p, int32_t* big_list, int32_t* big_count,
                                         hipStream_t s) {
    if (p.ntri <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(big_count, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_voxelize_reference, dim3((p.ntri + 255) / 256), dim3(256), 0, s, p, big_list, big_count);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_voxelize_reference_big, dim3(256 * 8), dim3(256), 0, s, p, big_list, big_count);
    return hipGetLastError();
}

hipError_t vct_launch_voxelize(const VctVoxParams& p, hipStream_t s) {
    if (p.nslots == 0u || p.nitems == 0u) return hipSuccess;
    const unsigned blocks = capped_grid(p.nitems, 256 * 64);
    const bool attr = p.stage_albedo != nullptr, falb = p.frag_alb != nullptr;
    const unsigned threads = p.nitems >= VCT_VOX_TINY_BLOCK_ITEMS ? 64u : (p.nitems >= VCT_VOX_SMALL_BLOCK_ITEMS ? 128u : 256u);
    if (attr && falb) hipLaunchKernelGGL((k_voxelize_bricks<true, true>), dim3(blocks), dim3(threads), 0, s, p);
    else if (attr) hipLaunchKernelGGL((k_voxelize_bricks<true, false>), dim3(blocks), dim3(threads), 0, s, p);
    else if (falb) hipLaunchKernelGGL((k_voxelize_bricks<false, true>), dim3(blocks), dim3(threads), 0, s, p);
    else hipLaunchKernelGGL((k_voxelize_bricks<false, false>), dim3(blocks), dim3(threads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.nmulti == 0u) return e;
    const unsigned mblocks = capped_grid(p.nmulti, 256 * 16);
    if (p.stage_albedo) hipLaunchKernelGGL(k_vox_resolve_multi<true>, dim3(mblocks), dim3(256), 0, s, p, p.multi_slot, p.nmulti);
    else hipLaunchKernelGGL(k_vox_resolve_multi<false>, dim3(mblocks), dim3(256), 0, s, p, p.multi_slot, p.nmulti);
    return hipGetLastError();
}

hipError_t vct_launch_dynamic_voxelize(const VctVoxParams& p, const VctDynArgs& d, bool slots_only, hipStream_t s,
                                       const VctDynEmisArgs* emis) {
    if (p.ntri <= 0) return hipSuccess;
    const dim3 grid((p.ntri + 255) / 256), big(capped_grid((size_t)p.ntri, 512)), block(256);
    const bool attr = d.acc_attr != nullptr;
    // the big list is complete when the first launch has ended; every later one reads its length from the device word
    hipLaunchKernelGGL((k_dyn_tris<false, false>), grid, block, 0, s, p, d);
    hipLaunchKernelGGL((k_dyn_big<false, false>), big, block, 0, s, p, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || slots_only) return e;
    if (emis) {
        DynEmisArgs de;
        static_cast<VctDynArgs&>(de) = d;
        de.e = *emis;
        if (attr) {
            hipLaunchKernelGGL((k_dyn_tris<true, true, true>), grid, block, 0, s, p, de);
            hipLaunchKernelGGL((k_dyn_big<true, true, true>), big, block, 0, s, p, de);
        } else {
            hipLaunchKernelGGL((k_dyn_tris<true, false, true>), grid, block, 0, s, p, de);
            hipLaunchKernelGGL((k_dyn_big<true, false, true>), big, block, 0, s, p, de);
        }
        return hipGetLastError();
    }
    if (attr) {
        hipLaunchKernelGGL((k_dyn_tris<true, true>), grid, block, 0, s, p, d);
        hipLaunchKernelGGL((k_dyn_big<true, true>), big, block, 0, s, p, d);
    } else {
        hipLaunchKernelGGL((k_dyn_tris<true, false>), grid, block, 0, s, p, d);
        hipLaunchKernelGGL((k_dyn_big<true, false>), big, block, 0, s, p, d);
    }
    return hipGetLastError();
}

hipError_t vct_launch_dynamic_merge(const VctDynMergeArgs& a, hipStream_t s, unsigned long long* acc_emis) {
    const dim3 grid(capped_grid(((size_t)a.d.max_bricks + 3) / 4, 256 * 32)), block(256);      // one wave per slot
    if (acc_emis) {
        DynEmisMergeArgs ae;
        static_cast<VctDynMergeArgs&>(ae) = a;
        ae.acc_emis = acc_emis;
        if (a.d.acc_attr) hipLaunchKernelGGL((k_dyn_merge<true, true>), grid, block, 0, s, ae);
        else hipLaunchKernelGGL((k_dyn_merge<false, true>), grid, block, 0, s, ae);
        return hipGetLastError();
    }
    if (a.d.acc_attr) hipLaunchKernelGGL(k_dyn_merge<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_dyn_merge<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t vct_launch_dynamic_unpool(const uint32_t* pool, const uint32_t* res_brick, const uint32_t* words, int set,
                                     uint32_t max_bricks, uint32_t nbricks, uint32_t* dense, hipStream_t s) {
    hipError_t e = hipMemsetAsync(dense, 0, (size_t)nbricks * 512 * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_dyn_unpool, dim3(capped_grid(((size_t)max_bricks + 3) / 4, 256 * 32)), dim3(256), 0, s, pool, res_brick,
                       words, set, max_bricks, nbricks, dense);
    return hipGetLastError();
}

hipError_t vct_launch_resolve(const VctResolveArgs& a, int V, bool dense, hipStream_t s) {
    const uint32_t nbricks = (uint32_t)(((size_t)V * V * V) / 512);
    // 4 waves per workgroup, one brick per wave
    hipLaunchKernelGGL(k_resolve_sparse, dim3(capped_grid(((size_t)nbricks + 3) / 4, 256 * 32)), dim3(256), 0, s, a, nbricks,
                       dense ? 1 : 0, nbricks > 524288u ? 1 : 0);
    return hipGetLastError();
}
