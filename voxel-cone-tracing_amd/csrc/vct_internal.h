// vct_internal.h -- shared between the C-ABI translation unit and the kernel files.
#ifndef VCT_INTERNAL_H_
#define VCT_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vct_layout.h"
#include "vct_trace_forms.h"

#if defined(__HIPCC__)
// unorm8 -> float, bit-identical to (float)c / 255.0f for every c in [0,255]: c * RN(1/255) misses for
// 126 of the 256 bytes; the two-term product below never does (tests/test_abi.py).
__device__ __forceinline__ float vct_unorm8_to_float(uint32_t c) {
    const float f = (float)c;
    return fmaf(f, 0x1.010102p-8f, f * -0x1.fdfdfep-33f);
}
// [GL] float -> unorm8, round to nearest
__device__ __forceinline__ uint32_t vct_float_to_unorm8(float f) {
    const float s = f * 255.0f + 0.5f;
    if (!(s > 0.0f)) return 0u;
    if (s >= 255.0f) return 255u;
    return (uint32_t)(int)s;
}
#endif

// ---- material textures (R/Model.h:126-136 loads them, R/Mesh.h:91-108 binds them) ---------------------------
// All textures of a scene live in one packed RGBA8 buffer, each with its mip chain behind level 0 when
// config.texture_mipmaps (glGenerateMipmap, R/Model.h:168).  texture(sampler2D, uv) is restated with the operation
// order of oracle/vct_oracle_raster.cpp: vcto_tex_sample (level 0, BILINEAR, GL_REPEAT) and vcto_tex_sample_lod
// (LINEAR_MIPMAP_LINEAR with the quad differences of the coordinate; oracle/vct_oracle.h "Mip-mapped sampling").
#define VCT_TEX_MAX_LEVELS 15       // 16384 x 16384 down to 1 x 1
struct VctTexDesc {
    uint32_t off;        // first texel of level 0 in the packed buffer
    int32_t w, h;
    uint32_t flags;      // bit 0: some texel has alpha != 255 (fragments need the alpha test of trace.fs:169-172); bit 1: square power of two
    int32_t nlev;        // levels stored (1: level 0 only)
    uint32_t lvl[VCT_TEX_MAX_LEVELS];     // texel offset of level k behind `off`
};
struct VctTextures {
    const uint32_t* texels;    // null: the scene has no textures
    const VctTexDesc* desc;
    const int32_t* mat_tex;    // [nmat][3] diffuse / specular / height texture index or -1
    const float* uv;           // [ntri][3][2]
    int32_t ntex;
    int32_t mips;              // 1: the textures carry mip chains and are sampled with implicit derivatives
};
#if defined(__HIPCC__)
__device__ __forceinline__ int vct_tex_of(const VctTextures& t, int material, int slot) {
    if (!t.texels) return -1;
    const int i = t.mat_tex[3 * (size_t)material + slot];
    return i >= 0 && i < t.ntex ? i : -1;
}
// [GL] bilinear, GL_REPEAT, on one level of W x H texels
__device__ __forceinline__ float4 vct_tex_bilinear(const uint32_t* __restrict__ base, int W, int H, float u, float v) {
    const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    const float a = x - fx, b = y - fy;
    // GL_REPEAT.  An integer remainder by a run-time divisor is ~25 instructions on this GPU and a bilinear tap used to
    // take four: the upper index follows from the lower one ((i + 1) mod n = wrap(i) + 1, or 0 at the end), and a size
    // that is a power of two (most maps) wraps with a mask -- the same integers either way.
    auto wrap = [](int i, int n) {
        if ((n & (n - 1)) == 0) return i & (n - 1);
        const int r = i % n;
        return r < 0 ? r + n : r;
    };
    const int i0 = wrap((int)fx, W), j0 = wrap((int)fy, H);
    const int i1 = i0 + 1 == W ? 0 : i0 + 1, j1 = j0 + 1 == H ? 0 : j0 + 1;
    const uint32_t p00 = base[(size_t)j0 * W + i0], p10 = base[(size_t)j0 * W + i1];
    const uint32_t p01 = base[(size_t)j1 * W + i0], p11 = base[(size_t)j1 * W + i1];
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    float4 o;
#define VCT_TEXCH(ch, sh)                                                                                  \
    o.ch = w00 * vct_unorm8_to_float((p00 >> sh) & 0xffu) + w10 * vct_unorm8_to_float((p10 >> sh) & 0xffu) + \
           w01 * vct_unorm8_to_float((p01 >> sh) & 0xffu) + w11 * vct_unorm8_to_float((p11 >> sh) & 0xffu);
    VCT_TEXCH(x, 0) VCT_TEXCH(y, 8) VCT_TEXCH(z, 16) VCT_TEXCH(w, 24)
#undef VCT_TEXCH
    return o;
}
__device__ __forceinline__ float4 vct_tex_sample(const VctTextures& t, int ti, float u, float v) {
    const VctTexDesc* d = t.desc + ti;
    return vct_tex_bilinear(t.texels + d->off, d->w, d->h, u, v);
}
// log2 without the math library, instruction for instruction oracle/vct_oracle_raster.cpp vcto_log2_det
__device__ __forceinline__ float vct_log2_det(float x) {
    const uint32_t b = __float_as_uint(x);
    int e = (int)(b >> 23) - 127;
    float f = __uint_as_float((b & 0x7fffffu) | 0x3f800000u);
    if (f > 1.41421354f) { f = f * 0.5f; e += 1; }
    const float s = __fdiv_rn(f - 1.0f, f + 1.0f);
    const float s2 = s * s;
    float p = 0.111111112f;
    p = fmaf(p, s2, 0.142857149f);
    p = fmaf(p, s2, 0.2f);
    p = fmaf(p, s2, 0.333333343f);
    p = fmaf(p, s2, 1.0f);
    return fmaf(s * p, 2.88539004f, (float)e);
}
// texture(sampler, (u, v)) with the quad differences (ds_dx, dt_dx, ds_dy, dt_dy) of the normalised coordinate
__device__ __forceinline__ float4 vct_tex_sample_lod(const VctTextures& t, int ti, float u, float v, float ds_dx,
                                                     float dt_dx, float ds_dy, float dt_dy) {
    const VctTexDesc* d = t.desc + ti;
    const int W = d->w, H = d->h, nlev = d->nlev;
    const uint32_t* base = t.texels + d->off;
    const uint32_t dflags = d->flags;
    // Texel offset of level k behind level 0.  A square power-of-two map stores W^2 (1 + 1/4 + ... ) texels in front of
    // level k = 4/3 (W^2 - W^2 / 4^k): the difference is a multiple of 3, so the division is one multiply by the inverse
    // of 3 modulo 2^32 -- the same integers as the table, without the round trip that depended on k.
    auto level_offset = [&](int k) -> uint32_t {
        if (dflags & 2u) {
            const uint32_t wh = (uint32_t)W * (uint32_t)W;
            return ((wh - (wh >> (2 * k))) << 2) * 0xaaaaaaabu;
        }
        return d->lvl[k];
    };
    if (!t.mips || nlev <= 1) return vct_tex_bilinear(base, W, H, u, v);
    const float du_dx = ds_dx * (float)W, dv_dx = dt_dx * (float)H;
    const float du_dy = ds_dy * (float)W, dv_dy = dt_dy * (float)H;
    const float ax = du_dx * du_dx + dv_dx * dv_dx, ay = du_dy * du_dy + dv_dy * dv_dy;
    const float m = ax > ay ? ax : ay;
    if (!(m > 1.0f)) return vct_tex_bilinear(base, W, H, u, v);                     // magnification (and NaN)
    const float lam = 0.5f * vct_log2_det(m);
    const int q = nlev - 1;
    if (lam >= (float)q) return vct_tex_bilinear(base + level_offset(q), max(1, W >> q), max(1, H >> q), u, v);
    const int k = (int)lam;
    const float f = lam - (float)k, g = 1.0f - f;
    const float4 t1 = vct_tex_bilinear(base + level_offset(k), max(1, W >> k), max(1, H >> k), u, v);
    const float4 t2 = vct_tex_bilinear(base + level_offset(k + 1), max(1, W >> (k + 1)), max(1, H >> (k + 1)), u, v);
    float4 o;
    o.x = fmaf(f, t2.x, g * t1.x); o.y = fmaf(f, t2.y, g * t1.y);
    o.z = fmaf(f, t2.z, g * t1.z); o.w = fmaf(f, t2.w, g * t1.w);
    return o;
}
#endif

// ---- shadow map words (R/Voxel_Cone_Tracing.h:79-105 keeps a DEPTH_COMPONENT24 texture) ----------------------------
// The map is stored as the very words the shadow pass's atomicMin leaves behind: the fp32 bits of the depth, already
// quantised to 24 bits ([GL] fixed-point depth: float(round(z * (2^24 - 1)) / (2^24 - 1)), in [0, 1] so <= 0x3f800000),
// plus an EPOCH in the two top bits: pass n writes with epoch 3 - (n & 3).  Positive floats order like their bit
// patterns and a lower epoch is a smaller word, so a new pass simply overwrites what older passes left (no clear, no
// conversion pass: the buffer is memset once every fourth pass, when the epoch wraps); a reader subtracts the pass's
// epoch base and clamps -- words of older passes and never-written ones (all ones) come out as depth 1.0, the
// cleared depth buffer.  Two VALU per texel instead of a 192 MiB conversion pass per shadow map.
#define VCT_SHADOW_ONE 0x3f800000u
#define VCT_SHADOW_EPOCH(e) ((uint32_t)(e) << 30)
#if defined(__HIPCC__)
__device__ __forceinline__ float vct_shadow_depth(uint32_t word, uint32_t ebase) {
    const uint32_t v = word - ebase;
    return __uint_as_float(v < VCT_SHADOW_ONE ? v : VCT_SHADOW_ONE);
}
// [GL] DEPTH_COMPONENT24: z in [0, 1) -> float(q / (2^24 - 1)), q = floor(z * (2^24 - 1) + 0.5) in double exactly as
// the oracle computes it (the product is exact in double, so the fma is the same single rounding as mul + add);
// float(q) / 16777215.0f (IEEE) equals float(double(q) / 16777215.0) for every q (tests/test_oracle_kat.py).
__device__ __forceinline__ uint32_t vct_depth24_bits(float z) {
    const uint32_t q = (uint32_t)floor(fma((double)z, 16777215.0, 0.5));
    return __float_as_uint(__fdiv_rn((float)q, 16777215.0f));
}
#endif

// PCF short cut.  A tap is a convex combination of four depths of the 6 x 6 window, so it lies between the window's
// smallest and largest depth -- up to rounding: the four weights are products of (a, 1 - a) x (b, 1 - b), each within
// 3 ulp of the exact product, and the four-term sum adds at most 4 more (mul + add or fma chain alike), so every tap of
// the window is within a factor 1 +- 2^-21 of [dmin, dmax].  With margins of 2^-19: when the compared depth is
// <= dmin * (1 - 2^-19) all 25 taps pass, when it is > dmax * (1 + 2^-19) none does -- and only a window the shadow
// boundary crosses pays for the 25 bilinear taps (~330 of the shade kernel's ~1200 instructions per pixel, the larger
// part of the voxelizer's per-fragment work).  Raw words order like their depths (an older epoch or a never-written
// word is larger than every word of the current pass and decodes to 1.0), so the minimum / maximum are taken on the
// words.  Returns 25 / 0, or -1: evaluate the taps.
#if defined(__HIPCC__)
__device__ __forceinline__ int vct_pcf_window_verdict(uint32_t wmin, uint32_t wmax, uint32_t ebase, float cur) {
    const float lo = vct_shadow_depth(wmin, ebase) * 0.999998f, hi = vct_shadow_depth(wmax, ebase) * 1.000002f;
    return cur <= lo ? 25 : (cur > hi ? 0 : -1);
}
// The same verdict from the tile table: (col0, row0) = first texel of a regular (unclamped, six consecutive texels per
// axis) window.  Tile (tx, ty) holds the bounds of texels [8 tx, 8 tx + 13) x [8 ty, 8 ty + 13) -- every window that
// STARTS in the tile lies inside that region -- so one 8-byte load bounds the window from outside.  -1: undecided.
#define VCT_SHADOW_TILE_SHIFT 3
#define VCT_SHADOW_TILE_REACH 5      // a window spans 6 texels: it ends at most 5 texels beyond the tile it starts in
__device__ __forceinline__ int vct_pcf_tile_verdict(const uint2* __restrict__ tiles, int S, uint32_t col0, uint32_t row0, float cur) {
    const uint32_t nb = ((uint32_t)S + 7u) >> VCT_SHADOW_TILE_SHIFT;
    const uint2 t = tiles[(row0 >> VCT_SHADOW_TILE_SHIFT) * nb + (col0 >> VCT_SHADOW_TILE_SHIFT)];
    return cur <= __uint_as_float(t.x) * 0.999998f ? 25 : (cur > __uint_as_float(t.y) * 1.000002f ? 0 : -1);
}
#endif

// Six consecutive shadow-map words (one row of a PCF window) as ONE dwordx4 + ONE dwordx2 load: the row starts at any
// 4-byte boundary (gfx950 under HSA runs with unaligned vector access enabled, and hipcc emits the wide loads for this
// packed type).  The PCF gathers are bound by the number of load instructions the texture-address unit has to spread
// over cache lines (36 dword loads per fragment: 70 of the voxelizer's 100 us at configs[1]), not by bytes.
struct __attribute__((packed, aligned(4))) VctWords6 { uint32_t v[6]; };
// The nine floats of one triangle in a per-vertex attribute array ([ntri][3][3]: 36 B records at 4-byte alignment) as
// dwordx4 + dwordx4 + dword instead of nine dword loads -- same reason.
struct __attribute__((packed, aligned(4))) VctTri9 { float v[9]; };

#define VCT_BIN_CSTRIDE 32          // words between the counters of two bins (vct_raster.hip)
#define VCT_BIN_HUGE_CAP 1024u      // records the tile-binned raster lets every bin scan (vct_raster.hip k_bin_setup)
#define VCT_NO_SLOT 0xffffffffu
#define VCT_TILE 8
#define VCT_TILE_PIX 64
#define VCT_GB_NPLANES 23
#define VCT_MAX_STEPS 1024
// Executed steps.  The screen trace STORES each tile's count into its own slot, tile_steps[tile] (frame-wide tile
// index; the tile's waves add theirs in LDS and the last one to arrive stores the sum): no global atomic, nothing to
// zero between launches, and the host gets the total (sum over the launched rows) as well as the per-tile-row cost
// histogram (vct_last_row_steps: load-aware slabs) from the same words.  (Device-scope atomicAdd into a shared bank
// cost 2.5 % of the trace when neighbouring tiles shared addresses.)  The bounce kernels, whose waves loop over many
// voxels, keep a small bank of atomic counters.
#define VCT_STEP_COUNTERS 256   // bounce kernels only (power of two)

// One texel buffer per wave serves every level of a chain whose levels all start below 4 GiB: the level's byte offset
// goes into the load's scalar offset operand (vct_trace.hip ChainRef; the CHAIN forms of the default trace kernel).  A
// chain with a level at or beyond 4 GiB (1024^3: level 1 starts at byte 2^32) has no such offset.
static inline bool vct_chain_form_fits(int V) { return vct_level_offset(V, vct_ilog2(V)) < (1ull << 30); }

// One entry per march step of a cone aperture.  The step sequence of trace.fs:90-104 (dist,
// diameter, lod) does not depend on the pixel, only on (V, G, tanHalfAngle, MAX_DISTANCE): the
// host evaluates it once with the reference's operation order and the kernel reads it through
// the scalar cache.
struct VctLevelRef {    // one mip level as the sampler needs it (all wave-uniform)
    uint32_t off;      // texel offset of the level in the chain
    uint32_t mask_x;   // x bits of the level's Morton index: 0x09249249 & (N^3 - 1)
    float fN;          // N = V >> level, as float
    int32_t m;         // N - 1
};

// The verified constant division of the march (vct_trace.hip div_const<1>): the two-term product
// fma(x, r_hi, x * r_lo) with r_hi + r_lo = 1/d to ~48 bits (2 VALU).  It is exact only for divisors the device has
// checked over every fp32 input.
// second argument of div_const<1> for divisor d with r = RN(1 / d): the low word of the reciprocal
static inline float vct_div_aux(float d, float r) {
    return (float)(1.0 / (double)d - (double)r);
}
struct VctStep {       // 64 B: one s_load_dwordx16 per march step
    float dist;        // trace.fs:91,103
    float occ_rcp;     // RN(1 / occ_den): reciprocal for the exact constant division (vct_trace.hip)
    float occ_den;     // 1 + 0.03*diameter            trace.fs:101 -- or, in a table built for the verified two-term
                       // division (vct_capi.hip refresh_steps), the low word r_lo of its reciprocal
    float frac;        // fract(lod) after [GL] clamp  trace.fs:97
    int32_t level;     // floor(lod)
    int32_t level2;    // min(level+1, maxLevel)
    int32_t two_levels;  // lod > 0 (minification) and frac != 0: blend level/level2; else `level` only
    float omf;         // 1 - frac (the level blend's other factor: one VALU per step less than computing it per lane)
    VctLevelRef l1, l2;
};

// Gloss classes on the device (include/vct.h "per-material gloss"): the class headers -- count, march steps and Phong
// exponent of each class -- in front of one step table per class, each built as the specular table is.  One allocation
// behind one pointer of VctTraceParams: the specular wave reads a header entry and a table through the constant address
// space with a wave-uniform class index (scalar loads, as it reads steps_specular), the composite reads its lane's
// exponent with one vector load.
struct VctGlossTable {
    int32_t nclasses;
    int32_t pad0[3];
    int32_t nsteps[8];
    float shininess[8];
    int32_t pad1[12];                   // the tables start 128 B in
    VctStep steps[8][VCT_MAX_STEPS];
};

#define VCT_COMP_GROUPS_SHIFT 8
#define VCT_COMP_AOV_SHIFT 16
#define VCT_COMP_ON 0x80000000u
#define VCT_COMP_EMISSION 0x40000000u   // the launch has pixel-emission planes (VctTraceParams::pix_emis): the composite adds them
struct VctTraceParams {
    const uint32_t* chain;              // Morton chain, RGBA8 packed
    uint32_t level_off[VCT_MAX_LEVELS]; // texel offsets
    int32_t V, nlev;
    float G, half_G, vs;
    float half_G_rcp;                   // RN(1 / half_G)
    float half_G_aux;                   // what div_const takes beside it: half_G, or (fast_div) the low word of 1 / half_G
    int32_t fast_div;                   // 1: every constant divisor admits the FMA-corrected division
    float cam[3];
    float light[3];
    float light_unit[3];                // normalize(light), the composite's L (vct_tilediv.h vct_light_unit): set by vct_launch_trace
    float ambient, shininess, max_alpha;
    int32_t wrap_repeat;
    const uint32_t* spread_lut;         // [1024] spread3(i) << 2: dilated byte offsets of an x coordinate (scalar loads)
    // footprint records of the levels >= 1 (vct_volume.hip k_build_cells), biased so that the record of Morton index c of
    // the level at texel offset `off` sits at cells_biased + (off + c) * 32; null: per-texel gathers everywhere
    const char* cells_biased;
    const VctStep* steps_diffuse;
    const VctStep* steps_specular;
    int32_t n_diffuse, n_specular;
    int32_t width, height, tiles_x, tiles_y;
    int32_t tile_row0, tile_row1;       // slab [row0,row1)
    // Interleaved slabs (vct_multi.hip): of the rows [row0, row1) only every row_stride-th is traced, starting with row0
    // (0 / 1: all of them); pack_rows = 1 writes traced row j to pixel rows 8j .. 8j+7 of `out` (a rank's packed slab of
    // an interleaved frame) instead of the row's own place in the frame.  k_trace_tile_split only.
    int32_t row_stride, pack_rows;
    int32_t ntiles;                     // tiles of this launch (rows traced x tiles_x): set by vct_launch_trace
    int32_t spec_prio;                  // 1: the specular waves raise their issue priority (slab launches, vct_trace.hip)
    uint32_t tile_mul, tile_shift;      // tile / tiles_x without a division (vct_tilediv.h): set by vct_launch_trace
    const float* gbuf;                  // tiled [tile][23][64]
    uint16_t* out;                      // RGBA16F [h][w][4]
    uint8_t* dbg_steps;                 // [npix][7] or null
    float* dbg_cones;                   // [npix][7][4] or null
    unsigned long long* step_counter;   // [VCT_STEP_COUNTERS] bounce kernels: partial sums of executed steps (zero at launch)
    uint32_t* tile_steps;               // [tiles] screen trace: executed steps of each tile (stored, not added)
    unsigned long long* stats;          // [32] wave-level march counters (builds with -DVCT_STATS=1 only)
    // second bounce (k_bounce): per-voxel attributes (pooled like the accumulators: [slot][512]), touched-brick
    // flags, output level 0
    // The five of them are read by the bounce kernels only and the dr_* beside them by the screen trace only (half-rate
    // diffuse gather: vct_set_diffuse_rate(ctx, 2), include/vct.h; vct_trace.hip k_point_march / k_diffuse_resolve /
    // k_trace_tile_split's SF_HALF forms; dr_ind != null in a screen trace's parameters selects it).  They share their
    // slots for the reason bounce_out and aov do.
    union { const uint32_t* attr_albedo;
            float4* dr_ind; };          // [h][w] the gather every pixel's composite takes (anchor, interpolated or fill)
    union { const uint32_t* attr_normal;
            float4* dr_coarse; };       // [ch][cw] the gather of each 2x2 quad's anchor, cw = ceil(w / 2), ch = ceil(h / 2)
    union { const uint32_t* brick_slot;
            uint8_t* dr_anchor; };      // [ch][cw] the anchor's place in its quad, j * 2 + i, or VCT_DR_NO_ANCHOR
    union { const uint32_t* brick_prev;
            uint32_t* dr_list; };       // [w * h] fill pixels (y * w + x) in no particular order
    // bounce_seen: bricks the bounce chain showed when its mips were last built
    // dr_ctr: counters of one half-rate pass, zeroed by its first launch: [0, VCT_DR_COUNTERS) executed steps of the coarse
    // and the listed march, [VCT_DR_COUNTERS, 2 VCT_DR_COUNTERS) pixels they marched, [2 VCT_DR_COUNTERS] entries of dr_list
    union { const uint32_t* bounce_seen;
            unsigned long long* dr_ctr; };
    // bounce_out is written by the bounce kernels only, aov read by the screen trace only: they share the slot, so the
    // screen trace's parameter block keeps its size (and the default kernels their code) with the lighting components
    union {
        uint32_t* bounce_out;
        uint16_t* aov;                  // per-component outputs (below): the frames that are on, back to back in bit order
    };
    uint32_t nbricks;
    // Lighting components (vct_set_lighting_components / vct_set_aov_outputs; k_trace_tile_split's SF_COMP forms, launched
    // when comp != 0): bits 0-4 the VCT_SHOW_* mask, bits 8-9 the cone groups marched (1: cones 0-5, 2: cone 6), bits
    // 16-18 the VCT_AOV_* outputs written to `aov`, bit 30 VCT_COMP_EMISSION, bit 31 set.  (It fills the padding in front of slot_brick.)
    uint32_t comp;
    // slot_brick is the bounce kernels', sky the screen trace's and the point queries' (include/vct.h "sky light"; the SKY
    // forms of k_trace_tile_split, k_point_march and k_query_march, launched when sky != null): one slot, for the reason
    // bounce_out and aov share theirs
    union { const uint32_t* slot_brick; // [nslots] the bricks a fragment of the mesh can land in (the voxelizer's slots)
            const float* sky; };        // [9][3] folded polynomial coefficients of the attached sky (vct_sky_check.h vct_sky_fold)
    uint32_t nslots;
    // anisotropic option: six directional chains (levels >= 1), Morton per level, each
    // `aniso_stride` texels; level k of a direction at texel offset level_off[k] - level_off[1]
    const uint32_t* aniso;
    uint32_t aniso_stride;
    uint32_t aniso_alt_slab;            // float4 offset from a level's LDS slab to its second ("-axis") slab
    // bounce_list / bounce_list_count are the bounce kernels', gloss / pix_gloss the screen trace's (include/vct.h
    // "per-material gloss"; k_trace_tile_split's SF_GLOSS forms, launched when pix_gloss != null): they share their slots
    // for the reason bounce_out and aov do
    union { uint32_t* bounce_list;      // global list of occupied voxels (Morton indices), brick by brick
            const VctGlossTable* gloss; };   // the class headers and one step table per class
    union { uint32_t* bounce_list_count;
            const uint8_t* pix_gloss; };     // pixel-gloss plane, tiled [tile][64]: a byte b means class (b < nclasses ? b : 0)
    union { uint32_t bounce_list_cap;
            int32_t dr_waves; };        // (half-rate pass) waves per 64 marched points: 1, or 2 with three cones each
    // brick_over is the bounce kernels', pix_emis the screen trace's: one slot, for the reason bounce_out and aov share theirs
    union { uint32_t* brick_over;       // bricks whose voxels did not fit the list
            const float* pix_emis; };   // pixel-emission planes, tiled [tile][3][64] (include/vct.h "emissive materials"); read when comp has VCT_COMP_EMISSION
    // Live-pixel compaction (config.trace_variant = 4; vct_trace.hip k_compact_tiles): the live pixels (albedo.a >= 0.5)
    // of every 16x16-pixel super-tile packed into whole waves.  vt_pix[v * 64 + lane] = tile << 6 | pixel of the tile
    // (all ones: no pixel), vt_count[0] = virtual tiles.  Null: lane = pixel of the launched tile.
    uint32_t* vt_pix;
    uint32_t* vt_count;
    // 1: every level of `chain` starts below 4 GiB and the context takes the kernels' CHAIN forms (vct_chain_form_fits,
    // vct_ctx chain_form).  Read by the launch dispatch, by no kernel.
    int32_t chain_form;
};
// What a newer form of a kernel needs beside it rides in a second argument struct (VctQueryArgs, VctBounceDynArgs): this
// one neither grows nor moves, so the kernels every existing launch takes keep their argument block and their code.
#define VCT_TRACE_PARAMS_BYTES 424
static_assert(sizeof(VctTraceParams) == VCT_TRACE_PARAMS_BYTES, "VctTraceParams neither grows nor moves");
#define VCT_DR_NO_ANCHOR 0xffu
#define VCT_DR_COUNTERS 256             // (power of two) a bank, for the reason VCT_STEP_COUNTERS is one
#define VCT_DR_CTR_WORDS (2 * VCT_DR_COUNTERS + 1)

// Point queries (include/vct.h "point queries"; vct_trace.hip k_query_march): what a query launch needs beside the march's
// part of VctTraceParams (vct_fill_march_params), as a second kernel argument -- VctTraceParams keeps its layout.
#define VCT_QUERY_GATHER 0
#define VCT_QUERY_CONE 1
#define VCT_QUERY_KEY_BITS 28           // sort key: bits 0-2 octant, 3-26 Morton code of the start point's cell, bit 27 non-finite
struct VctQueryArgs {
    const float* pts;                   // [n] vct_gather_point (12 floats) or vct_cone_point (9 floats), 4-byte aligned
    const uint32_t* index;              // [n] the order the points are marched in (VCT_QUERY_SORT_CELLS) or null: as given
    float* out;                         // [n][4] gather / cone, at the caller's index
    float* out_cones;                   // [n][6][4] or null (gather)
    uint8_t* out_steps;                 // [n][6] (gather) / [n] (cone) or null
    unsigned long long* ctr;            // [VCT_DR_COUNTERS] partial sums of executed steps (zero at launch)
    uint32_t n;
    int32_t specular;                   // (cone) 1: the specular step table, 0: the diffuse one
};
// marches q.n points; kind: VCT_QUERY_GATHER / _CONE.  p: vct_fill_march_params' fields only
hipError_t vct_launch_query(const VctTraceParams& p, const VctQueryArgs& q, int kind, hipStream_t s);
// keys[i] = sort key of point i (VCT_QUERY_KEY_BITS bits), index[i] = i
hipError_t vct_launch_query_keys(const VctTraceParams& p, const VctQueryArgs& q, int kind, uint32_t* keys, uint32_t* index, hipStream_t s);

#ifndef VCT_VOX_CHUNK
#define VCT_VOX_CHUNK 4096u       // most fragments one work item (workgroup) of the voxelize pass takes (vct_capi.hip build_voxel_slots)
#endif
struct VctVoxParams {
    int32_t V;
    float G, model_scale;
    const float* pos;          // [ntri][9]
    const int32_t* material;   // [ntri]
    const float* albedo;       // [nmat][4]
    int32_t ntri;
    const uint32_t* shadow;    // [S*S] shadow-map words (vct_shadow_depth) or null
    uint32_t shadow_ebase;     // epoch base of the pass that produced them
    int32_t shadow_size;
    const uint2* shadow_tiles; // [ceil(S/8)]^2 decoded (min, max) per dilated 8 x 8 tile (vct_launch_shadow_minmax) or null
    float light_vp[16];
    // Per brick the uploaded mesh can touch (found once per mesh) there is a SLOT: brick_slot maps brick -> slot
    // (VCT_NO_SLOT: no fragment ever lands there).  A 1024^3 grid costs the surface, not 16 GiB.
    // North-star mode: the fragments of the mesh sorted by slot (frag_sorted[slot_first[s] .. slot_first[s + 1]),
    // entry = triangle << 9 | voxel inside the brick), accumulated in LDS by one workgroup per slot and resolved into
    // stage[slot][512] (+ the voxel attributes).  Reference mode: acc[nslots][512][2] in HBM, (triangle + 1) << 32 | rgb
    // by atomicMax.
    unsigned long long* acc;   // [nslots][512][2] (reference mode)
    const uint32_t* brick_slot;   // [V^3 / 512]
    uint32_t* brick_mark;      // mark_only (reference mode, at upload): bricks a fragment lands in
    int32_t mark_only;
    const uint32_t* frag_sorted;  // [nfrag]
    // light-independent per-fragment values, written by k_frag_geom: the fragment's clamped barycentrics (b0, b1) -- once
    // per mesh -- and, in a scene with textures, its albedo (once per change of the textures / texture coordinates)
    const float2* frag_bary;      // [nfrag]
    const float* frag_alb;        // [nfrag][3] or null (no textures: the material's colour is read per fragment)
    const uint32_t* tri_qnrm;     // [ntri][3] quantised front-face normal (voxel attributes) or null
    const uint32_t* slot_first;   // [nslots + 1]
    const uint32_t* slot_brick;   // [nslots]
    uint32_t nslots;
    // Work items of the pass: a slot's fragments in chunks of at most VCT_VOX_CHUNK, one workgroup per chunk, heaviest
    // slots first (built on the host once per mesh).  A slot of one chunk is accumulated and resolved in LDS; the chunks of a
    // larger one add their LDS partial sums to the slot's accumulators in HBM (acc2: [multi][512][2], acc2_attr:
    // [multi][512][3]); a second small kernel resolves those slots (multi_slot[multi]) and re-zeroes the accumulators.
    const uint4* items;        // [nitems] (slot, first fragment, fragments, index among the multi-chunk slots or ~0)
    uint32_t nitems;
    unsigned long long* acc2;
    unsigned long long* acc2_attr;
    const uint32_t* multi_slot;
    uint32_t nmulti;
    uint32_t* stage;           // [nslots][512] resolved RGBA8 of the pass (Morton order inside the brick)
    uint32_t* stage_albedo;    // [nslots][512] or null (config.voxel_attributes)
    uint32_t* stage_normal;
    uint32_t* brick_flags;     // [V^3 / 512] raised for bricks written by a pass, consumed by the sparse resolve
    float proj[48];            // ProjX, ProjY, ProjZ (VCT.h:128-134), column-major; reference mode only
    VctTextures tex;           // diffuse textures + texture coordinates (vox.fs:56); texels == null: flat colours
};

// what the sparse resolve of vct_inject_light reads and writes (vct_voxelize.hip k_resolve_sparse)
struct VctResolveArgs {
    uint32_t* level0;                // [V^3] Morton
    uint32_t* flags;                 // [V^3 / 512] bricks written by the pass (consumed) ...
    uint32_t* prev;                  // ... and by the pass before it (updated)
    const uint32_t* brick_slot;      // [V^3 / 512]
    // north-star mode: the staging pool of the pass, [nslots][512] each; the attribute pair is null without
    // config.voxel_attributes and is copied into the context's pooled attributes.  stage == null: reference mode
    const uint32_t* stage;
    const uint32_t* stage_albedo;
    const uint32_t* stage_normal;
    uint32_t* attr_albedo;
    uint32_t* attr_normal;
    unsigned long long* acc;         // reference mode: [nslots][512][2] last-writer words (re-zeroed)
    // north-star mode with emissive materials: the emission pool, [nslots][512] RGBA8 like `stage`, added to the staged
    // texel per byte with saturation (include/vct.h "emissive materials"); null: the staged texel as it is
    const uint32_t* emis;
};

// inputs of the raster stages (vct_raster.hip); all device pointers
struct VctRasterArgs {
    const float* pos;            // [ntri][9] model space
    const float* nrm;            // [ntri][9] per-vertex normal / tangent / bitangent (G-buffer only)
    const float* tan;
    const float* bit;
    const int32_t* material;     // [ntri]
    const int32_t* tri_alpha;    // [ntri] alpha-test class of the triangle (vct_raster.hip k_tri_alpha) or null
    const float* albedo;         // [nmat][4]
    const float* specular;       // [nmat][3]
    const float* emission;       // [nmat][4] material emission (rgb, pad) or null (G-buffer shade: the pixel-emission planes)
    const uint8_t* mat_gloss;    // [nmat] gloss class per material or null (G-buffer shade: the pixel-gloss plane)
    int32_t ntri;
    float model_scale;
    // Visibility words: 64-bit (depth | id) of the main draw, W*H; 32-bit depth-only of the shadow pass, S*S.
    // Invariant between passes: every word is all-ones ("empty") -- the consumer of a word resets it.
    unsigned long long* vis;
    uint32_t* vis32;             // = the shadow-map words of the context
    uint32_t vis32_ebase;        // epoch base this shadow pass writes with
    int32_t* wave_list;          // [2*ntri] medium sub-triangles
    uint32_t* wave_count;
    int32_t* group_list;         // [2*ntri] small-medium sub-triangles (one 16-lane group each)
    uint32_t* group_count;
    uint2* items;                // tile work items of huge sub-triangles
    uint32_t* item_count;
    uint32_t item_capacity;
    uint32_t* next_counts;       // [3] the other counter set (item, wave, group): zeroed by this pass for the next
    void* recs;                  // [2 * ntri] 96-byte set-up records of the listed sub-triangles (vct_raster.hip SubTriRec)
    VctTextures tex;             // material textures + texture coordinates (G-buffer pass)
    // Tile-binned visibility (vct_raster.hip "Tile-binned visibility"; binned == 0: the direct form above).  Scratch of
    // one pass kind: records, (bin, record) pairs, per-bin entry ranges, work items, the list of huge records, and two
    // alternating sets of eight counters (a pass zeroes the other set; bin_count is left zero by k_bin_alloc).
    int32_t binned;
    void* bin_recs;              // [bin_rec_cap] 160-byte BinRec
    uint32_t bin_rec_cap;
    uint2* bin_entries;          // [bin_entry_cap] one per (sub-triangle, 16x16 bin) overlap
    uint32_t bin_entry_cap;
    uint32_t* bin_count;         // [bins * VCT_BIN_CSTRIDE] (a bin's counter has a cache line to itself)
    uint32_t* bin_cursor;        // [bins * VCT_BIN_CSTRIDE]
    uint4* bin_items;            // [bin_item_cap]
    uint32_t bin_item_cap;
    uint32_t* bin_huge;          // [bin_huge_cap]
    uint32_t bin_huge_cap;
    uint32_t* bin_ctr;           // [8] this pass's counters
    uint32_t* bin_next_ctr;      // [8] the next pass's
};

hipError_t vct_launch_shadow_raster(const VctRasterArgs& a, const float light_vp[16], int S, hipStream_t s);
// float depths in [0, 1] <-> shadow-map words (uploads of maps made elsewhere, downloads)
hipError_t vct_launch_shadow_encode(const float* depth, uint32_t* words, size_t n, uint32_t ebase, hipStream_t s);
hipError_t vct_launch_shadow_decode(const uint32_t* words, float* depth, size_t n, uint32_t ebase, hipStream_t s);
// Depth bounds of the shadow map per 8 x 8-texel tile, each over the tile DILATED by the reach of a PCF window (13 x 13
// texels; decoded words: monotonic in depth), rebuilt after a pass / upload: [ceil(S / 8)]^2 (min, max) pairs.  Where the
// compared depth lies outside the bounds of the tile a window starts in, all 25 taps pass or fail
// (vct_pcf_window_verdict's margins hold for any superset of the window) and the window is never fetched.
hipError_t vct_launch_shadow_minmax(const uint32_t* words, uint32_t ebase, int S, uint2* tiles, hipStream_t s);
// tile rows [row0, row1) only (whole frame: 0 .. ceil(H/8)); visibility (k_raster_vis + k_raster_mid) and shading
// (k_gbuffer_shade, the only part that reads the shadow map) are separate calls so that a stream wait can sit between
hipError_t vct_launch_gbuffer_visibility(const VctRasterArgs& a, const float view_proj[16], int W, int H, int row0, int row1,
                                         hipStream_t s);
// `dyn` not null: the pass drew the dynamic mesh into a second visibility buffer (vct_launch_dynamic_visibility) and the
// DYN instantiation of the shade kernel resolves the two words of every pixel (include/vct.h "dynamic mesh", drawing)
struct VctDynShadeArgs {
    unsigned long long* vis;     // [H][W] second visibility buffer, ids from 0
    const float* pos;            // [ntri][9] draw copy of the positions
    const float* nrm;            // [ntri][9] face frame at all three vertices
    const float* tan;
    const float* bit;
    const int32_t* material;     // [ntri]
    const float* albedo;         // [nmat][4] (rgb used; the alpha plane is 1)
    float specular[3];           // the constant of vct_set_dynamic_draw
    const float* emission;       // [nmat][4] the table of vct_set_dynamic_emission or null: dynamic pixels emit 0
};
hipError_t vct_launch_gbuffer_shade(const VctRasterArgs& a, const float view_proj[16], int W, int H, int row0, int row1,
                                    const uint32_t* shadow, uint32_t shadow_ebase, int shadow_size, const uint2* shadow_tiles,
                                    const float light_vp[16], float* tiled, float* emis_tiled, uint8_t* gloss_tiled, hipStream_t s,
                                    const VctDynShadeArgs* dyn = nullptr);
// The dynamic mesh's own visibility pass of the main draw: the direct form over a.pos (the draw copy) into a.vis (the
// second buffer) with the scratch in `a`, no material -- no alpha test -- and the scissor rows of the static pass.
hipError_t vct_launch_dynamic_visibility(const VctRasterArgs& a, const float view_proj[16], int W, int H, int row0, int row1,
                                         hipStream_t s);
// k_dyn_draw_prepare, one thread per dynamic triangle: the draw copy of `pos` (a triangle with a coordinate v for which
// !(fabsf(v * model_scale) <= vertex_limit) becomes nine zeros -- a point, culled by the set-up) and the face frame
// (u, t, b) = vct_import_frame(cross(p1 - p0, p2 - p0)), written to all three vertices of draw_nrm / _tan / _bit.
// corner_nrm not null (include/vct.h "dynamic mesh", Normals): the NRM instantiation of the same kernel, which reads the
// triangle's corner normals, moves them with a mover's matrices and writes vct_import_corner_frame per corner.  (Host
// side only: the kernels take the members one by one, and the forms without normals take what they always took.)
struct VctDynPrepare {
    float model_scale, vertex_limit;
    float *draw_pos, *draw_nrm, *draw_tan, *draw_bit;      // [ntri][9] each
    const float* corner_nrm;                               // [ntri][3][3], or null: face frames
};
hipError_t vct_launch_dynamic_draw_prepare(const float* pos, int32_t ntri, const VctDynPrepare& prepare, hipStream_t s);
// Parts of the dynamic mesh (include/vct.h "dynamic mesh", Parts): pos[t] = the rest triangle t moved by the 3 x 4 matrix
// table[3 * part[t] ..].  part[t] was checked on the host; the table is the library's own allocation, so its rows are
// 16-byte aligned.  (This struct and the skin's are kernel arguments: their layout is the kernels' scalar loads.)
struct VctDynPartsArgs {
    const float* rest;           // [ntri][9]
    const int32_t* part;         // [ntri] in 0 .. nparts-1
    const float4* table;         // [nparts][3] rows of the matrices
    float* pos;                  // [ntri][9] the layer's current positions
};
// A skin of the dynamic mesh (include/vct.h "dynamic mesh", Skin): pos[t] = the rest triangle t, each corner moved by
// the blend of four rows of the table with the corner's four weights.  The indices were checked on the host against the
// table's rows and packed; all four arrays are the library's own.
struct VctDynSkinArgs {
    const float* rest;           // [ntri][9]
    const uint16_t* bone;        // [ntri][3][4] in 0 .. nbones-1
    const float* weight;         // [ntri][3][4]
    const float4* table;         // [nbones][3] rows of the matrices
    float* pos;                  // [ntri][9] the layer's current positions
};
// The attached mover's update, one thread per triangle: the arguments of its kind (host side only; a kernel takes the
// one that is in use) into k_dyn_move, or -- `prepare` not null -- into the kind's instantiation of k_dyn_draw_prepare,
// which stores the positions and goes on to the draw copy and the frames in the same launch.
struct VctDynMoverArgs {
    bool is_skin;
    VctDynPartsArgs parts;       // !is_skin
    VctDynSkinArgs skin;         // is_skin
};
hipError_t vct_launch_dynamic_move(const VctDynMoverArgs& a, int32_t ntri, const VctDynPrepare* prepare, hipStream_t s);
// one level of a texture's mip chain from its parent (pw x ph -> w x h), glGenerateMipmap restated as in the oracle
hipError_t vct_launch_tri_alpha(const VctRasterArgs& a, int32_t* out, hipStream_t s);
hipError_t vct_launch_tex_mip(const uint32_t* parent, int pw, int ph, uint32_t* level, int w, int h, hipStream_t s);
// vct_planes.hip: linear planes [nplanes][h*w] <-> tiled [tile][nplanes][64] of `elem`-byte elements (pixels outside the
// frame are tiled as 0), for the kinds of planes a frame slot has: 23 floats (the G-buffer), 3 floats (pixel-emission and
// lit planes), 1 byte (the pixel-gloss plane); any other kind is hipErrorInvalidValue
#define VCT_EMIS_NPLANES 3
hipError_t vct_launch_tile_planes(const void* linear, void* tiled, int nplanes, size_t elem, int w, int h, hipStream_t s);
hipError_t vct_launch_untile_planes(const void* tiled, void* linear, int nplanes, size_t elem, int w, int h, hipStream_t s);
// (vct_variant_takes_row_subsets, which variants take strided or packed tile rows: vct_trace_forms.h, with the launch plan)
// sets p.ntiles on its own copy; march_form: the division form dispatched (vct_trace.hip)
// marks (optional, half-rate passes only): three events recorded between the pass's four launches
hipError_t vct_launch_trace(const VctTraceParams& p, int variant, hipStream_t s, int* march_form = nullptr,
                            const hipEvent_t* marks = nullptr);
hipError_t vct_launch_divide_selftest(float d, unsigned long long* mismatches, hipStream_t s);
// typed-buffer texel loads (RGBA8 UNORM -> four floats in the texture path) against the exact decode, n texels
// buf: [lead][n][n] texels, out: 4 words (vct_trace.hip k_texel_buffer_selftest)
hipError_t vct_launch_texel_buffer_selftest(const uint32_t* buf, uint32_t lead, uint32_t n, unsigned long long* out, hipStream_t s);
hipError_t vct_launch_area_divide_selftest(uint64_t seed, uint64_t count, unsigned long long* out, hipStream_t s);
hipError_t vct_launch_linear_to_morton(const uint32_t* lin, uint32_t* mor, int N, hipStream_t s);
hipError_t vct_launch_morton_to_linear(const uint32_t* mor, uint32_t* lin, int N, hipStream_t s);
// bricks_now / bricks_seen (optional): per-8^3-brick occupancy flags of level 0 for the sparse form
hipError_t vct_launch_build_mips(uint32_t* chain, int V, const uint32_t* bricks_now, uint32_t* bricks_seen,
                                 hipStream_t s);
hipError_t vct_launch_build_mips_aniso(const uint32_t* level0, uint32_t* aniso, int V, hipStream_t s);
hipError_t vct_launch_build_cells(const uint32_t* chain, uint4* cells, int V, hipStream_t s);
// fragment list of the conservative voxelizer, built at upload: small triangles (+ the list of the big ones), big
// triangles, then the counting sort by brick slot
hipError_t vct_launch_vox_plan(const VctVoxParams& p, uint32_t* plan, uint2* frags,
                               int32_t* big_list, bool write, hipStream_t s);
hipError_t vct_launch_vox_plan_big(const VctVoxParams& p, const int32_t* big_list, int n_big, uint32_t* plan, uint2* frags,
                                   bool write, hipStream_t s);
hipError_t vct_launch_frag_mark(const uint2* frags, uint32_t n, uint32_t* mark, hipStream_t s);
hipError_t vct_launch_frag_count(const uint2* frags, uint32_t n, const uint32_t* brick_slot, uint32_t* count, hipStream_t s);
hipError_t vct_launch_frag_scatter(const uint2* frags, uint32_t n, const uint32_t* brick_slot, const uint32_t* first,
                                   uint32_t* cursor, uint32_t* sorted, uint32_t* slot_brick, hipStream_t s);
hipError_t vct_launch_voxelize(const VctVoxParams& p, hipStream_t s);
hipError_t vct_launch_frag_geom(const VctVoxParams& p, float2* bary, float* frag_alb, hipStream_t s);
hipError_t vct_launch_tri_nrm(const VctVoxParams& p, uint32_t* tri_nrm, hipStream_t s);
hipError_t vct_launch_resolve(const VctResolveArgs& a, int V, bool dense, hipStream_t s);
// mark[b] != 0 -> slot[b] = next free slot (order irrelevant), else VCT_NO_SLOT; *count = slots handed out
hipError_t vct_launch_assign_slots(const uint32_t* mark, uint32_t* slot, uint32_t* count, uint32_t nbricks, hipStream_t s);
hipError_t vct_launch_slot_bricks(const uint32_t* slot, uint32_t nbricks, uint32_t* slot_brick, hipStream_t s);
// pooled per-voxel attribute -> dense Morton volume (downloads)
hipError_t vct_launch_unpool(const uint32_t* pooled, const uint32_t* brick_slot, uint32_t* dense, uint32_t nbricks, hipStream_t s);
hipError_t vct_launch_voxelize_reference(const VctVoxParams& p, int32_t* big_list, int32_t* big_count,
                                         hipStream_t s);
// `dyn` not null: the bounce over a chain the dynamic layer was merged into (include/vct.h "dynamic mesh", the second
// bounce) -- k_bounce_dyn_map writes brick_res (all VCT_NO_SLOT on entry) from the resolved list, then the DYN
// instantiations of the three bounce kernels run with these pointers behind VctTraceParams
struct VctBounceDynArgs {
    const uint32_t* res_brick;   // [max_bricks] slot -> brick of the last resolved pass
    const uint32_t* used;        // the statistics word of that pass: slots in use
    const uint32_t* pool_rad;    // [max_bricks][512] the layer's pools
    const uint32_t* pool_alb;
    const uint32_t* pool_nrm;
    uint32_t* brick_res;         // [nbricks] brick -> resolved slot
    uint32_t max_bricks;
    uint32_t list_slots;         // static slots + max_bricks (vct_dynamic_check.h): what the list kernel's grid is sized for
};
hipError_t vct_launch_bounce(const VctTraceParams& p, hipStream_t s, const VctBounceDynArgs* dyn = nullptr);

// ---- the dynamic mesh (include/vct.h "dynamic mesh"; k_dyn_* in vct_voxelize.hip) ----
// Voxelized by itself every pass, with no plan: bricks are claimed in a [V^3/512] table (VCT_NO_SLOT -> VCT_DYN_CLAIMED ->
// slot number), fragments meet in HBM accumulators [slot][512] laid out like acc2 / acc2_attr, and the merge behind the
// static resolve turns them into texels.  Device words of the layer (VctDynArgs::words):
#define VCT_DYN_CLAIMED 0xfffffffeu     // a brick whose winner has not stored its slot yet, or got none (capacity)
#define VCT_DYN_W_NEED 0                // bricks the pending pass claimed = slot numbers drawn
#define VCT_DYN_W_FRAGS 1               // its conservative fragments
#define VCT_DYN_W_SKIPPED 2             // its triangles outside the vertex contract
#define VCT_DYN_W_NBIG 3                // triangles in big_list
#define VCT_DYN_W_STATS 8               // two sets of 8 words, written in turn by the merges: need, used, fragments, skipped, left out
#define VCT_DYN_WORDS 32
struct VctDynArgs {
    uint32_t* words;                    // [VCT_DYN_WORDS]
    uint32_t* brick_slot;               // [V^3 / 512]; all VCT_NO_SLOT between passes
    uint32_t* slot_brick;               // [max_bricks] slot -> brick of the pending pass
    int32_t* big_list;                  // [ntri] triangles whose box exceeds VCT_VOX_BIG voxels
    uint32_t max_bricks;
    float vertex_limit;                 // VCT_VERTEX_LIMIT_GRIDS * grid_world_size
    unsigned long long* acc;            // [max_bricks][512][2] sumR | sumG << 32, sumB | count << 32
    unsigned long long* acc_attr;       // [max_bricks][512][3] or null (config.voxel_attributes)
};
// slots (claim) then fragments, small triangles by a thread each, big ones by a workgroup each; p: mesh, grid, shadow map
// `emis` not null (vct_set_dynamic_emission): the EMIS instantiations of the fragment kernels, which also add every
// fragment's unorm8(emission[material]) to the emission sums
struct VctDynEmisArgs {
    const float* emission;              // [nmat][4] (rgb, 0) of the dynamic mesh
    unsigned long long* acc_emis;       // [max_bricks][512][2]: r | g << 32, b; all zero between passes
};
hipError_t vct_launch_dynamic_voxelize(const VctVoxParams& p, const VctDynArgs& d, bool slots_only, hipStream_t s,
                                       const VctDynEmisArgs* emis = nullptr);
struct VctDynMergeArgs {
    VctDynArgs d;
    uint32_t nbricks;
    int32_t set;                        // the statistics set this merge writes (the other holds the last resolved pass)
    int32_t discard;                    // 1: only re-zero the accumulators and the table (a pass that was never resolved)
    uint32_t* res_brick;                // [max_bricks] slot -> brick of the last resolved pass; 0 for a slot without one
    uint32_t* pool_rad;                 // [max_bricks][512] the layer's texels, attributes (null without) of the last resolved pass
    uint32_t* pool_alb;
    uint32_t* pool_nrm;
    uint32_t* level0;                   // [V^3] Morton
    uint32_t* brick_prev;               // [V^3 / 512]
};
// acc_emis not null: the pass was voxelized with the emission table -- the EMIS instantiation resolves and re-zeroes the sums
hipError_t vct_launch_dynamic_merge(const VctDynMergeArgs& a, hipStream_t s, unsigned long long* acc_emis = nullptr);
// pooled [slot][512] of the resolved pass of statistics set `set` -> dense Morton volume (zero elsewhere)
hipError_t vct_launch_dynamic_unpool(const uint32_t* pool, const uint32_t* res_brick, const uint32_t* words, int set,
                                     uint32_t max_bricks, uint32_t nbricks, uint32_t* dense, hipStream_t s);

// the voxel view (include/vct.h "voxel view", vct_voxview.hip)
struct VctVoxViewParams {
    const uint32_t* texels;            // the viewed level (Morton), or the pooled attribute [slot][512] when brick_slot is set
    const uint32_t* brick_slot;        // [V^3 / 512] brick -> slot of a pooled attribute; null: `texels` is a level of a chain
    unsigned long long* occ;           // occupancy words, [occ_dim^3]: one bit per 8^3 block, one word per 32^3 region
    int32_t N;                         // cells per side of the viewed level, V >> level
    int32_t occ_dim;                   // max(1, N / 32)
    float G, max_alpha;
    float m[16];                       // column-major inverse view-projection
    int32_t width, height, tiles_x, tiles_y;
    uint16_t* out;                     // RGBA16F [h][w][4]
};
hipError_t vct_launch_voxview_occupancy(const VctVoxViewParams& p, hipStream_t s);
// skip = false: the instantiation without the occupancy look-ups (every block is fetched): the A/B arm of the measurements
hipError_t vct_launch_voxview(const VctVoxViewParams& p, bool skip, hipStream_t s);

// the G-buffer import (include/vct.h "G-buffer import", k_gbuffer_import in vct_raster.hip)
struct vct_gbuffer_import;
struct VctImportArgs {
    const vct_gbuffer_import* desc;    // a checked descriptor (vct_import_check.h) whose pointers are device pointers
    int32_t W, H, row0, row1;          // the frame; tile rows [row0, row1) are written
    const uint32_t* shadow;            // the context's shadow-map words or null, as vct_launch_gbuffer_shade takes them
    uint32_t shadow_ebase;
    int32_t shadow_size;
    const uint2* shadow_tiles;
    const float* light_vp;             // [16]
    float* tiled;                      // [tile][23][64]
    const float* emission;             // [nmat][4] with emis_tiled [tile][3][64], or both null: the planes are not written
    float* emis_tiled;
    const uint8_t* mat_gloss;          // [nmat] with gloss_tiled [tile][64], or both null
    uint8_t* gloss_tiled;
    int32_t nmat;
};
hipError_t vct_launch_gbuffer_import(const VctImportArgs& a, hipStream_t s);

// local lights (include/vct.h "local lights", vct_lights.hip): the folded table (vct_lights_check.h VctLightDev, 64 B per
// light) is read at wave-uniform indices by both kernels
struct VctLightDev;
struct VctLightVoxArgs {
    const VctLightDev* lights;         // [nlights]
    int32_t nlights;                   // 1 .. VCT_LIGHTS_MAX
    int32_t V;
    float G;
    uint32_t* level0;                  // [V^3] Morton; bricks the last resolve wrote (brick_prev) are updated in place
    const uint32_t* attr_albedo;       // [nslots][512] the pooled voxel attributes of that resolve
    const uint32_t* attr_normal;
    const uint32_t* slot_brick;        // [nslots]
    const uint32_t* brick_prev;        // [V^3 / 512]
    uint32_t nslots;
};
struct VctLightPixArgs {
    const VctLightDev* lights;
    int32_t nlights;
    int32_t width, height, tiles_x;
    int32_t row0, row1;                // tile rows filled
    float cam[3];
    float shininess;                   // config.shininess; with a gloss plane, class_shininess[class of the pixel]
    uint32_t show;                     // VCT_SHOW_* mask of the launch that follows
    const float* gbuf;                 // tiled [tile][23][64]
    const float* emis;                 // tiled [tile][3][64] pixel-emission planes or null
    const uint8_t* pix_gloss;          // tiled [tile][64] or null
    int32_t nclasses;
    float class_shininess[8];
    float* lit;                        // tiled [tile][3][64]
};
hipError_t vct_launch_light_voxels(const VctLightVoxArgs& a, hipStream_t s);
hipError_t vct_launch_light_pixels(const VctLightPixArgs& a, hipStream_t s);

#endif
