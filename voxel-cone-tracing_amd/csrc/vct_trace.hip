// vct_trace.hip -- per-pixel cone trace (6 diffuse + 1 specular) through the Morton brick chain.
//
// Replaces the fragment stage of the reference's main draw: S/VoxelConeTracing.fs:59-66
// (SampleVoxels), :82-107 (Voxel_Cone_Tracing), :165-228 (gather + composite), with the driver's
// textureLod (trilinear x 2 levels, GL_REPEAT, texel centres -- OpenGL 4.3 core)
// written out by hand because there is no texture unit behind a HIP pointer.
//
// Arithmetic contract: the march is operation-for-operation the scalar oracle's (fp32, explicit
// fmaf only where the oracle has one or where the fused form is provably the same bits), so
// per-cone step counts and the raw cone vec4s are bit-identical; compile with -ffp-contract=off.
//
// Kernels in this file: k_trace_tile_split (default: an 8x8 screen tile = 3 waves -- cones 0-2, cones
// 3-5, specular -- with an LDS hand-off and a last-arriver composite; its GLOSS forms march the specular cone once per
// gloss class present in the tile), k_trace_tile (one wave per
// tile; A/B variants), k_bounce_list/_march/_bricks (second bounce, same march), k_point_march + k_diffuse_resolve (half-rate
// diffuse gather, same march), k_query_march + k_query_keys (point queries, same march), k_divide_selftest.
//
// Mapping: lane = pixel of the tile, a wave marches its cones one after the other.  The kernel
// was VALU-issue bound from round 1 (profiles/r01a: 995 M VALU wave-instructions per 1080p frame, half of the
// wave cycles spent waiting to issue, 12 % waiting on memory) to round 5 (543 M), and on gfx950 only fp32
// fma/mul/add and plain logic ops issue in 2 cycles per wave -- conversions, floor, bit-field,
// 3-operand integer ops take 4 (tools/valu_bench.hip).  The dominant cost per march step was
// turning 2 x 8 RGBA8 texels into 64 floats (cvt + exact /255) and the Morton address of each, so
// the sampler is organised to do that work once per wave instead of once per lane -- and since round 6 the
// conversion itself is left to the texture path: a level is read as an RGBA8 UNORM TEXEL BUFFER (typed-buffer
// loads, level_texel_buffer / texel_f32 below), whose UNORM8 -> fp32 conversion is bit for bit (float)c / 255.0f
// on this GPU (tools/unorm_probe.hip, vct_selftest_texel_buffer).  447 M VALU wave-instructions per frame now,
// vector pipes 83 % busy, 38 % of the wave-cycles waiting on memory (profiles/r06f_final.txt).
//
//   cooperative sample (the common case): the 64 trilinear footprints of a tile at one march
//   step almost always fall inside one 4x4x4 texel block of the level (neighbouring pixels trace
//   near-parallel cones; ~85 % of wave-level samples of the 1080p bench frame).  The block is
//   anchored at the centre pixel's footprint; lane l fetches block texel (l&3, (l>>2)&3, l>>4)
//   with ONE load (Morton index = scalar-unit spread of the anchor + a per-lane dilated-integer
//   add; the four channels arrive as floats), parks the float4 in a wave-private 1 KiB LDS slab, and
//   every lane gathers its own 8 texels with ds_read_b128 at constant offsets {0,1,4,5,16,..}.
//   If the whole block is zero (ballot) the sample is exactly 0 and everything else is skipped.
//
//   per-lane sample (incoherent waves: silhouettes, random G-buffers): 8 texel loads per lane as in a
//   plain gather (phases of 2 + 2 + 4), the dilated coordinates from the anchor path's table, the +1
//   neighbours derived by dilated increments.
//
// Both produce the same bits.  Divisions by wave-uniform constants use a two-term reciprocal product
// instead of the 10-instruction IEEE sequence, for divisors the device has verified exhaustively
// (vct_capi.hip: divisor_verified).
#include <hip/hip_fp16.h>

#include <type_traits>
#include <utility>

#include "../../include/vct.h"
#include "vct_internal.h"
#include "vct_texel.h"
#include "vct_tilediv.h"
#include "vct_trace_forms.h"


namespace {

struct F3 { float x, y, z; };
struct F4 { float x, y, z, w; };

__device__ __forceinline__ F3 f3(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ float dot3(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ F3 cross3(F3 a, F3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// IEEE-correct fp32 divide / sqrt (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; the
// __fsqrt_rn intrinsic maps to the 1-ulp native sqrt and must not be used here).
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }
__device__ __forceinline__ float sqrt_rn(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ F3 normalize3(F3 a) {
    const float l = sqrt_rn(dot3(a, a));
    return {div_rn(a.x, l), div_rn(a.y, l), div_rn(a.z, l)};
}
__device__ __forceinline__ F3 reflect3(F3 I, F3 N) {
    const float d = 2.0f * dot3(N, I);
    return {I.x - d * N.x, I.y - d * N.y, I.z - d * N.z};
}

// x / d for a wave-uniform divisor d: the IEEE division costs v_div_scale x2, v_rcp, 4 fma, v_div_fmas, v_div_fixup.
// Rounds 1-3: q = x*r; e = fma(-d, q, x); q = fma(e, r, q) with r = RN(1/d) -- three instructions, one correction
// round.  Since round 4: t = x * r_lo; q = fma(x, r_hi, t) with r_hi = RN(1/d), r_lo = RN(1/d - r_hi) -- TWO
// instructions: r_hi + r_lo is 1/d to ~48 bits, the fma adds the two products exactly and rounds once, so q is the
// correctly rounded quotient unless x/d lies within ~2^-47 of a rounding boundary.  Neither form is correctly rounded
// for every divisor, so both are used only for divisors the DEVICE has verified: before a step table is used,
// vct_capi.hip runs k_divide_selftest for each of its divisors (half_G and the per-step occlusion denominators) over
// EVERY fp32 x of the domain below and requires the IEEE quotient bit for bit (results cached per divisor; all 334
// divisors of the BASELINE grids and apertures pass, in either form: csrc/vct_divisors.h); a table with a divisor that
// fails runs the IEEE-divide instantiation.  Atrium 0.6177 -> 0.6107 ms, street at 1024^3 / 4K 2.727 -> 2.711 ms.
// Domain: x == +0 and every finite |x| >= 2^-100 whose quotient is a normal number (host-side precondition on
// d: vct_capi.hip divisor_ok; below that the low product x * r_lo -- or the remainder e of the older form -- loses
// bits to underflow; the sign of a zero quotient is not preserved).
// The march stays inside the domain by construction:
//   * coordinates: |x| < 2^-100 or x == -0 gives |q| < 2^-26, and u = fma(q, .5, .5) = 0.5 for any
//     such q, exactly as with the IEEE quotient;
//   * occlusion numerator oma * vc.w: never -0, and either +0 or >= 2^-98 -- a non-zero filter
//     fraction is >= 2^-25 (u = fma(ux, N, -0.5) is exact and a multiple of 2^-25 near 0), so a
//     non-zero trilinear weight is >= 2^-75, a non-zero texel >= 1/255, the level blend factors are
//     0 or >= 2^-10 and oma >= 2^-5 (both checked on the host: vct_capi.hip refresh_steps).
#define VCT_DIV_TINY 0x1p-100f
// MODE 0: the IEEE division, 1: the verified form (two-term product), 2: x * r alone -- NOT exact: only the opt-in "loose" trace
// variant that prices the exactness (config.trace_variant = 3, k_trace_tile_split<.., 2, ..>) uses it
// `d`: the divisor -- or, for MODE 1, the low word r_lo of its reciprocal (the host puts it where the
// divisor used to be: VctStep::occ_den, VctTraceParams::half_G_aux)
template <int MODE>
__device__ __forceinline__ float div_const(float x, float d, float r) {
    if (MODE == 0) return x / d;
    if (MODE == 2) return x * r;
    // x / d = x * (r_hi + r_lo) (1 + e), |e| < 2^-47: the one rounding of the fma is the rounding of the quotient unless
    // x / d lies within 2^-47 of a rounding boundary -- which the device rules out per divisor, over every fp32 x
    return fmaf(x, r, x * d);
}

// unorm8 -> float, bit-identical to (float)c / 255.0f for every c in [0,255]:
// c * RN(1/255) misses for 126 of the 256 bytes; the two-term product below never does
// (checked exhaustively in tests/test_abi.py::test_unorm8_decode_exact).
__device__ __forceinline__ float unorm8(uint32_t c) { return vct_unorm8_to_float(c); }

// level_texel_buffer / texel_f32 (a level of the chain as an RGBA8 UNORM texel buffer) and pack_half2: vct_texel.h

// LDS operations of one wave execute in order, so a slab written and then read by the lanes of
// the same wave needs no s_barrier -- only the compiler must not reorder across this point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// HIP's __ballot()/__any() lower to v_cndmask + v_cmp_ne; the builtin is the compare mask itself.
__device__ __forceinline__ unsigned long long ballot64(bool pred) {
    return __builtin_amdgcn_ballot_w64(pred);
}
// the sum of v over the 64 lanes, in every lane (the waves' executed-step counts; the self-test's mismatch count)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Dilated anchor coordinates come from a table: computing spread3() of three scalars took 41 scalar-unit instructions
// per level sample, and the scalar pipe issues one instruction per 4 cycles per SIMD (tools/valu_bench.hip: s_add /
// s_and / s_mul 4.17 cycles at any occupancy) -- with half as many SALU as VALU instructions it was 68 % busy, and a
// padding experiment showed the march paying 2.1 us per scalar instruction added to a step against 1.4 us per vector
// one.  (Re-measured on the kernel of 8 waves per SIMD and 0.515 ms: 0.93 us per scalar instruction added to every step,
// 1.22 us per vector one -- profiles/experiments/README.md, round 17: the price list of the scalar-side changes since.)
// One s_load_dword per axis replaces 13 instructions.  Entry i = spread3(i) << 2 (byte offset of the x axis).
// (Round 17: a table per axis with the entries in place and the other bits set takes the two shifts and the three ORs
// with the masks' complements out of a fetch -- and the allocation that came with it ten more scalars through the spill
// lanes: 5 us slower than without.  profiles/experiments/README.md.)
typedef const __attribute__((address_space(4))) uint32_t* SpreadLut;
// byte offset of x coordinate (a & m) in dilated form; m4 = m << 2.  All 32-bit, so the table entry is one
// s_load_dword with an SGPR offset.
__device__ __forceinline__ uint32_t spread_byte(SpreadLut lut, int a, uint32_t m4) {
    const uint32_t off = ((uint32_t)a << 2) & m4;
    return *(SpreadLut)((const __attribute__((address_space(4))) char*)lut + off);
}

// A chain as the samplers read it (wave-uniform): its first texel and the texel buffer over it, formed once per wave.
// The samplers' loads take a level's texels in one of two forms (LevelBuf):
//   CHAIN      the chain's resource and the level's BYTE offset in the load's scalar offset operand: one shift per fetch
//   otherwise  a resource over the level itself and 0: a shift, a 64-bit add, a mask and the stride word -- six scalar
//              instructions in front of every fetch, cooperative or per lane
// Same address, same conversion (k_texel_buffer_selftest), same bits.  A byte offset has 32 bits, so CHAIN serves chains
// whose levels all start below 4 GiB (vct_internal.h vct_chain_form_fits; the host chooses per context: vct_ctx
// chain_form, VCT_LEVEL_DESCRIPTORS).  It is a template flag of the default kernel's GL_REPEAT forms (k_trace_tile_split)
// and nothing else: there the march's scalar stream is what a fetch waits behind, and a flag tested per fetch costs
// what the flag saves.  Whichever member a form does not read is never formed.
struct ChainRef { const uint32_t* base; vct_v4i32 tb; };
__device__ __forceinline__ ChainRef chain_ref(const uint32_t* chain) { return {chain, level_texel_buffer(chain)}; }
struct LevelBuf { vct_v4i32 tb; uint32_t soffset; };
template <bool CHAIN>
__device__ __forceinline__ LevelBuf level_buf(const ChainRef& ch, const VctLevelRef lv) {
    if constexpr (CHAIN) return {ch.tb, lv.off << 2};
    else return {level_texel_buffer(ch.base + lv.off), 0u};
}

struct LaneBlock {      // this lane's texel inside the cooperative 4x4x4 block
    ChainRef chain;             // (wave-uniform) the launch's chain, p.chain
    SpreadLut lut;              // (wave-uniform) the dilated-coordinate table
    const uint32_t* lut_vec;    // the same table through a plain global pointer (per-lane gather)
    int lane;
    uint32_t sbx, sby, sbz;     // texel-INDEX offsets: dilated (l&3), ((l>>2)&3)<<1, (l>>4)<<2
};
// the exact unorm8 -> float decode of one channel of a packed texel, where a texel is not read through the texture path
template <int SHIFT, bool LOOSE = false>
__device__ __forceinline__ float unorm8_of(uint32_t t) {
    if (LOOSE) return (float)((t >> SHIFT) & 0xffu) * 0x1.010102p-8f;     // one multiply: wrong in the last bit for 126 of the 256 bytes
    return vct_unorm8_to_float((t >> SHIFT) & 0xffu);
}

// Instrumented build (-DVCT_STATS=1, tools/trace_stats.py): wave-level counters of the march, kept in
// SGPRs and flushed once per wave.  The production build compiles all of it away.
#ifndef VCT_STATS
#define VCT_STATS 0
#endif
struct MarchStats {
    uint32_t wave_steps;       // march-loop iterations executed by the wave
    uint32_t lane_steps;       // sum over those iterations of the live lanes (== executed cone steps)
    uint32_t coop_zero;        // level samples served by the cooperative block, block all zero (skipped)
    uint32_t coop_hit;         // level samples served by the cooperative block, gathered through LDS
    uint32_t fallback;         // level samples that took the per-lane gather
    uint32_t fallback_lanes;   // live lanes in those
    uint32_t fallback_fits;    // per-lane samples whose live footprints WOULD fit one 4x4x4 block (anchored at their minimum)
    uint32_t greedy_blocks, greedy_le2, greedy_le3, greedy_le4;   // blocks a greedy multi-anchor cover of them would need
    uint32_t two_blocks;       // (unused: the two-block experiment's counter, kept so that the layout stays)
    // round 5 (review item 3): would sharing inside smaller lane groups serve the per-lane samples?  Per per-lane sample:
    uint32_t quads_live;       // 2x2-pixel quads with a live lane
    uint32_t quads_fit333;     // ... whose live footprints span <= 1 texel per axis (their union fits a 3x3x3 block)
    uint32_t quads_same;       // ... whose live footprints are one and the same 2x2x2 cell
    uint32_t quadrants_live;   // 4x4-pixel quadrants with a live lane
    uint32_t quadrants_fit444; // ... whose live footprints fit a 4x4x4 block of their own
    // round 7: block reuse (BlockDesc below), per cooperative sample, [first / second level of the step]:
    //   0 candidates: the second slab holds a block of this level          1 hits: every live footprint lies inside it
    //   2 hits whose block was all zero      3 candidates whose anchor equals the one a fresh block would take
    uint32_t reuse[2][4];
};

// ---- the pieces the three samplers below share: written once, the oracle's operations in the oracle's order ---------
// A lane's trilinear footprint in a level: lower corner (unreduced integer coordinates) and filter fractions.
struct Footprint { int i0, j0, k0; float a, b, c; };
__device__ __forceinline__ Footprint footprint_of(const VctLevelRef lv, float ux, float uy, float uz) {
    const float fN = lv.fN;
    // ux * fN is exact (power of two), so the fused form is the oracle's (ux*fN) - 0.5f bit for bit
    const float u = fmaf(ux, fN, -0.5f), v = fmaf(uy, fN, -0.5f), w = fmaf(uz, fN, -0.5f);
    const float fu = floorf(u), fv = floorf(v), fw = floorf(w);
    const float a = u - fu, b = v - fv, c = w - fw;
    return {(int)fu, (int)fv, (int)fw, a, b, c};
}
// The cooperative 4x4x4 block is anchored one texel below the footprint of the tile's centre pixel (lane 27) if that
// lane is live, else of the first live lane.  `am` = ballot of the live lanes, not empty.
struct Anchor { int x, y, z; };
__device__ __forceinline__ int anchor_lane(unsigned long long am) {
    return ((am >> 27) & 1ull) ? 27 : (int)__ffsll((long long)am) - 1;
}
__device__ __forceinline__ Anchor anchor_of(const Footprint& f, int src) {
    return {__builtin_amdgcn_readlane(f.i0, src) - 1, __builtin_amdgcn_readlane(f.j0, src) - 1,
            __builtin_amdgcn_readlane(f.k0, src) - 1};
}
// Where this lane's footprint starts inside the block at `an`, and the live lanes whose footprint does not lie inside
// it (an offset outside 0..2, negative ones included: the compare is unsigned).  `out` == 0: the block serves the wave.
struct BlockFit { int dx, dy, dz; unsigned long long out; };
__device__ __forceinline__ BlockFit block_fit(const Footprint& f, const Anchor an, unsigned long long am) {
    const int dx = f.i0 - an.x, dy = f.j0 - an.y, dz = f.k0 - an.z;
    const uint32_t far = max(max((uint32_t)dx, (uint32_t)dy), (uint32_t)dz);
    return {dx, dy, dz, ballot64(far > 2u) & am};
}
// Index inside the level of the block texel this lane fetches: texel (l&3, (l>>2)&3, l>>4) of the block at `an`.
// Texels are addressed by their Morton INDEX inside the level (< 2^30): the dilated-integer arithmetic yields it
// directly, and the level is a texel buffer whose structured load takes the index (no shift, no 64-bit address add).
template <bool WRAP>
__device__ __forceinline__ uint32_t block_texel_index(const VctLevelRef lv, const Anchor an, const LaneBlock& lb) {
    if (WRAP) {
        // scalar unit: dilate the anchor; vector unit: one dilated add per axis
        const uint32_t MX = lv.mask_x, MY = MX << 1, MZ = MX << 2;
        const uint32_t m4 = (uint32_t)lv.m << 2;
        // (the table holds spread3(i) << 2: the scalar unit shifts it into place -- one shift for two of the axes, as before)
        const uint32_t sax = spread_byte(lb.lut, an.x, m4) >> 2;
        const uint32_t say = spread_byte(lb.lut, an.y, m4) >> 1;
        const uint32_t saz = spread_byte(lb.lut, an.z, m4);
        return (((sax | ~MX) + lb.sbx) & MX) | (((say | ~MY) + lb.sby) & MY) | (((saz | ~MZ) + lb.sbz) & MZ);
    } else {
        const int x = min(max(an.x + (lb.lane & 3), 0), lv.m);
        const int y = min(max(an.y + ((lb.lane >> 2) & 3), 0), lv.m);
        const int z = min(max(an.z + (lb.lane >> 4), 0), lv.m);
        return vct_morton3((uint32_t)x, (uint32_t)y, (uint32_t)z);
    }
}
// float4 of a slab at which a lane's footprint starts (gather_block's q); a lane that is not live reads the block's first
__device__ __forceinline__ int block_slot(bool act, int dx, int dy, int dz) { return act ? (dz * 4 + dy) * 4 + dx : 0; }
// (channels are >= +0: the block is empty iff no channel of any lane's texel has a bit set)
__device__ __forceinline__ unsigned long long block_texel_mask(const float4 d) {
    return ballot64((__float_as_uint(d.x) | __float_as_uint(d.y) | __float_as_uint(d.z) | __float_as_uint(d.w)) != 0u);
}

// Block reuse (round 7).  A march step usually samples a level the wave sampled one step earlier, at most a texel or two
// further on: a diffuse cone's LOD grows 1.1 per step, so the lower level of a step is the upper level of the step before;
// a specular cone stays on one pair of levels for several steps.  A 4x4x4 block covers three footprint origins per axis
// and a coherent tile's 64 footprints span one or two, so the block fetched then usually still holds every texel the
// new sample reads.  The wave therefore keeps a descriptor -- wave-uniform, four SGPRs -- of the block in its SECOND
// slab (blk + 64, the one the upper level of a step fills); a cooperative sample of either level whose live footprints
// all lie inside that block gathers from it and skips the table loads, the index arithmetic, the load, the zero ballot
// and the LDS write.  A block's texels are a function of (level, anchor + s mod N) alone, so a lane whose offsets
// against ANY anchor lie in 0..2 reads the eight texel values it reads from a block anchored at the centre lane's
// footprint (sample_level's rule): same bits.
// The chain does not change during a launch, so the descriptor lives across the cones of a wave; it starts invalid.
// (A descriptor for each slab would also serve the lower level of a specular step, but its four SGPRs more put the
// default kernel into scratch and made it slower than without reuse: profiles/experiments/README.md, round 7.)
// -DVCT_REUSE=0 builds the kernels without the path (vct_trace_forms.h, with the rule which forms take it: split_reuse).
#define VCT_NO_BLOCK 0xfffffff0u     // BlockDesc::id of a slab that holds nothing (no level starts there)
struct BlockDesc {
    // the level (VctLevelRef::off: a multiple of 8, every level in front of it holds a power of 8 texels >= 8) | 1 when
    // the block is in the slab; without the bit the block is all zero and the slab holds nothing.  Or VCT_NO_BLOCK.
    uint32_t id;
    Anchor an;          // in the sampler's unreduced integer coordinates
};
__device__ __forceinline__ BlockDesc no_block() { return {VCT_NO_BLOCK, {0, 0, 0}}; }

// the trilinear fold of a lane's 8 texels out of a block in LDS; q = the lane's lower corner in the slab
// NARROW: two texels in flight where there are four -- the same fold in the same order, eight registers fewer at the
// kernel's widest point (the whole-frame march under the 64-register bound: k_trace_tile_split's MINW)
template <bool NARROW = false>
__device__ __forceinline__ F4 gather_block(const float4* q, float a, float b, float c) {
    F4 r;
    const float a0 = 1.0f - a, b0 = 1.0f - b, c0 = 1.0f - c;
    const float ab00 = a0 * b0, ab10 = a * b0, ab01 = a0 * b, ab11 = a * b;
    if constexpr (NARROW) {
        {
            const float4 t0 = q[0], t1 = q[1];
            const float w0 = ab00 * c0, w1 = ab10 * c0;
#define VCT_ACC(ch) r.ch = w0 * t0.ch; r.ch = fmaf(w1, t1.ch, r.ch);
            VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            const float4 t2 = q[4], t3 = q[5];
            const float w2 = ab01 * c0, w3 = ab11 * c0;
#define VCT_ACC(ch) r.ch = fmaf(w2, t2.ch, r.ch); r.ch = fmaf(w3, t3.ch, r.ch);
            VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            const float4 t4 = q[16], t5 = q[17];
            const float w4 = ab00 * c, w5 = ab10 * c;
#define VCT_ACC(ch) r.ch = fmaf(w4, t4.ch, r.ch); r.ch = fmaf(w5, t5.ch, r.ch);
            VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            const float4 t6 = q[20], t7 = q[21];
            wave_sync();
            const float w6 = ab01 * c, w7 = ab11 * c;
#define VCT_ACC(ch) r.ch = fmaf(w6, t6.ch, r.ch); r.ch = fmaf(w7, t7.ch, r.ch);
            VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
        }
        return r;
    }
    {   // lower z plane first, then the upper one: half the texel registers live at a time
        const float4 t0 = q[0], t1 = q[1], t2 = q[4], t3 = q[5];
        const float w0 = ab00 * c0, w1 = ab10 * c0, w2 = ab01 * c0, w3 = ab11 * c0;
#define VCT_ACC(ch) r.ch = w0 * t0.ch; r.ch = fmaf(w1, t1.ch, r.ch); r.ch = fmaf(w2, t2.ch, r.ch); r.ch = fmaf(w3, t3.ch, r.ch);
        VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
    }
    __builtin_amdgcn_sched_barrier(0);
    {
        const float4 t4 = q[16], t5 = q[17], t6 = q[20], t7 = q[21];
        wave_sync();
        const float w4 = ab00 * c, w5 = ab10 * c, w6 = ab01 * c, w7 = ab11 * c;
#define VCT_ACC(ch) r.ch = fmaf(w4, t4.ch, r.ch); r.ch = fmaf(w5, t5.ch, r.ch); r.ch = fmaf(w6, t6.ch, r.ch); r.ch = fmaf(w7, t7.ch, r.ch);
        VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
    }
    return r;
}

// VCT_STATS only: the census of a per-lane sample -- would one block anchored at the live footprints' minimum serve it,
// how many blocks a greedy multi-anchor cover needs, and whether sharing inside 2x2-pixel quads or 4x4-pixel quadrants
// would (MarchStats: fallback*, greedy*, quads*, quadrants*).
__device__ __forceinline__ void per_lane_census(MarchStats& ms, const Footprint& f, bool act, unsigned long long am, int lane) {
    const int i0 = f.i0, j0 = f.j0, k0 = f.k0;
    ++ms.fallback; ms.fallback_lanes += (uint32_t)__popcll(am);
    int lo[3] = {act ? i0 : 0x7fffffff, act ? j0 : 0x7fffffff, act ? k0 : 0x7fffffff};
    int hi[3] = {act ? i0 : -0x7fffffff, act ? j0 : -0x7fffffff, act ? k0 : -0x7fffffff};
    for (int off = 32; off > 0; off >>= 1)
        for (int q = 0; q < 3; ++q) { lo[q] = min(lo[q], __shfl_xor(lo[q], off)); hi[q] = max(hi[q], __shfl_xor(hi[q], off)); }
    if (hi[0] - lo[0] <= 2 && hi[1] - lo[1] <= 2 && hi[2] - lo[2] <= 2) ++ms.fallback_fits;
    // greedy cover: blocks anchored at the first lane not yet covered
    unsigned long long pending = am;
    int nb = 0;
    while (pending != 0ull && nb < 16) {
        const BlockFit fit = block_fit(f, anchor_of(f, (int)__ffsll((long long)pending) - 1), ~0ull);
        pending &= fit.out;
        ++nb;
    }
    // the same range test inside 2x2-pixel quads (lanes l, l^1, l^8, l^9) and 4x4-pixel quadrants (+ l^2, l^16, ...)
    int qlo[3] = {act ? i0 : 0x7fffffff, act ? j0 : 0x7fffffff, act ? k0 : 0x7fffffff};
    int qhi[3] = {act ? i0 : -0x7fffffff, act ? j0 : -0x7fffffff, act ? k0 : -0x7fffffff};
    bool qany = act;
    auto widen = [&](int off) {
        for (int q = 0; q < 3; ++q) { qlo[q] = min(qlo[q], __shfl_xor(qlo[q], off)); qhi[q] = max(qhi[q], __shfl_xor(qhi[q], off)); }
        qany = qany || (__shfl_xor((int)qany, off) != 0);
    };
    widen(1); widen(8);
    const int span2 = max(max(qhi[0] - qlo[0], qhi[1] - qlo[1]), qhi[2] - qlo[2]);
    const bool lead2 = (lane & 9) == 0;                      // one lane per quad
    ms.quads_live += (uint32_t)__popcll(ballot64(lead2 && qany));
    ms.quads_fit333 += (uint32_t)__popcll(ballot64(lead2 && qany && span2 <= 1));
    ms.quads_same += (uint32_t)__popcll(ballot64(lead2 && qany && span2 == 0));
    widen(2); widen(16);
    const int span4 = max(max(qhi[0] - qlo[0], qhi[1] - qlo[1]), qhi[2] - qlo[2]);
    const bool lead4 = (lane & 27) == 0;                     // one lane per quadrant
    ms.quadrants_live += (uint32_t)__popcll(ballot64(lead4 && qany));
    ms.quadrants_fit444 += (uint32_t)__popcll(ballot64(lead4 && qany && span4 <= 2));
    ms.greedy_blocks += (uint32_t)nb;
    if (nb <= 2) ++ms.greedy_le2;
    if (nb <= 3) ++ms.greedy_le3;
    if (nb <= 4) ++ms.greedy_le4;
}

// [GL] tri(level): trilinear, texel centres, REPEAT (or clamp).  `level` is wave-uniform; must be
// called in wave-uniform control flow with at least one lane `act`.  Lanes without `act` help
// fetch the block and return garbage-free zeros / unused values.
// Over the shared pieces above: the choice between the cooperative block (COOP, every live footprint inside the block
// at the anchor) and the per-lane gather, the per-lane gather itself (texel loads in phases of 2 + 2 + 4, or one
// footprint record with CELLS), and where the issue priority (PRIO) is raised and dropped.
template <bool WRAP, VctLevelForm LEVEL>
__device__ __forceinline__ F4 sample_level(const ChainRef& chain, const VctLevelRef lv,
                                           float ux, float uy, float uz, bool act, unsigned long long am,
                                           float4* __restrict__ blk, const LaneBlock& lb, MarchStats& ms,
                                           const char* __restrict__ cells = nullptr) {
    constexpr bool COOP = (LEVEL & LF_COOP) != 0, LOOSE = (LEVEL & LF_LOOSE) != 0, CELLS = (LEVEL & LF_CELLS) != 0;
    constexpr bool PRIO = (LEVEL & LF_PRIO) != 0, NARROW = (LEVEL & LF_NARROW) != 0, CHAIN = (LEVEL & LF_CHAIN) != 0;
    // `am` is ballot64(act), passed in so that compound predicates are ANDed as lane masks on the
    // scalar unit (a ballot of `x && y` costs a v_cndmask + v_cmp_ne pair to materialise the bool).
    // Issue priority raised from here until the sample's loads are out (round 6): a wave that is forming
    // addresses gets its instructions ahead of the waves that are folding texels, so its loads leave earlier and more of
    // their latency lies under the other waves' arithmetic (A/B, 4 interleaved rounds: kernel -1.7 %, one-stream step
    // -1.3 %, vct_gi_pass -0.9 % on the atrium; street 4K -0.5 %).  PRIO is a template parameter: the launches of whole frames
    // take the instantiation with it, slab launches the one without -- there the priority goes to the specular waves, the
    // tail of a short launch (spec_prio; 8-way slabs 0.0881 ms with that against 0.0900 with this).  The same choice behind
    // a wave-uniform flag cost the default kernel 60 B of scratch per lane.
    if (PRIO) __builtin_amdgcn_s_setprio(1);
    const int m = lv.m;
    const Footprint f = footprint_of(lv, ux, uy, uz);
    const float a = f.a, b = f.b, c = f.c;
    const int i0 = f.i0, j0 = f.j0, k0 = f.k0;
    const uint32_t MX = lv.mask_x, MY = MX << 1, MZ = MX << 2;
    const LevelBuf lvb = level_buf<CHAIN>(chain, lv);
    const vct_v4i32 tb = lvb.tb;
    const uint32_t so = lvb.soffset;

    F4 r = {0.0f, 0.0f, 0.0f, 0.0f};
    const Anchor an = anchor_of(f, anchor_lane(am));          // (without COOP nothing reads these two: compiled away)
    const BlockFit fit = block_fit(f, an, am);
    if (COOP && fit.out == 0ull) {
        const float4 d = texel_f32(tb, block_texel_index<WRAP>(lv, an, lb), so);
        if (PRIO) __builtin_amdgcn_s_setprio(0);
        const bool any_texel = block_texel_mask(d) != 0ull;
        if (VCT_STATS) { if (any_texel) ++ms.coop_hit; else ++ms.coop_zero; }
        if (any_texel) {     // all 64 texels zero: every footprint sums to exactly +0
            blk[lb.lane] = d;
            wave_sync();
            r = gather_block<NARROW>(blk + block_slot(act, fit.dx, fit.dy, fit.dz), a, b, c);
        }
    } else {
      if (VCT_STATS) per_lane_census(ms, f, act, am, lb.lane);
      if (act) {
        uint32_t mx0, mx1, my0, my1, mz0, mz1;
        if (WRAP) {
            if (!CELLS) {
                // the dilated coordinates from the table the anchor path reads with scalar loads -- here one 4-byte VECTOR
                // load per axis (a 4 KiB table, cache resident) instead of ten vector instructions, half of them 4-cycle ones
                const uint32_t m4 = (uint32_t)m << 2;
                const char* lutb = (const char*)lb.lut_vec;      // (entries are spread3(i) << 2)
                mx0 = *(const uint32_t*)(lutb + (((uint32_t)i0 << 2) & m4)) >> 2;
                my0 = *(const uint32_t*)(lutb + (((uint32_t)j0 << 2) & m4)) >> 1;
                mz0 = *(const uint32_t*)(lutb + (((uint32_t)k0 << 2) & m4));
            } else {
                // (the instantiation with footprint records serves volumes that do NOT fit the caches: every sample is a
                // per-lane one and the memory pipe is what binds -- the table's three loads per sample cost it 1-3 %)
                mx0 = vct_spread3((uint32_t)i0 & (uint32_t)m);
                my0 = vct_spread3((uint32_t)j0 & (uint32_t)m) << 1;
                mz0 = vct_spread3((uint32_t)k0 & (uint32_t)m) << 2;
            }
            mx1 = ((mx0 | ~MX) + 1u) & MX;      // dilated increment, wraps at N
            my1 = ((my0 | ~MY) + 2u) & MY;
            mz1 = ((mz0 | ~MZ) + 4u) & MZ;
        } else {
            const int ci0 = min(max(i0, 0), m), ci1 = min(max(i0 + 1, 0), m);
            const int cj0 = min(max(j0, 0), m), cj1 = min(max(j0 + 1, 0), m);
            const int ck0 = min(max(k0, 0), m), ck1 = min(max(k0 + 1, 0), m);
            mx0 = vct_spread3((uint32_t)ci0); mx1 = vct_spread3((uint32_t)ci1);
            my0 = vct_spread3((uint32_t)cj0) << 1; my1 = vct_spread3((uint32_t)cj1) << 1;
            mz0 = vct_spread3((uint32_t)ck0) << 2; mz1 = vct_spread3((uint32_t)ck1) << 2;
        }
        if (!CELLS) {
            // eight typed-buffer loads: every texel arrives as four floats.  Phases of 2 + 2 + 4 texels: the first phase is
            // where most else is still live (both planes' addresses, all weight inputs), the last one where least is
            // (A/B: 4 + 4 spills five registers at 72 VGPRs and runs 1-2.5 % slower; pairs only: slower on the street)
            const float a0 = 1.0f - a, b0 = 1.0f - b, c0 = 1.0f - c;
            const float ab00 = a0 * b0, ab10 = a * b0, ab01 = a0 * b, ab11 = a * b;
            {
                const float4 f0 = texel_f32(tb, mx0 | my0 | mz0, so), f1 = texel_f32(tb, mx1 | my0 | mz0, so);
                const float w0 = ab00 * c0, w1 = ab10 * c0;
#define VCT_ACC(ch) r.ch = w0 * f0.ch; r.ch = fmaf(w1, f1.ch, r.ch);
                VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
            }
            __builtin_amdgcn_sched_barrier(0);
            {
                const float4 f2 = texel_f32(tb, mx0 | my1 | mz0, so), f3 = texel_f32(tb, mx1 | my1 | mz0, so);
                const float w2 = ab01 * c0, w3 = ab11 * c0;
#define VCT_ACC(ch) r.ch = fmaf(w2, f2.ch, r.ch); r.ch = fmaf(w3, f3.ch, r.ch);
                VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (NARROW) {       // phases of 2 + 2 + 2 + 2
                {
                    const float4 f4 = texel_f32(tb, mx0 | my0 | mz1, so), f5 = texel_f32(tb, mx1 | my0 | mz1, so);
                    const float w4 = ab00 * c, w5 = ab10 * c;
#define VCT_ACC(ch) r.ch = fmaf(w4, f4.ch, r.ch); r.ch = fmaf(w5, f5.ch, r.ch);
                    VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
                }
                __builtin_amdgcn_sched_barrier(0);
                {
                    const float4 f6 = texel_f32(tb, mx0 | my1 | mz1, so), f7 = texel_f32(tb, mx1 | my1 | mz1, so);
                    if (PRIO) __builtin_amdgcn_s_setprio(0);
                    const float w6 = ab01 * c, w7 = ab11 * c;
#define VCT_ACC(ch) r.ch = fmaf(w6, f6.ch, r.ch); r.ch = fmaf(w7, f7.ch, r.ch);
                    VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
                }
            } else {
                const float4 f4 = texel_f32(tb, mx0 | my0 | mz1, so), f5 = texel_f32(tb, mx1 | my0 | mz1, so);
                const float4 f6 = texel_f32(tb, mx0 | my1 | mz1, so), f7 = texel_f32(tb, mx1 | my1 | mz1, so);
                if (PRIO) __builtin_amdgcn_s_setprio(0);
                const float w4 = ab00 * c, w5 = ab10 * c, w6 = ab01 * c, w7 = ab11 * c;
#define VCT_ACC(ch) r.ch = fmaf(w4, f4.ch, r.ch); r.ch = fmaf(w5, f5.ch, r.ch); r.ch = fmaf(w6, f6.ch, r.ch); r.ch = fmaf(w7, f7.ch, r.ch);
                VCT_ACC(x) VCT_ACC(y) VCT_ACC(z) VCT_ACC(w)
#undef VCT_ACC
            }
        } else {
            // Footprint records (round 5; vct_set_footprint_records): a per-lane sample of a level >= 1 is ONE 32-byte fetch of
            // the footprint's 8 texels (vct_volume.hip k_build_cells) instead of eight 4-byte ones from 2-4 cache lines.  Same
            // bits.  Dense random 1024^3 chain + random G-buffer (the one HBM-bound case): 5.61 -> 2.86 ms; cache-resident
            // scenes: street at 1024^3 / 4K 2.72 -> 2.70 ms, atrium 0.611 -> 0.613 (profiles/experiments/README.md).  Off
            // unless the context asks for it.
            uint32_t t[8];
            const uint32_t* __restrict__ base = chain.base + lv.off;
            if (WRAP && lv.off != 0u) {     // (CELLS instantiations are launched with records present)
                // footprint record of the lower corner: the 8 texels as 32 contiguous bytes (levels >= 1; Morton index * 32
                // = byte offset of the record, < 2^32 for every level but the first of a 2048^3 grid, which has none)
                const char* cb = cells + ((size_t)lv.off << 5);
                const uint32_t ro = (mx0 | my0 | mz0) << 5;
                const uint4 lo = *(const uint4*)(cb + ro);
                const uint4 hi = *(const uint4*)(cb + ro + 16u);
                t[0] = lo.x; t[1] = lo.y; t[2] = lo.z; t[3] = lo.w;
                t[4] = hi.x; t[5] = hi.y; t[6] = hi.z; t[7] = hi.w;
            } else {
                t[0] = base[mx0 | my0 | mz0]; t[1] = base[mx1 | my0 | mz0];
                t[2] = base[mx0 | my1 | mz0]; t[3] = base[mx1 | my1 | mz0];
                t[4] = base[mx0 | my0 | mz1]; t[5] = base[mx1 | my0 | mz1];
                t[6] = base[mx0 | my1 | mz1]; t[7] = base[mx1 | my1 | mz1];
            }
            if (PRIO) __builtin_amdgcn_s_setprio(0);
            const float a0 = 1.0f - a, b0 = 1.0f - b, c0 = 1.0f - c;
            const float wg[8] = {(a0 * b0) * c0, (a * b0) * c0, (a0 * b) * c0, (a * b) * c0,
                                 (a0 * b0) * c,  (a * b0) * c,  (a0 * b) * c,  (a * b) * c};
            r.x = wg[0] * unorm8_of<0, LOOSE>(t[0]);
            r.y = wg[0] * unorm8_of<8, LOOSE>(t[0]);
            r.z = wg[0] * unorm8_of<16, LOOSE>(t[0]);
            r.w = wg[0] * unorm8_of<24, LOOSE>(t[0]);
#pragma unroll
            for (int i = 1; i < 8; ++i) {
                r.x = fmaf(wg[i], unorm8_of<0, LOOSE>(t[i]), r.x);
                r.y = fmaf(wg[i], unorm8_of<8, LOOSE>(t[i]), r.y);
                r.z = fmaf(wg[i], unorm8_of<16, LOOSE>(t[i]), r.z);
                r.w = fmaf(wg[i], unorm8_of<24, LOOSE>(t[i]), r.w);
            }
        }
      }
    }
    // (every path above lowers the priority behind its last load -- a new one has to as well; one more s_setprio 0 here
    // would be a repeat on all of them: profiles/experiments/README.md, round 17)
    return r;
}

// The same sample with block reuse (BlockDesc above): cooperative, exact, no footprint records.  `blk` is the wave's
// FIRST slab whichever level of the step this is; SLAB says which slab this sample fills (0: blk, 1: blk + 64) and
// `held` describes the block in the second one.
// Over the shared pieces: the fit test runs against the held block first and against a fresh anchor only when that
// fails, and a fresh block of the second slab becomes the held one.
template <bool WRAP, VctLevelForm LEVEL, int SLAB>
__device__ __forceinline__ F4 sample_level_reuse(const ChainRef& chain, const VctLevelRef lv,
                                                 float ux, float uy, float uz, bool act, unsigned long long am,
                                                 float4* __restrict__ blk, const LaneBlock& lb, MarchStats& ms,
                                                 BlockDesc& held) {
    constexpr bool PRIO = (LEVEL & LF_PRIO) != 0, NARROW = (LEVEL & LF_NARROW) != 0, CHAIN = (LEVEL & LF_CHAIN) != 0;
    // (GL_REPEAT only: k_trace_tile_split switches the path off in clamp mode)
    if (PRIO) __builtin_amdgcn_s_setprio(1);
    const Footprint f = footprint_of(lv, ux, uy, uz);
    // how the sample is served -- an integer, not flags: wave-uniform integers stay in one SGPR, while booleans merged
    // across branches become lane masks.  0: by no block (yet), 1: by an all-zero block, 2: by the block of the wave's
    // slabs in which this lane's footprint starts at float4 `at` (set on the routes that gather and read on no other:
    // a value for the rest is a v_mov on the routes that do not need it)
    int mode = 0, at;
    // the second slab holds a block of this level: compared on the scalar unit, a sample without one pays nothing more
    if ((held.id & ~1u) == lv.off) {
        const BlockDesc cd = held;
        const BlockFit fit = block_fit(f, cd.an, am);
        if (VCT_STATS) {
            const Anchor fresh = anchor_of(f, anchor_lane(am));
            ++ms.reuse[SLAB][0];
            if (fit.out == 0ull) { ++ms.reuse[SLAB][1]; if (!(cd.id & 1u)) ++ms.reuse[SLAB][2]; }
            if (fresh.x == cd.an.x && fresh.y == cd.an.y && fresh.z == cd.an.z) ++ms.reuse[SLAB][3];
        }
        if (fit.out == 0ull) {
            // every live footprint lies inside it: the block is in LDS already, or known to be all zero -- nothing to fetch
            if (PRIO) __builtin_amdgcn_s_setprio(0);
            mode = 1 + (int)(cd.id - lv.off);       // 1 + the zero bit, as a difference: its range is the compiler's to guess (below)
            at = block_slot(act, fit.dx, fit.dy, fit.dz) + 64;
        }
    }
    if (mode == 0) {
        // sample_level's cooperative block, into this sample's slab
        const Anchor an = anchor_of(f, anchor_lane(am));
        const BlockFit fit = block_fit(f, an, am);
        if (fit.out == 0ull) {
            const uint32_t idx = block_texel_index<true>(lv, an, lb);
            const LevelBuf lvb = level_buf<CHAIN>(chain, lv);
            const float4 d = texel_f32(lvb.tb, idx, lvb.soffset);
            if (PRIO) __builtin_amdgcn_s_setprio(0);
            const unsigned long long any_texel = block_texel_mask(d);
            if (VCT_STATS) { if (any_texel != 0ull) ++ms.coop_hit; else ++ms.coop_zero; }
            // (the descriptor's zero bit is written as a constant on either side of the ballot's branch: formed from
            // the ballot, it came back from the vector unit through a v_cndmask and a v_readfirstlane)
            mode = 1;
            if (SLAB == 1) held = {lv.off, an};
            if (any_texel != 0ull) {
                mode = 2;
                if (SLAB == 1) held.id = lv.off | 1u;
                blk[SLAB * 64 + lb.lane] = d;
                wave_sync();
                at = block_slot(act, fit.dx, fit.dy, fit.dz) + SLAB * 64;
            }
        }
    }
    // Round 18: the word is tested by two conditions of which the compiler cannot tell that one is the other's complement
    // (it does not know that the word stays below 3).  Routes told apart by `if ... else` or by early returns come out of
    // the compiler's structured control flow with a lane-mask flag -- set to -1 in front of the first side, cleared
    // behind it, and-not-ed with exec and branched on in front of the second: six scalar instructions of routing around
    // the gather where these two compares and branches are four, and the four v_mov of a zero result executed on the
    // per-lane route as well.  (Routes that end in returns or gotos of their own compile to a word like this one, made
    // by the compiler, or to more such flags; the gather once per route put the kernel into scratch:
    // profiles/experiments/README.md, round 18.)
    F4 r;
    if (mode == 2) r = gather_block<NARROW>(blk + at, f.a, f.b, f.c);
    if (mode < 2) {
        r = {0.0f, 0.0f, 0.0f, 0.0f};     // all 64 texels zero: every footprint sums to exactly +0
        // incoherent footprints: the per-lane gather, which leaves the slabs and the descriptor alone
        if (mode == 0) r = sample_level<WRAP, level_form_without(LEVEL, LF_COOP | LF_REUSE)>(chain, lv, ux, uy, uz, act, am, blk, lb, ms);
    }
    return r;
}

// level SLAB (0: first, 1: second) of a march step, with or without block reuse; `blk` is the wave's first slab
template <bool WRAP, VctLevelForm LEVEL, int SLAB>
__device__ __forceinline__ F4 sample_step_level(const VctTraceParams& p, const VctLevelRef lv, float ux, float uy, float uz,
                                                bool act, unsigned long long am, float4* __restrict__ blk,
                                                const LaneBlock& lb, MarchStats& ms, BlockDesc& held) {
    if constexpr ((LEVEL & LF_REUSE) != 0) {
        static_assert(WRAP && (LEVEL & LF_COOP) && !(LEVEL & LF_CELLS), "block reuse: cooperative sampler, GL_REPEAT, no footprint records");
        return sample_level_reuse<WRAP, LEVEL, SLAB>(lb.chain, lv, ux, uy, uz, act, am, blk, lb, ms, held);
    } else {
        return sample_level<WRAP, LEVEL>(lb.chain, lv, ux, uy, uz, act, am, blk + SLAB * 64, lb, ms, p.cells_biased);
    }
}

// Anisotropic option (oracle/vct_oracle.h "anisotropic (directional) mip volumes"): a level >= 1 is
// sampled from the three directional chains the cone direction faces, weighted by dir^2.  The chain
// of an axis depends on the sign of that direction component, which is per lane: when the live
// lanes disagree the axis is sampled once per sign with the lanes split by mask (rare: a tile's
// cones are near-parallel), so sample_level always sees a wave-uniform chain.
// Over the shared pieces (footprint_of, anchor_of, block_fit, block_texel_index, block_slot, gather_block) its
// cooperative GL_REPEAT path adds: one set-up for all six chains, which share their geometry; per axis one or two
// block loads by the lanes' signs, decoded into the slab of the sign (blk, or blk + p.aniso_alt_slab); and the dir^2
// weighting of the three gathers.  Footprints that do not fit one block, clamp mode and the per-lane sampler go
// through sample_level once per axis and sign.
struct AnisoCone {
    float wx, wy, wz;       // dir.x^2, dir.y^2, dir.z^2
    bool nx, ny, nz;        // component not >= 0: the chain pre-integrated towards -axis
};

template <bool WRAP, bool COOP>
__device__ __forceinline__ F4 sample_aniso(const VctTraceParams& p, const VctLevelRef lv, float ux,
                                           float uy, float uz, bool act, unsigned long long m,
                                           float4* __restrict__ blk, const LaneBlock& lb, const AnisoCone& ac,
                                           MarchStats& ms) {
    constexpr VctLevelForm LEVEL = level_form(COOP ? LF_COOP : LF_NONE);      // of the samples that go through sample_level
    // chain pointer of direction d such that (pointer + lv.off) is the level's first texel
    auto chain_of = [&](int d) { return p.aniso + (size_t)d * p.aniso_stride - p.level_off[1]; };
    const unsigned long long mx = ballot64(ac.nx) & m, my = ballot64(ac.ny) & m, mz = ballot64(ac.nz) & m;
    F4 tx, ty, tz;
    bool done = false;
    if (COOP && WRAP) {
        // An axis whose live lanes disagree on the sign (cones along a coordinate axis have components ~0 of either
        // sign) fetches both of its chains into two slabs and every lane gathers from the one its sign selects.
        const Footprint f = footprint_of(lv, ux, uy, uz);
        const Anchor an = anchor_of(f, anchor_lane(m));
        const BlockFit fit = block_fit(f, an, m);
        if (fit.out == 0ull) {
            done = true;
            const uint32_t idx = block_texel_index<true>(lv, an, lb);
            const unsigned long long mneg[3] = {mx, my, mz};
            const bool lneg[3] = {ac.nx, ac.ny, ac.nz};
            uint32_t tpos[3], tneg[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {          // all block loads first (up to 6 in flight)
                tpos[k] = mneg[k] != m ? (chain_of(2 * k) + lv.off)[idx] : 0u;          // some lane is >= 0
                tneg[k] = mneg[k] != 0ull ? (chain_of(2 * k + 1) + lv.off)[idx] : 0u;   // some lane is < 0
            }
            const int slot = block_slot(act, fit.dx, fit.dy, fit.dz);
            float4* alt = p.aniso_alt_slab ? blk + p.aniso_alt_slab : blk;      // slab of the "towards -axis" chain
            F4 out3[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                F4 r = {0.0f, 0.0f, 0.0f, 0.0f};
                if (ballot64((tpos[k] | tneg[k]) != 0u) != 0ull) {
                    auto dec = [](uint32_t t) {
                        float4 d;
                        d.x = unorm8(t & 0xffu); d.y = unorm8((t >> 8) & 0xffu);
                        d.z = unorm8((t >> 16) & 0xffu); d.w = unorm8(t >> 24);
                        return d;
                    };
                    if (mneg[k] != m) blk[lb.lane] = dec(tpos[k]);
                    if (mneg[k] != 0ull) alt[lb.lane] = dec(tneg[k]);
                    wave_sync();
                    r = gather_block((lneg[k] ? alt : blk) + slot, f.a, f.b, f.c);
                }
                out3[k] = r;
            }
            tx = out3[0]; ty = out3[1]; tz = out3[2];
        }
    }
    if (!done) {
        // per axis: lanes that disagree on the sign are served in two masked passes
        auto axis_sample = [&](int axis, bool neg, unsigned long long mn) -> F4 {
            if (mn == 0ull) return sample_level<WRAP, LEVEL>(chain_ref(chain_of(2 * axis)), lv, ux, uy, uz, act, m, blk, lb, ms);
            if (mn == m) return sample_level<WRAP, LEVEL>(chain_ref(chain_of(2 * axis + 1)), lv, ux, uy, uz, act, m, blk, lb, ms);
            const F4 a = sample_level<WRAP, LEVEL>(chain_ref(chain_of(2 * axis)), lv, ux, uy, uz, act && !neg, m & ~mn, blk, lb, ms);
            const F4 b = sample_level<WRAP, LEVEL>(chain_ref(chain_of(2 * axis + 1)), lv, ux, uy, uz, act && neg, mn, blk, lb, ms);
            return neg ? b : a;
        };
        tx = axis_sample(0, ac.nx, mx);
        ty = axis_sample(1, ac.ny, my);
        tz = axis_sample(2, ac.nz, mz);
    }
    F4 r;
    r.x = ac.wx * tx.x; r.x = fmaf(ac.wy, ty.x, r.x); r.x = fmaf(ac.wz, tz.x, r.x);
    r.y = ac.wx * tx.y; r.y = fmaf(ac.wy, ty.y, r.y); r.y = fmaf(ac.wz, tz.y, r.y);
    r.z = ac.wx * tx.z; r.z = fmaf(ac.wy, ty.z, r.z); r.z = fmaf(ac.wz, tz.z, r.z);
    r.w = ac.wx * tx.w; r.w = fmaf(ac.wy, ty.w, r.w); r.w = fmaf(ac.wz, tz.w, r.w);
    return r;
}

// trace.fs:82-107 with the pixel-independent step sequence read from `tab`.
// The step table is read through the constant address space: a wave-uniform index then becomes one
// scalar s_load_dwordx16 instead of vector loads + v_readfirstlane, and the entry of step k+1 is
// requested while step k is being marched.
typedef const __attribute__((address_space(4))) VctStep* StepTable;

__device__ __forceinline__ VctStep load_step(StepTable t, int k) {
    VctStep s;
    s.dist = t[k].dist; s.occ_rcp = t[k].occ_rcp; s.occ_den = t[k].occ_den; s.frac = t[k].frac;
    s.level = t[k].level; s.level2 = t[k].level2; s.two_levels = t[k].two_levels; s.omf = t[k].omf;
    s.l1.off = t[k].l1.off; s.l1.mask_x = t[k].l1.mask_x; s.l1.fN = t[k].l1.fN; s.l1.m = t[k].l1.m;
    s.l2.off = t[k].l2.off; s.l2.mask_x = t[k].l2.mask_x; s.l2.fN = t[k].l2.fN; s.l2.m = t[k].l2.m;
    return s;
}

// One march step with the table entry `st`; `live` = ballot of the lanes still marching.  A macro, not a lambda: the
// plain loop of the anisotropic march must compile exactly as it did before the unrolled form existed (a lambda cost it 7 %).
//   position: trace.fs:98 + :61-63  (q * 0.5f is exact, so fmaf(q, .5, .5) is the oracle's q*.5f + .5f; a coordinate below
//             div_const's 2^-100 domain gives |q| < 2^-26 and u = 0.5 either way)
//   sample:   textureLod = blend of the two levels (frac == 0: one level, decided in the table)
//   composite: trace.fs:100 (colour), :101 (occlusion), :102 (alpha), front to back
#define VCT_MARCH_STEP(st, act, live)                                                                        \
        const float px = start.x + dir.x * st.dist; \
        const float py = start.y + dir.y * st.dist; \
        const float pz = start.z + dir.z * st.dist; \
        const float ux = fmaf(div_const<FASTDIV>(px, p.half_G_aux, p.half_G_rcp), 0.5f, 0.5f); \
        const float uy = fmaf(div_const<FASTDIV>(py, p.half_G_aux, p.half_G_rcp), 0.5f, 0.5f); \
        const float uz = fmaf(div_const<FASTDIV>(pz, p.half_G_aux, p.half_G_rcp), 0.5f, 0.5f); \
        F4 vc = (ANISO && st.level >= 1) ? sample_aniso<WRAP, COOP>(p, st.l1, ux, uy, uz, act, live, blk, lb, ac, ms) \
                                         : sample_step_level<WRAP, LEVEL, 0>(p, st.l1, ux, uy, uz, act, live, blk, lb, ms, held); \
        if (st.two_levels) { \
            const F4 t2 = ANISO ? sample_aniso<WRAP, COOP>(p, st.l2, ux, uy, uz, act, live, blk + 64, lb, ac, ms) \
                                : sample_step_level<WRAP, LEVEL, 1>(p, st.l2, ux, uy, uz, act, live, blk, lb, ms, held); \
            const float g = st.omf;      /* 1 - frac, from the table */ \
            vc.x = fmaf(st.frac, t2.x, g * vc.x); \
            vc.y = fmaf(st.frac, t2.y, g * vc.y); \
            vc.z = fmaf(st.frac, t2.z, g * vc.z); \
            vc.w = fmaf(st.frac, t2.w, g * vc.w); \
        } \
        if (act) { \
            const float oma = 1.0f - alpha; \
            cr = fmaf(oma, vc.x, cr); \
            cg = fmaf(oma, vc.y, cg); \
            cb = fmaf(oma, vc.z, cb); \
            occ = occ + div_const<FASTDIV>(oma * vc.w, st.occ_den, st.occ_rcp); \
            alpha = fmaf(oma, vc.w, alpha); \
            ++steps; \
        }

// Sky light (include/vct.h "sky light"; p.sky: the folded polynomial coefficients [9][3]): what a marched cone adds behind
// its loop -- the part 1 - alpha of its footprint that reached open air, times the sky's radiance along the cone.  The
// chain is csrc/vct_sky_check.h vct_sky_eval's, operation for operation.  The 27 coefficients are wave-uniform scalar
// loads through the constant address space, issued here and not held across the march; of the march only `alpha` and the
// direction outlive the loop.  fmaxf is maxNum: a NaN sum gives 0, a NaN alpha T = 0, and fmaf(T, sky, NaN) stays NaN.
typedef const __attribute__((address_space(4))) float* SkyPoly;
__device__ __forceinline__ void sky_epilogue(const VctTraceParams& p, bool alive, F3 d, float alpha, float& cr, float& cg, float& cb) {
    // (the pointer and the direction through empty asm: where one direction serves several marches -- the class loop of the
    // GLOSS forms -- the loads and the five products are loop-invariant, and hoisted they live across every march: 4 VGPRs
    // and the 8th wave of the HALF form, 6 more spilled SGPRs and 8 B of scratch in the PRIO form)
    SkyPoly q = (SkyPoly)p.sky;
    float x = d.x, y = d.y, z = d.z;
    asm volatile("" : "+s"(q), "+v"(x), "+v"(y), "+v"(z));
    const float xy = x * y, yz = y * z, zz = fmaf(3.0f * z, z, -1.0f), xz = x * z, xxyy = fmaf(x, x, -(y * y));
    const float T = fmaxf(1.0f - alpha, 0.0f);
    float sky[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = q[c];
        s = fmaf(q[3 + c], y, s);
        s = fmaf(q[6 + c], z, s);
        s = fmaf(q[9 + c], x, s);
        s = fmaf(q[12 + c], xy, s);
        s = fmaf(q[15 + c], yz, s);
        s = fmaf(q[18 + c], zz, s);
        s = fmaf(q[21 + c], xz, s);
        s = fmaf(q[24 + c], xxyy, s);
        sky[c] = fmaxf(s, 0.0f);
    }
    if (alive) {          // a lane that is not alive keeps the zero cone
        cr = fmaf(T, sky[0], cr);
        cg = fmaf(T, sky[1], cg);
        cb = fmaf(T, sky[2], cb);
    }
}

// REUSE: `held` describes the block in the wave's second slab (BlockDesc); the caller keeps it across the cones of a wave
// SKY: VCT_SKY_INSIDE the sky epilogue above, behind the loops; VCT_SKY_ALPHA the alpha the epilogue would take goes to
// *alpha_out and the caller applies it (the class loop of the GLOSS forms: once per lane, behind the loop).  The loop body
// is the same in all three.
#define VCT_SKY_NONE 0
#define VCT_SKY_INSIDE 1
#define VCT_SKY_ALPHA 2
template <bool WRAP, int FASTDIV, VctMarchForm MARCH, int SKY = VCT_SKY_NONE>
__device__ __forceinline__ F4 cone_march(const VctTraceParams& p, bool alive, F3 start, F3 dir,
                                         const VctStep* tab_global, int n,
                                         float4* __restrict__ blk, const LaneBlock& lb,
                                         int& steps_out, MarchStats& ms, BlockDesc& held, float* alpha_out = nullptr) {
    constexpr bool COOP = (MARCH & MF_COOP) != 0, ANISO = (MARCH & MF_ANISO) != 0;
    constexpr VctLevelForm LEVEL = march_level_form(MARCH, FASTDIV);
    const StepTable tab = (StepTable)tab_global;
    float cr = 0.0f, cg = 0.0f, cb = 0.0f, occ = 0.0f;
    int steps = 0;
    AnisoCone ac = {0.0f, 0.0f, 0.0f, false, false, false};
    if (ANISO) {
        ac.wx = dir.x * dir.x; ac.wy = dir.y * dir.y; ac.wz = dir.z * dir.z;
        ac.nx = !(dir.x >= 0.0f); ac.ny = !(dir.y >= 0.0f); ac.nz = !(dir.z >= 0.0f);
    }
    // A lane whose sample position is not finite (start or direction NaN / inf: a degenerate tangent frame, the camera on
    // the surface point -- include/vct.h "G-buffer contract") has NaN filter weights at every step, so the oracle's first
    // sample is NaN whatever the texels hold and its march ends there: one step, (NaN, NaN, NaN, NaN).  The cooperative
    // sampler skips the weights when its block is all zero and would hand such a lane +0 and let it march on, so these
    // lanes start with alpha = NaN: trace.fs:94's alpha < max_alpha never holds for them, they take no part in the march
    // and get the oracle's result below.  (x * 0 is NaN for NaN and inf, else +-0, and the chain ends in + 0.0f, so a
    // finite position gives exactly +0 whatever its size: nothing here can overflow.  A position that is finite at the
    // first step stays finite inside the contract: |dir| <= 1, dist < max_distance.)
    const float wx = start.x + dir.x * p.vs, wy = start.y + dir.y * p.vs, wz = start.z + dir.z * p.vs;      // step 0: dist = vs
    float alpha = fmaf(wx, 0.0f, fmaf(wy, 0.0f, fmaf(wz, 0.0f, 0.0f)));
    const unsigned long long alive_mask = ballot64(alive);
    if constexpr (!ANISO) {
    // Two steps per loop iteration (A/B: 0.6281 -> 0.6216 ms at 256^3, 2.659 -> 2.623 ms at 512^3 / 4K; not the anisotropic
    // march: its body, twice, spills and ran 7x slower), the table entries ping-pong between two register sets: the entry of step k + 1 is
    // requested while step k is marched and is never copied (the rotating form below moves 12 SGPRs per step, and
    // the scalar pipe is the march's second bound).
    // (the step body goes through a lambda here: measured 2 % faster than the macro expanded in place, while the
    // plain loop below wants the macro expanded in place -- register allocation differs, the instructions do not)
    auto march_step = [&](const VctStep& st, const bool act, const unsigned long long live) { VCT_MARCH_STEP(st, act, live) };
    VctStep ea = load_step(tab, 0), eb = ea;
    for (int k = 0; k < n;) {
        {
            const bool act = alive && (alpha < p.max_alpha);     // trace.fs:94 (dist < MAX: table)
            const unsigned long long live = ballot64(alpha < p.max_alpha) & alive_mask;
            if (live == 0ull) break;
            if (VCT_STATS) { ++ms.wave_steps; ms.lane_steps += (uint32_t)__popcll(live); }
            eb = load_step(tab, k + 1 < n ? k + 1 : k);
            march_step(ea, act, live);
            if (++k >= n) break;
        }
        {
            const bool act = alive && (alpha < p.max_alpha);
            const unsigned long long live = ballot64(alpha < p.max_alpha) & alive_mask;
            if (live == 0ull) break;
            if (VCT_STATS) { ++ms.wave_steps; ms.lane_steps += (uint32_t)__popcll(live); }
            ea = load_step(tab, k + 1 < n ? k + 1 : k);
            march_step(eb, act, live);
            ++k;
        }
    }
    } else {
    VctStep nxt = load_step(tab, 0);
    for (int k = 0; k < n; ++k) {
        const bool act = alive && (alpha < p.max_alpha);     // trace.fs:94 (dist < MAX: table)
        const unsigned long long live = ballot64(alpha < p.max_alpha) & alive_mask;
        if (live == 0ull) break;
        if (VCT_STATS) { ++ms.wave_steps; ms.lane_steps += (uint32_t)__popcll(live); }
        const VctStep st = nxt;
        nxt = load_step(tab, k + 1 < n ? k + 1 : k);
        VCT_MARCH_STEP(st, act, live)
    }
    }
    // a lane that never marched because it started with alpha = NaN: in the oracle trace.fs:94 holds once (its alpha starts
    // at 0), the sample is NaN, and then alpha is NaN
    // (SKY: what trace.fs:94 saw last -- a lane that took no step has the oracle's initial 0, also where this march started
    // it with NaN; if the patch below applies, the cone is NaN whatever T is)
    [[maybe_unused]] const float alpha_seen = steps == 0 ? 0.0f : alpha;
    if (alive && steps == 0 && alpha != alpha && n > 0 && 0.0f < p.max_alpha) {
        cr = cg = cb = occ = __builtin_nanf("");
        steps = 1;
    }
    if constexpr (SKY == VCT_SKY_INSIDE) sky_epilogue(p, alive, dir, alpha_seen, cr, cg, cb);
    if constexpr (SKY == VCT_SKY_ALPHA) *alpha_out = alpha_seen;
    steps_out = steps;
    return {cr, cg, cb, occ};
}

// the march without block reuse
template <bool WRAP, int FASTDIV, VctMarchForm MARCH, int SKY = VCT_SKY_NONE>
__device__ __forceinline__ F4 cone_march(const VctTraceParams& p, bool alive, F3 start, F3 dir,
                                         const VctStep* tab_global, int n,
                                         float4* __restrict__ blk, const LaneBlock& lb,
                                         int& steps_out, MarchStats& ms) {
    static_assert(!(MARCH & MF_REUSE), "a march with block reuse takes the caller's descriptor");
    BlockDesc none = no_block();
    return cone_march<WRAP, FASTDIV, MARCH, SKY>(p, alive, start, dir, tab_global, n, blk, lb, steps_out, ms, none);
}

// `specular`: the wave marches the specular cone (the reuse counters are kept per kind of wave)
__device__ __forceinline__ void flush_stats(const VctTraceParams& p, const MarchStats& ms, int lane, bool specular = false) {
    if (VCT_STATS && p.stats && lane == 0) {
        for (int i = 0; i < 8; ++i)
            if (ms.reuse[i >> 2][i & 3]) atomicAdd(p.stats + 16 + (specular ? 8 : 0) + i, (unsigned long long)ms.reuse[i >> 2][i & 3]);
        const uint32_t v[16] = {ms.wave_steps, ms.lane_steps, ms.coop_zero, ms.coop_hit, ms.fallback,
                                ms.fallback_lanes, ms.fallback_fits, ms.greedy_blocks, ms.greedy_le2, ms.greedy_le3,
                                ms.greedy_le4, ms.quads_live, ms.quads_fit333, ms.quads_same, ms.quadrants_live,
                                ms.quadrants_fit444};
        for (int i = 0; i < 16; ++i)
            if (v[i]) atomicAdd(p.stats + i, (unsigned long long)v[i]);
    }
}

__constant__ float kConeDirs[18] = {0.0f, 0.0f, 1.0f,
                                    0.0f, 0.866025f, 0.5f,
                                    0.823639f, 0.267617f, 0.5f,
                                    0.509037f, -0.700629f, 0.5f,
                                    -0.509037f, -0.700629f, 0.5f,
                                    -0.823639f, 0.267617f, 0.5f};            // trace.fs:49-57
__constant__ float kConeWeights[6] = {0.25f, 0.15f, 0.15f, 0.15f, 0.15f, 0.15f};   // trace.fs:48

// ---- tile-level building blocks: what the tile kernels and the bounce do outside the march, written once --------
// Each performs the oracle's fp32 operations in the oracle's order.  The ones that read the G-buffer read it through
// the pointer they are given, where they are called: the callers stage those reads around the marches (k_trace_tile).
__device__ __forceinline__ LaneBlock make_lane_block(const VctTraceParams& p, int lane) {
    LaneBlock lb;
    lb.lane = lane;
    lb.chain = chain_ref(p.chain);
    lb.lut = (SpreadLut)p.spread_lut; lb.lut_vec = p.spread_lut;
    lb.sbx = vct_spread3((uint32_t)lane & 3u);
    lb.sby = vct_spread3(((uint32_t)lane >> 2) & 3u) << 1;
    lb.sbz = vct_spread3((uint32_t)lane >> 4) << 2;
    return lb;
}
// plane k of this lane's pixel; `gb` = the tile's G-buffer + the pixel's index inside the tile
__device__ __forceinline__ float gb_plane(const float* gb, int k) { return gb[k * VCT_TILE_PIX]; }
__device__ __forceinline__ F3 gb_planes3(const float* gb, int k) { return f3(gb_plane(gb, k), gb_plane(gb, k + 1), gb_plane(gb, k + 2)); }
__device__ __forceinline__ F3 cone_start(F3 P, F3 N, float vs) {                   // trace.fs:92
    return f3(P.x + N.x * vs, P.y + N.y * vs, P.z + N.z * vs);
}
// the cones' start point and the frame k0, k1, k2 their directions are combined in, from a fragment's Position_world,
// Normal_world, Tangent_world and BiTangent_world (G-buffer planes 0-11, or a caller's gather point)
__device__ __forceinline__ void cone_frame(F3 P, F3 Nw, F3 T, F3 B, float vs, F3& start, F3& k0, F3& k1, F3& k2) {
    // trace.fs:175: inverse(transpose(mat3(T,B,N))) = columns (BxN, NxT, TxB) / det
    const F3 c0 = cross3(B, Nw), c1 = cross3(Nw, T), c2 = cross3(T, B);
    const float inv_det = div_rn(1.0f, dot3(T, c0));
    k0 = f3(c0.x * inv_det, c0.y * inv_det, c0.z * inv_det);
    k1 = f3(c1.x * inv_det, c1.y * inv_det, c1.z * inv_det);
    k2 = f3(c2.x * inv_det, c2.y * inv_det, c2.z * inv_det);
    start = cone_start(P, Nw, vs);
}
__device__ __forceinline__ void cone_frame_from_gbuffer(const float* gb, float vs, F3& start, F3& k0, F3& k1, F3& k2) {
    const F3 P = gb_planes3(gb, 0), Nw = gb_planes3(gb, 3), T = gb_planes3(gb, 6), B = gb_planes3(gb, 9);
    cone_frame(P, Nw, T, B, vs, start, k0, k1, k2);
}
// direction of diffuse cone i in the frame (b0, b1, b2)                             trace.fs:196-199
__device__ __forceinline__ F3 cone_dir(F3 b0, F3 b1, F3 b2, int i) {
    const float* d = &kConeDirs[3 * i];
    const float ddx = d[0], ddy = d[1], ddz = d[2];
    return normalize3(f3(b0.x * ddx + b1.x * ddy + b2.x * ddz, b0.y * ddx + b1.y * ddy + b2.y * ddz,
                         b0.z * ddx + b1.z * ddy + b2.z * ddz));
}
// the weighted sum of the diffuse cones: an fma chain over cones 0..5, in that order (V4: F4, or the float4 parked in LDS)
template <class V4>
__device__ __forceinline__ F4 fold_cone(F4 ind, int i, V4 c) {
    const float wgt = kConeWeights[i];
    return {fmaf(wgt, c.x, ind.x), fmaf(wgt, c.y, ind.y), fmaf(wgt, c.z, ind.z), fmaf(wgt, c.w, ind.w)};
}
// The diffuse gather of one point: the six cones of the frame (b0, b1, b2), one after the other, folded in cone order.
// march(dir, st) marches one cone and leaves its step count in st; per_cone(i, cone, st) is the caller's business with
// cone i (debug outputs).  `total` grows by the lane's executed steps.                            trace.fs:196-199
template <class March, class PerCone>
__device__ __forceinline__ F4 gather_six_cones(F3 b0, F3 b1, F3 b2, int& total, March march, PerCone per_cone) {
    F4 ind = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
        int st;
        const F4 c = march(cone_dir(b0, b1, b2, i), st);
        total += st;
        ind = fold_cone(ind, i, c);
        per_cone(i, c, st);
    }
    return ind;
}
// the specular cone runs along reflect(-E, N) with the bump normal N (planes 12-14)     trace.fs:217-218
// E, the unit vector from the point to the camera (:181), is the composite's too (:213): the one copy of its arithmetic
__device__ __forceinline__ F3 eye_dir(F3 P, const float cam[3]) {
    return normalize3(f3(cam[0] - P.x, cam[1] - P.y, cam[2] - P.z));                    // :181
}
__device__ __forceinline__ F3 specular_dir(F3 E, F3 N) {
    return normalize3(reflect3(f3(E.x * -1.0f, E.y * -1.0f, E.z * -1.0f), N));          // :217
}
// tile / tiles_x, both below 2^31, by the launch's multiplier and shift (vct_tilediv.h; set by vct_launch_trace)
__device__ __forceinline__ int tile_row_of(const VctTraceParams& p, int tile) {
    return (int)vct_tilediv((uint32_t)tile, (uint32_t)p.tiles_x, p.tile_mul, p.tile_shift);
}
// config.debug_outputs: cone i's raw vec4 and step count.  `pixel()` re-derives the pixel's index per store (see k_trace_tile)
template <class Pixel>
__device__ __forceinline__ void store_debug_cone(const VctTraceParams& p, Pixel pixel, int i, F4 c, int st,
                                                 bool alive, bool in_frame) {
    if (p.dbg_cones && alive) {
        float* d = p.dbg_cones + pixel() * 28 + 4 * i;
        d[0] = c.x; d[1] = c.y; d[2] = c.z; d[3] = c.w;
    }
    if (p.dbg_steps && in_frame) p.dbg_steps[pixel() * 7 + i] = (uint8_t)st;
}
// a discarded pixel keeps the clear colour (alpha 1)                                VCT.h:156-159
__device__ __forceinline__ float clear_colour(const VctTraceParams& p) { return p.ambient < 0.5f ? 0.5f : 1.0f; }

// The composite of one pixel inside the frame from its gathered diffuse cones `ind`, its specular cone `sc` and its eye
// vector E (eye_dir: the specular cone's set-up has it already), read from planes 12-22 of `gb`        trace.fs:179-227
// L = normalize(LightDirection) is the launch's: p.light_unit, the same bits from the host (vct_tilediv.h).
// COMP: the Show* ternaries (include/vct.h) as selects on the wave-uniform mask, and the per-component outputs.
// VCT_SHOW_ALL selects every unmasked value, and without COMP every select is decided here: the operations and their
// order are the same in all three cases.
// COMP with VCT_COMP_EMISSION in the mask word (wave-uniform): out.rgb = ((A + D) + S) + E, one fp32 add per channel, last,
// E from the launch's pixel-emission planes at em_offset() = tile * 192 + lane (include/vct.h "emissive materials").
// `shininess`: the exponent of :213 -- p.shininess, or the lane's gloss class's (the SF_GLOSS forms of k_trace_tile_split).
template <bool COMP, class V4, class Pixel, class EmOffset>
__device__ __forceinline__ void composite(const VctTraceParams& p, const float* gb, F4 ind, V4 sc, F3 E,
                                          bool alive, Pixel pixel, EmOffset em_offset, float shininess) {
    const F3 N = gb_planes3(gb, 12);
    const float alb_r = gb_plane(gb, 15), alb_g = gb_plane(gb, 16), alb_b = gb_plane(gb, 17), alb_a = gb_plane(gb, 18);
    const float shadow = gb_plane(gb, 22);
    const F3 L = f3(p.light_unit[0], p.light_unit[1], p.light_unit[2]);    // :179
    const float cos_theta = fmaxf(dot3(N, L), 0.0f);                        // :188
    const uint32_t comp = COMP ? (uint32_t)__builtin_amdgcn_readfirstlane((int)p.comp) : 0u;
    const uint32_t show = COMP ? comp & (uint32_t)VCT_SHOW_ALL : (uint32_t)VCT_SHOW_ALL;
    const bool s_dd = !COMP || (show & VCT_SHOW_DIFFUSE), s_ao = !COMP || (show & VCT_SHOW_AMBIENT_OCCLUSION);
    const bool s_ird = !COMP || (show & VCT_SHOW_INDIRECT_DIFFUSE), s_ds = !COMP || (show & VCT_SHOW_SPECULAR);
    const bool s_irs = !COMP || (show & VCT_SHOW_INDIRECT_SPECULAR);
    const float raw_dd = shadow * cos_theta;
    const float direct_diffuse = s_dd ? raw_dd : 0.0f;                      // :192 (:190)
    const float occlusion = s_ao ? 1.0f - ind.w : 1.0f;                    // :201
    const float ird_r = s_ird ? ind.x : 0.0f, ird_g = s_ird ? ind.y : 0.0f, ird_b = s_ird ? ind.z : 0.0f;   // :203
    const float dr = (direct_diffuse + occlusion * ird_r) * alb_r;          // :205
    const float dg = (direct_diffuse + occlusion * ird_g) * alb_g;
    const float db = (direct_diffuse + occlusion * ird_b) * alb_b;
    const F3 R = normalize3(reflect3(f3(L.x * -1.0f, L.y * -1.0f, L.z * -1.0f), N));   // :212
    const float spec = powf(fmaxf(dot3(E, R), 0.0f), shininess);            // :213
    const float raw_ds = spec * shadow;
    const float direct_spec = s_ds ? raw_ds : 0.0f;                         // :214 (:215)
    const float spec_occ = s_ao ? 1.0f - sc.w : 1.0f;                       // :221
    const float irs_r = s_irs ? sc.x : 0.0f, irs_g = s_irs ? sc.y : 0.0f, irs_b = s_irs ? sc.z : 0.0f;
    const float sr = (irs_r + spec_occ * direct_spec) * gb_plane(gb, 19);   // :223
    const float sg = (irs_g + spec_occ * direct_spec) * gb_plane(gb, 20);
    const float sb = (irs_b + spec_occ * direct_spec) * gb_plane(gb, 21);
    const float ar = p.ambient * alb_r * occlusion;                         // :225
    const float ag = p.ambient * alb_g * occlusion;
    const float ab = p.ambient * alb_b * occlusion;
    float o0 = ar + dr + sr, o1 = ag + dg + sg, o2 = ab + db + sb, o3 = alb_a;   // :227
    if (COMP && (comp & VCT_COMP_EMISSION)) {
        const float* em = p.pix_emis + em_offset();
        o0 = o0 + em[0]; o1 = o1 + em[VCT_TILE_PIX]; o2 = o2 + em[2 * VCT_TILE_PIX];
    }
    if (!alive) {
        const float cc = clear_colour(p);
        o0 = cc; o1 = cc; o2 = cc; o3 = 1.0f;
    }
    uint2 pk;
    pk.x = pack_half2(o0, o1);
    pk.y = pack_half2(o2, o3);
    *reinterpret_cast<uint2*>(p.out + pixel() * 4) = pk;
    if (COMP) {     // raw per-component values, one 8-byte store per output; discarded pixels get zeros
        const uint32_t which = comp >> VCT_COMP_AOV_SHIFT;
        const size_t frame_halves = (size_t)p.width * p.height * 4;
        uint16_t* dst = p.aov + pixel() * 4;        // the outputs that are on, in bit order
        uint2 q;
        if (which & VCT_AOV_INDIRECT_DIFFUSE) {
            q.x = alive ? pack_half2(ind.x, ind.y) : 0u;
            q.y = alive ? pack_half2(ind.z, ind.w) : 0u;
            *reinterpret_cast<uint2*>(dst) = q;
            dst += frame_halves;
        }
        if (which & VCT_AOV_INDIRECT_SPECULAR) {
            q.x = alive ? pack_half2(sc.x, sc.y) : 0u;
            q.y = alive ? pack_half2(sc.z, sc.w) : 0u;
            *reinterpret_cast<uint2*>(dst) = q;
            dst += frame_halves;
        }
        if (which & VCT_AOV_DIRECT) {
            q.x = alive ? pack_half2(raw_dd, raw_ds) : 0u;
            q.y = alive ? pack_half2(shadow, 1.0f) : 0u;
            *reinterpret_cast<uint2*>(dst) = q;
        }
    }
}

// Workgroups are dealt to XCDs round-robin by the dispatcher (block b -> XCD b % 8); the tile order is
// remapped so that every XCD works on short runs of neighbouring tiles (neighbouring tiles march
// through neighbouring voxels and share that XCD's L2) while the runs of all XCDs interleave over
// the frame -- one long contiguous run per XCD loses more to imbalance between cheap and expensive
// screen regions than it gains in locality (profiles/r01h_ab_xcd_map.txt).  Run length measured: none
// (round-robin) 0.764 ms, one contiguous run per XCD 0.797, 16: 0.756, 60: 0.779, 240: 0.758.
__device__ __forceinline__ int xcd_remap(int b, int nblocks) {
    // runs of 16 consecutive blocks per XCD: a permutation inside every full group of
    // 8*run blocks; the last partial group keeps identity
    const int run = 16, group = 8 * run;
    const int g = b / group, local = b - g * group;
    return (g + 1) * group <= nblocks ? g * group + (local & 7) * run + (local >> 3) : b;
}

// tiles (waves) per workgroup: single-wave workgroups dispatch with the finest granularity, which
// balances the tail best (0.822 -> 0.800 ms against 4 waves; profiles/r01g_ab_waves_per_block.txt)
#ifndef VCT_WAVES_PER_BLOCK
#define VCT_WAVES_PER_BLOCK 1
#endif
// (VCT_TRACE_MIN_WAVES, the waves per SIMD the register allocator must leave room for: vct_trace_forms.h)

// One wave per tile, lane = pixel, the 7 cones in sequence; VCT_WAVES_PER_BLOCK horizontally
// adjacent tiles per workgroup, in the tile order of xcd_remap.
template <bool WRAP, int FASTDIV, bool COOP>
__global__ void __launch_bounds__(64 * VCT_WAVES_PER_BLOCK, VCT_TRACE_MIN_WAVES)
k_trace_tile(const VctTraceParams p) {
    constexpr VctMarchForm MARCH = march_form(COOP ? MF_COOP : MF_NONE);
    __shared__ float4 lds_blk[VCT_WAVES_PER_BLOCK][2][64];
    const int lane = threadIdx.x & 63;
    // wave-uniform by construction; readfirstlane tells the compiler, so tile indices, the tile's
    // G-buffer base and the LDS slab base live in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float4* blk = &lds_blk[wave][0][0];

    const int ntiles = (p.tile_row1 - p.tile_row0) * p.tiles_x;
    const int vb = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int ti = vb * VCT_WAVES_PER_BLOCK + wave;
    if (ti >= ntiles) return;

    const LaneBlock lb = make_lane_block(p, lane);
    MarchStats ms = {};

    const int tile = p.tile_row0 * p.tiles_x + ti;
    const int ty = tile_row_of(p, tile), tx = tile - ty * p.tiles_x;
    // Pixel / G-buffer addresses are re-derived from the lane id wherever they are needed (a few
    // integer ops) rather than carried in 64-bit VGPR pairs across the march loops, where they
    // would be spilled to scratch under the 80-VGPR budget.
    auto fresh_lane = [&]() { int l = lane; asm volatile("" : "+v"(l)); return l; };
    auto pixel_index = [&]() {
        const int l = fresh_lane();
        return (size_t)(ty * VCT_TILE + (l >> 3)) * p.width + (tx * VCT_TILE + (l & 7));
    };
    auto gbuf_ptr = [&](int l) {
        return p.gbuf + (size_t)tile * (VCT_GB_NPLANES * VCT_TILE_PIX) + l;
    };
    const int x = tx * VCT_TILE + (lane & 7), y = ty * VCT_TILE + (lane >> 3);
    // The G-buffer is read in three stages (cone frame, specular direction, composite) instead of
    // once up front: the 23 planes are only L1/L2 re-reads, while every VGPR kept live across the
    // march loops costs occupancy, and resident waves are what hides the sampler's latency chain.
    const float* gb = gbuf_ptr(lane);
    const bool in_frame = (x < p.width) && (y < p.height);
    const bool alive = in_frame && !(gb_plane(gb, 18) < 0.5f);      // trace.fs:171 discard

    F3 start, k0, k1, k2;
    cone_frame_from_gbuffer(gb, p.vs, start, k0, k1, k2);

    int total = 0;
    const F4 ind = gather_six_cones(k0, k1, k2, total,
        [&](F3 dir, int& st) { return cone_march<WRAP, FASTDIV, MARCH>(p, alive, start, dir, p.steps_diffuse, p.n_diffuse, blk, lb, st, ms); },
        [&](int i, F4 c, int st) { store_debug_cone(p, pixel_index, i, c, st, alive, in_frame); });

    // stage 2: the specular cone, from a fresh pointer: re-read instead of keeping planes live
    const float* gb2 = gbuf_ptr(fresh_lane());
    const F3 Rd = specular_dir(eye_dir(gb_planes3(gb2, 0), p.cam), gb_planes3(gb2, 12));
    int st6;
    const F4 sc = cone_march<WRAP, FASTDIV, MARCH>(p, alive, start, Rd, p.steps_specular, p.n_specular, blk, lb, st6, ms);
    total += st6;
    store_debug_cone(p, pixel_index, 6, sc, st6, alive, in_frame);

    // stage 3: composite (E again from planes 0-2: three L1 re-reads, against three registers live across the march)
    const float* gb3 = gbuf_ptr(fresh_lane());
    if (in_frame) composite<false>(p, gb3, ind, sc, eye_dir(gb_planes3(gb3, 0), p.cam), alive, pixel_index, [] { return (size_t)0; }, p.shininess);
    // executed-step count: wave reduction, stored into the tile's slot (a plain store: no atomic, nothing to clear)
    total = wave_sum(total);
    if (lane == 0) p.tile_steps[tile] = (uint32_t)total;
    flush_stats(p, ms, lane);
}

// ---- the same trace with each tile split over 3 waves ------------------------------------------
// A wave that marches all 71 steps of a tile lives ~140 us; at the end of a launch the GPU drains
// for about half of that with ever fewer waves resident (measured: +55..66 us per launch, 7 % of a
// 1080p frame but 37 % of the 0.15 ms slab an 8-GPU rank traces).  Here a tile is a workgroup of 3
// waves -- diffuse cones 0-2, diffuse cones 3-5, the specular cone (21 / 21 / 29 steps) -- that
// leave their cones in LDS and exit (the first wave the fold of its own, the prefix of the chain;
// "Cone hand-over" in the kernel); the last one to arrive continues the fold in the oracle's order
// (the weighted sum is an fma chain over cones 0..5) and composites.  Same bits, waves one third as
// long, no wave ever waits on another.
#ifndef VCT_SPLIT
#define VCT_SPLIT 3               // waves per tile: 3 = {cones 0-2, cones 3-5, specular}, 4 = {0-1, 2-3, 4-5, specular}, 7 = one cone each
#endif
// A/B at 256^3 / 1080p (round 3, ms): 3 waves 0.615; 4 waves 0.661 and 7 waves 0.808 although they balance the waves
// better and fill the CU's 28 wave slots exactly -- every wave pays the G-buffer fetch + frame inversion again and
// a shorter wave amortises that start-up stall over fewer march steps; 2 waves {0-3, 4-5 + specular} 0.639.
#define VCT_CONES_PER_WAVE (6 / (VCT_SPLIT - 1))
static_assert(VCT_SPLIT == 3 || VCT_SPLIT == 4 || VCT_SPLIT == 7, "VCT_SPLIT must be 3, 4 or 7");
// The forms of this kernel (ANISO, COMPACT, CELLS, PRIO, COMP, HALF, GLOSS, SKY, CHAIN), which of them exist, the waves per
// SIMD of each (split_min_waves: its launch bound) and what its marches derive from it (split_march_form: NARROW, REUSE):
// vct_trace_forms.h.
typedef const __attribute__((address_space(4))) VctGlossTable* GlossTable;
// the lane's class: its byte of the tile's plane under the clamp rule -- never an index before the clamp
__device__ __forceinline__ int gloss_class_of(const VctTraceParams& p, int tile, int pix, int nclasses) {
    const int b = (int)p.pix_gloss[(size_t)tile * VCT_TILE_PIX + pix];
    return b < nclasses ? b : 0;
}
template <bool WRAP, int FASTDIV, VctSplitForm FORM>
__global__ void __launch_bounds__(64 * VCT_SPLIT, split_min_waves(WRAP, FORM))
k_trace_tile_split(const VctTraceParams p) {
    static_assert(VctSplitFormChecked<WRAP, FORM>::value, "a form the kernel has no code for");
    constexpr bool ANISO = (FORM & SF_ANISO) != 0, COMPACT = (FORM & SF_COMPACT) != 0, PRIO = (FORM & SF_PRIO) != 0;
    constexpr bool COMP = (FORM & SF_COMP) != 0, HALF = (FORM & SF_HALF) != 0, GLOSS = (FORM & SF_GLOSS) != 0, SKY = (FORM & SF_SKY) != 0;
    constexpr VctMarchForm MARCH = split_march_form(WRAP, FORM);       // of every march of this kernel
    __shared__ float4 lds_blk[VCT_SPLIT][ANISO ? 4 : 2][64];   // per wave: level-1 slab, level-2 slab (+ their "-axis" slabs)
    // Cone hand-over.  The workgroup's LDS stays allocated until its last wave ends while the waves that ended free their
    // slots and registers, so what a tile declares caps how many tiles fill a CU's wave slots: the cones travel in the
    // slabs, which a wave's marches have finished with, and only a diffuse wave's earlier cones need room of their own.
    //   first diffuse wave   folds its own cones from +0 -- the prefix of the oracle's chain over cones 0..5, operation
    //                        for operation -- and leaves that one float4 in its first slab; between its marches the
    //                        running fold waits in lds_pre (x, y, z) and in the one register a diffuse wave carries
    //                        across its marches (w; the wave's step count, which has that register in the other waves,
    //                        waits in lds_steps): registers held across the marches put the kernel into scratch, and a
    //                        fourth plane of floats puts the tile over 9 KiB
    //   other diffuse waves  cannot fold without the prefix: raw cones, all but the last in lds_raw, the last in the
    //                        first slab
    //   specular wave        its cone in its second slab, E in its first; with GLOSS it marches once per class, and a
    //                        lane's cone waits in lds_gloss from its own march on (four registers held across the class
    //                        loop cost the HALF forms their eighth wave and put the clamp-mode ones into scratch): the
    //                        last arriver reads it there
    // Every slab is written behind the wave's last march: between two marches nothing writes one (`held` describes the
    // second slab, and the first is refilled by every sample that reads it).
    constexpr int RAW_WAVES = VCT_SPLIT - 2, RAW_CONES = VCT_CONES_PER_WAVE - 1;
    __shared__ float4 lds_raw[RAW_WAVES * RAW_CONES > 0 ? RAW_WAVES * RAW_CONES : 1][64];
    __shared__ float lds_pre[3][64];
    __shared__ uint16_t lds_steps[64];
    __shared__ float4 lds_gloss[GLOSS ? 64 : 1];       // (referenced by the GLOSS forms only: the others declare none of it)
    static_assert(VCT_CONES_PER_WAVE * VCT_MAX_STEPS < (1 << 16), "a lane's steps over the cones of a wave fit lds_steps");
    // Arrival word: bits 28-31 count the waves that have arrived, bits 0-27 sum their executed steps -- one returning
    // atomic per wave raises both, and the last arriver stores the total.  A tile executes at most 64 lanes x (6 diffuse
    // cones + 8 gloss classes) x VCT_MAX_STEPS steps, and VCT_SPLIT arrivals fit four bits:
    static_assert(64ull * (6 + 8) * VCT_MAX_STEPS < (1ull << 28) && VCT_SPLIT < 16, "the arrival word holds count and step total");
    __shared__ uint32_t lds_arrive;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float4* blk = &lds_blk[wave][0][0];
    if (threadIdx.x == 0) lds_arrive = 0u;
    __syncthreads();

    const int ntiles = p.ntiles;          // (host-computed: a division here is ~40 instructions per wave -- 1 % of the frame)
    const int ti = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    if (ti >= ntiles) return;
    // Live-pixel compaction (experiment, trace_variant 4): the wave's 64 pixels come from the compaction list -- the live
    // pixels of a 16x16 super-tile -- instead of being the launched tile's.  `cpix` = tile << 6 | pixel of the tile.
    constexpr bool compact = COMPACT;         // (a separate instantiation: the default kernel carries none of this)
    uint32_t cpix = 0u;
    if (compact) {
        if ((uint32_t)ti >= *p.vt_count) {
            if (threadIdx.x == 0) p.tile_steps[p.tile_row0 * p.tiles_x + ti] = 0u;
            return;
        }
        cpix = p.vt_pix[(size_t)ti * 64 + lane];
    }

    const LaneBlock lb = make_lane_block(p, lane);
    MarchStats ms = {};
    // block reuse (BlockDesc), in the forms split_reuse names; the others never read the descriptor
    BlockDesc held = no_block();

    // (interleaved slabs: traced row j of the launch is tile row row0 + j * stride; the plain launch pays no second division)
    int lrow = 0, tile0 = p.tile_row0 * p.tiles_x + ti;           // tile0: where the wave's step count is stored
    if (p.row_stride > 1) {
        lrow = tile_row_of(p, ti);
        tile0 = (p.tile_row0 + lrow * p.row_stride) * p.tiles_x + (ti - lrow * p.tiles_x);
    }
    const bool cvalid = !compact || cpix != 0xffffffffu;
    const int tile = compact ? (cvalid ? (int)(cpix >> 6) : 0) : tile0;
    const int ty = tile_row_of(p, tile), tx = tile - ty * p.tiles_x;
    // tile row of the output (a packed slab holds its rows back to back)
    const int oy = p.pack_rows ? (p.row_stride > 1 ? lrow : ty - p.tile_row0) : ty;
    const int plane_ = compact ? (int)(cpix & 63u) : lane;        // this lane's pixel inside its tile
    auto fresh_lane = [&]() { int l = plane_; asm volatile("" : "+v"(l)); return l; };
    auto pixel_index = [&]() {
        const int l = fresh_lane();
        return (size_t)(oy * VCT_TILE + (l >> 3)) * p.width + (tx * VCT_TILE + (l & 7));
    };
    auto gbuf_ptr = [&](int l) {
        return p.gbuf + (size_t)tile * (VCT_GB_NPLANES * VCT_TILE_PIX) + l;
    };
    const int x = tx * VCT_TILE + (plane_ & 7), y = ty * VCT_TILE + (plane_ >> 3);
    const float* gb = gbuf_ptr(plane_);
    const bool in_frame = cvalid && (x < p.width) && (y < p.height);
    const bool alive = in_frame && !(gb_plane(gb, 18) < 0.5f);      // trace.fs:171 discard
    int total = 0;
    // COMP: a cone group nothing reads (march_groups bit 0: cones 0-5, bit 1: cone 6) is marched over 0 steps -- zero
    // cones into LDS and the debug outputs, 0 steps, and the wave arrives at once.  The count is wave-uniform (the
    // parameter word through readfirstlane), so the march loop is not entered on a scalar branch.
    const uint32_t groups = COMP ? (uint32_t)__builtin_amdgcn_readfirstlane((int)p.comp) >> VCT_COMP_GROUPS_SHIFT : 3u;
    const int n_diffuse = (groups & 1u) ? p.n_diffuse : 0, n_specular = (groups & 2u) ? p.n_specular : 0;
    // SKY: a table of 0 steps is a cone that is all sky, so a group nothing reads must not look like one: its lanes go
    // into the march as not alive (the zero cone, 0 steps -- what the 0-step march gives without a sky)
    const bool march_d = SKY ? alive && (groups & 1u) != 0u : alive, march_s = SKY ? alive && (groups & 2u) != 0u : alive;
    if (HALF && wave < VCT_SPLIT - 1) {
        // 0 steps: the wave arrives at once (the skip mechanism of COMP, without its zero cones)
    } else if (wave < VCT_SPLIT - 1) {
        F3 start, k0, k1, k2;
        cone_frame_from_gbuffer(gb, p.vs, start, k0, k1, k2);
        // (a wave that marches nothing folds or hands over zero cones: a zero prefix stays +0 through the fmas)
        // `carried` is the one register a diffuse wave holds across its marches.  In the first wave it is the BITS of the
        // prefix's w until the last cone is folded (the lane's step count waits in lds_steps), in the other waves the
        // lane's step count; behind the loop it is the lane's step count in every wave, and only then goes into `total`.
        int carried = 0;
        const int first = wave * VCT_CONES_PER_WAVE;
        // (LDS addresses from a fresh copy of the lane id: hoisted out of the loop they live across the marches)
        auto own_lane = [&]() { int l = lane; asm volatile("" : "+v"(l)); return l; };
#pragma unroll 1
        for (int i = first; i < first + VCT_CONES_PER_WAVE; ++i) {      // :196-199
            int st;
            const F4 c = cone_march<WRAP, FASTDIV, MARCH, SKY ? VCT_SKY_INSIDE : VCT_SKY_NONE>(p, march_d, start, cone_dir(k0, k1, k2, i),
                                                                       p.steps_diffuse, n_diffuse, blk, lb, st, ms, held);
            const bool last = i - first == RAW_CONES;      // behind the wave's last march: into its first slab
            const int l = own_lane();
            F4 out = c;
            if (wave == 0) {
                F4 pre = {0.0f, 0.0f, 0.0f, 0.0f};
                int sum = st;
                if (i != 0) {
                    pre = {lds_pre[0][l], lds_pre[1][l], lds_pre[2][l], __int_as_float(carried)};
                    sum += (int)lds_steps[l];
                }
                out = fold_cone(pre, i, c);
                if (!last) {
                    lds_pre[0][l] = out.x; lds_pre[1][l] = out.y; lds_pre[2][l] = out.z; carried = __float_as_int(out.w);
                    lds_steps[l] = (uint16_t)sum;
                } else carried = sum;
            } else {
                carried += st;
                if (!last) lds_raw[(wave - 1) * RAW_CONES + (i - first)][l] = make_float4(c.x, c.y, c.z, c.w);
            }
            if (last) blk[l] = make_float4(out.x, out.y, out.z, out.w);
            store_debug_cone(p, pixel_index, i, c, st, alive, in_frame);
        }
        total = carried;
    } else {
        // the specular wave is the longest of a tile (29 march steps against 21) and the last ones of a launch are its
        // tail: raised issue priority lets them run ahead of the diffuse waves, which have the slack.  Pays when the
        // launch is a slab of a multi-GPU frame (8-way slabs of the 1080p frame: 0.1085 -> 0.1052 ms mean, 0.115 ->
        // 0.111 ms max), costs 0.5 % on the whole frame: the host sets it for launches of at most half the frame.
        // (the PRIO instantiation -- whole frames -- sets and resets the priority around every sample's loads instead)
        if (!PRIO && p.spec_prio) __builtin_amdgcn_s_setprio(1);
        const F3 P = gb_planes3(gb, 0), Nw = gb_planes3(gb, 3), N = gb_planes3(gb, 12);
        const F3 start = cone_start(P, Nw, p.vs);
        // E is the composite's too: this wave hands it over in its own first slab and its cone in its second -- no LDS of
        // their own -- once its marches are over and nothing reads its slabs again, in every form of this arm, also the
        // 0-step ones of COMP and HALF (GLOSS: the cone is in lds_gloss already)
        const F3 E = eye_dir(P, p.cam);
        auto hand_over_e = [&](F3 e) { blk[lane] = make_float4(e.x, e.y, e.z, 0.0f); };
        auto hand_over = [&](F4 cone, F3 e) {
            blk[64 + lane] = make_float4(cone.x, cone.y, cone.z, cone.w);
            hand_over_e(e);
        };
        if constexpr (GLOSS) {
            // One march per class present among the live lanes: the class of the first remaining lane, wave-uniform, picks
            // the table and its step count by scalar loads; the lanes of that class march, write their cone and leave the
            // mask.  A lane marches exactly once, so nothing depends on the order of the classes.  `held` stays live across
            // the marches: it describes a block by (level, anchor) alone, every sample tests its own footprints against it,
            // and between two marches nothing writes the wave's slabs (the first slab is refilled by every sample that
            // reads it, the second only together with the descriptor) -- so the lane's cone waits in lds_gloss.
            const GlossTable gt = (GlossTable)p.gloss;
            const int cls = gloss_class_of(p, tile, plane_, gt->nclasses);
            const F3 dir = specular_dir(E, N);
            if (!alive) {     // what a lane that marches nothing gets from the one march of the other forms
                lds_gloss[lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p.dbg_steps && in_frame) p.dbg_steps[pixel_index() * 7 + 6] = 0;
            }
            [[maybe_unused]] float sky_alpha = 0.0f;       // SKY: what the lane's own march saw last
            for (unsigned long long rest = ballot64(alive); rest != 0ull;) {
                const int k = __builtin_amdgcn_readlane(cls, (int)__ffsll((long long)rest) - 1);
                const bool mine = alive && cls == k;
                int st;
                float a = 0.0f;
                const F4 sc = cone_march<WRAP, FASTDIV, MARCH, SKY ? VCT_SKY_ALPHA : VCT_SKY_NONE>(
                    p, mine && march_s, start, dir, &p.gloss->steps[k][0], (groups & 2u) ? gt->nsteps[k] : 0, blk, lb, st, ms, held, &a);
                total += st;          // (0 for the lanes that did not march)
                if (mine) lds_gloss[lane] = make_float4(sc.x, sc.y, sc.z, sc.w);
                if (SKY && mine) sky_alpha = a;
                store_debug_cone(p, pixel_index, 6, sc, st, mine && !SKY, mine);      // (SKY: the cone is stored below)
                rest &= ~ballot64(mine);
            }
            if constexpr (SKY) {
                // the sky once per lane, behind the class loop, from the alpha its own march handed out: inside the march
                // (as in every other form) the epilogue costs the clamp-mode GLOSS kernels 4 VGPRs -- the 8th wave of the
                // HALF form -- and the PRIO one 8 B of scratch.  Same chain, same operands, same bits.
                const float4 v = lds_gloss[lane];
                F4 sc = {v.x, v.y, v.z, v.w};
                sky_epilogue(p, march_s, dir, sky_alpha, sc.x, sc.y, sc.z);
                lds_gloss[lane] = make_float4(sc.x, sc.y, sc.z, sc.w);
                store_debug_cone(p, pixel_index, 6, sc, 0, alive, false);
            }
            // (E again from planes 0-2, L1 re-reads: live across the class loop it costs the clamp-mode GLOSS kernels 3 VGPRs
            // -- the 8th wave of the HALF forms, 16 B of scratch in the PRIO ones)
            hand_over_e(eye_dir(gb_planes3(gbuf_ptr(fresh_lane()), 0), p.cam));
        } else {
        int st6;
        const F4 sc = cone_march<WRAP, FASTDIV, MARCH, SKY ? VCT_SKY_INSIDE : VCT_SKY_NONE>(p, march_s, start, specular_dir(E, N),
                                                                    p.steps_specular, n_specular, blk, lb, st6, ms, held);
        total += st6;
        store_debug_cone(p, pixel_index, 6, sc, st6, alive, in_frame);
        hand_over(sc, E);
        }
    }
    total = wave_sum(total);
    flush_stats(p, ms, lane, wave == VCT_SPLIT - 1);

    // arrival: LDS operations of a wave are performed in order, so what the wave hands over is in LDS before the
    // word is raised; whoever raises its count to VCT_SPLIT sees all of it
    __threadfence_block();
    uint32_t before = 0u;
    if (lane == 0) before = atomicAdd(&lds_arrive, (uint32_t)total + (1u << 28));
    before = (uint32_t)__builtin_amdgcn_readfirstlane((int)before);
    if ((before >> 28) != VCT_SPLIT - 1) return;
    __threadfence_block();
    // one plain store per tile: no global atomic, nothing to clear
    if (lane == 0) p.tile_steps[tile0] = (before + (uint32_t)total) & 0x0fffffffu;

    // the last wave continues the first wave's prefix over the other diffuse cones in the oracle's order and composites
    const float* gb3 = gbuf_ptr(fresh_lane());
    if (in_frame) {
        F4 ind = {0.0f, 0.0f, 0.0f, 0.0f};
        if (HALF) {
            const float4 v = p.dr_ind[pixel_index()];
            ind = {v.x, v.y, v.z, v.w};
        } else {
            const float4 pre = lds_blk[0][0][lane];
            ind = {pre.x, pre.y, pre.z, pre.w};
#pragma unroll
            for (int i = VCT_CONES_PER_WAVE; i < 6; ++i) {
                const int w = i / VCT_CONES_PER_WAVE, j = i % VCT_CONES_PER_WAVE;
                ind = fold_cone(ind, i, j < RAW_CONES ? lds_raw[(w - 1) * RAW_CONES + j][lane] : lds_blk[w][0][lane]);
            }
        }
        float shininess = p.shininess;
        if constexpr (GLOSS) {
            const GlossTable gt = (GlossTable)p.gloss;
            shininess = p.gloss->shininess[gloss_class_of(p, tile, fresh_lane(), gt->nclasses)];
        }
        const float4 e = lds_blk[VCT_SPLIT - 1][0][lane];
        float4 sc;
        if constexpr (GLOSS) sc = lds_gloss[lane]; else sc = lds_blk[VCT_SPLIT - 1][1][lane];
        composite<COMP>(p, gb3, ind, sc, f3(e.x, e.y, e.z), alive, pixel_index,
                        [&]() { return (size_t)tile * (VCT_EMIS_NPLANES * VCT_TILE_PIX) + fresh_lane(); }, shininess);
    }
}

// ---- Half-rate diffuse gather (include/vct.h vct_set_diffuse_rate) ------------------------------------------------------
// The six diffuse cones are 63 % of a frame's steps and their gather varies slowly over a surface: at rate 2 one pixel
// per 2x2 quad -- its ANCHOR -- marches them, the other pixels take the 9:3:3:1 mean of the (up to) four nearest
// anchors' gathers that lie on their surface, and a pixel none of them serves marches its own (a FILL pixel).  Four
// launches on the slot's stream:
//   k_point_march<.., LISTED = false>   lane = one quad of an 8x8 block of quads: finds the anchor, marches its cones
//   k_diffuse_resolve                   lane = one pixel: acceptance test, interpolation, fill list (one append per wave)
//   k_point_march<.., LISTED = true>    lane = one entry of the fill list, over the list's device-side count
//   k_trace_tile_split<.., SF_HALF ..>  specular cone + composite with the gather of p.dr_ind
// The marches are cone_march with rate 1's inputs, so cones and gather of a marched pixel are rate 1's, bit for bit.
__device__ __forceinline__ const float* gb_of_pixel(const VctTraceParams& p, int x, int y) {
    return p.gbuf + (size_t)((y >> 3) * p.tiles_x + (x >> 3)) * (VCT_GB_NPLANES * VCT_TILE_PIX) + (((y & 7) << 3) | (x & 7));
}
// (a.x*b.x + a.y*b.y) + a.z*b.z, every operation rounded on its own (include/vct.h: no fused operation)
__device__ __forceinline__ float dot3_rn(F3 a, F3 b) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fmul_rn(a.z, b.z));
}
// this lane's place among the lanes of mask m below it
__device__ __forceinline__ uint32_t lane_rank(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

#ifndef VCT_POINT_MIN_WAVES
#define VCT_POINT_MIN_WAVES 5     // the cone frame and the running gather stay live across the marches: as the bounce (6 spills 12-22 registers)
#endif
// WAVES = 1: one wave marches the six cones of its 64 points (the shape of k_bounce_march); 2: a workgroup of two waves
// with cones 0-2 and 3-5, the second hands its three over in LDS and the first folds all six in the oracle's order.
template <bool WRAP, int FASTDIV, bool LISTED, int WAVES, bool SKY = false>
__global__ void __launch_bounds__(64 * WAVES, VCT_POINT_MIN_WAVES)
k_point_march(const VctTraceParams p) {
    __shared__ float4 lds_blk[WAVES][2][64];
    __shared__ float4 lds_cone[WAVES == 2 ? 3 : 1][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float4* blk = &lds_blk[wave][0][0];
    const LaneBlock lb = make_lane_block(p, lane);
    MarchStats ms = {};
    const int cw = (p.width + 1) >> 1, ch = (p.height + 1) >> 1;
    const int bxn = (cw + 7) >> 3;
    const uint32_t nfill = LISTED ? (uint32_t)p.dr_ctr[2 * VCT_DR_COUNTERS] : 0u;
    const uint32_t nitems = LISTED ? (nfill + 63u) >> 6 : (uint32_t)(bxn * ((ch + 7) >> 3));       // workgroup-uniform
    unsigned long long wave_steps = 0;
    uint32_t wave_marched = 0u;
    for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
        // the point of this lane: pixel (x, y); a lane without one reads pixel 0 and its result is discarded
        int x = 0, y = 0;
        bool alive = false;
        uint32_t code = VCT_DR_NO_ANCHOR;
        const int by = LISTED ? 0 : (int)it / bxn, bx = LISTED ? 0 : (int)it - by * bxn;
        const int cx = bx * 8 + (lane & 7), cy = by * 8 + (lane >> 3);          // (coarse march: this lane's quad)
        if (!LISTED) {
            if (cx < cw && cy < ch) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {          // (0,0), (1,0), (0,1), (1,1): the first pixel that is not discarded
                    const int px = 2 * cx + (k & 1), py = 2 * cy + (k >> 1);
                    if (!alive && px < p.width && py < p.height && !(gb_plane(gb_of_pixel(p, px, py), 18) < 0.5f)) {
                        alive = true; x = px; y = py; code = (uint32_t)k;
                    }
                }
            }
        } else {
            const uint32_t e = it * 64u + (uint32_t)lane;
            if (e < nfill) {
                const uint32_t pix = p.dr_list[e];
                y = (int)(pix / (uint32_t)p.width); x = (int)(pix - (uint32_t)y * (uint32_t)p.width);
                alive = true;
            }
        }
        const float* gb = gb_of_pixel(p, x, y);
        auto pixel_index = [&]() { return (size_t)y * p.width + x; };
        F3 start, k0, k1, k2;
        cone_frame_from_gbuffer(gb, p.vs, start, k0, k1, k2);
        F4 ind = {0.0f, 0.0f, 0.0f, 0.0f};
        int total = 0;
        const int first = WAVES == 2 ? wave * 3 : 0;
#pragma unroll 1
        for (int i = first; i < first + 6 / WAVES; ++i) {
            int st;
            const F4 c = cone_march<WRAP, FASTDIV, march_form(MF_COOP), SKY ? VCT_SKY_INSIDE : VCT_SKY_NONE>(p, alive, start, cone_dir(k0, k1, k2, i), p.steps_diffuse,
                                                                                   p.n_diffuse, blk, lb, st, ms);
            total += st;
            bool handed = false;
            if constexpr (WAVES == 2) {
                if (wave == 1) { lds_cone[i - 3][lane] = make_float4(c.x, c.y, c.z, c.w); handed = true; }
            }
            if (!handed) ind = fold_cone(ind, i, c);
            store_debug_cone(p, pixel_index, i, c, st, alive, alive);
        }
        if constexpr (WAVES == 2) {
            __syncthreads();
            if (wave == 0)
                for (int i = 3; i < 6; ++i) ind = fold_cone(ind, i, lds_cone[i - 3][lane]);
        }
        if (wave == 0) {
            const float4 v = make_float4(ind.x, ind.y, ind.z, ind.w);
            if (LISTED) {
                if (alive) p.dr_ind[pixel_index()] = v;
            } else if (cx < cw && cy < ch) {
                p.dr_coarse[(size_t)cy * cw + cx] = v;          // (no anchor: no sample -- zeros nobody reads)
                p.dr_anchor[(size_t)cy * cw + cx] = (uint8_t)code;
            }
            wave_marched += (uint32_t)__popcll(ballot64(alive));
        }
        if (WAVES == 2) __syncthreads();          // lds_cone is written again by the next round
        // (spelt out, not wave_sum: through the helper the 16 instantiations hoist the lane arithmetic in another order)
        for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
        wave_steps += (unsigned long long)total;
    }
    if (lane == 0) {
        const uint32_t slot = (blockIdx.x * WAVES + wave) & (VCT_DR_COUNTERS - 1);
        if (wave_steps) atomicAdd(p.dr_ctr + slot, wave_steps);
        if (wave_marched) atomicAdd(p.dr_ctr + VCT_DR_COUNTERS + slot, (unsigned long long)wave_marched);
    }
    flush_stats(p, ms, lane);
}

// ---- Point queries (include/vct.h "point queries": vct_gather_points, vct_cone_points) ---------------------------------------
// The march of the screen trace for points the caller names: light probes, lightmap texels, particles.  One wave per 64
// consecutive entries of the (possibly permuted: q.index) list, lane = point, a fixed grid striding over the items as
// k_point_march<LISTED> does.  KIND = VCT_QUERY_GATHER: cone_frame on the point's own T, B, N, P, six diffuse cones, the
// fold of fold_cone in cone order -- the arithmetic of a pixel of k_trace_tile*, so the same bits.  VCT_QUERY_CONE: one
// cone along the caller's direction from cone_start(P, N), with the diffuse or the specular step table.  DEBUG: the raw
// cones and / or per-cone step counts are wanted too.
// The cooperative block serves waves whose points are neighbours in space (a lightmap in row order, a sorted list), the
// per-lane gather the others: sample_level's own decision, per sample.  A record is 48 (36) bytes at 4-byte alignment and
// arrives as dwordx4 loads (VctTri9's reason); results leave as one dwordx4 store per vec4.  Address safety: a point is
// addressed by an entry index < n (or the library's own permutation of those); coordinates reach memory only through
// sample_level's masked / clamped texel indices.  Tail lanes (n not a multiple of 64) re-read the last point, march as
// `alive = false` and store nothing.
struct __attribute__((packed, aligned(4))) VctFloats12 { float v[12]; };
struct __attribute__((packed, aligned(4))) VctFloats4 { float v[4]; };
__device__ __forceinline__ void store_vec4(float* dst, F4 c) {
    VctFloats4 o;
    o.v[0] = c.x; o.v[1] = c.y; o.v[2] = c.z; o.v[3] = c.w;
    *(VctFloats4*)dst = o;
}
template <bool WRAP, int FASTDIV, int KIND, bool DEBUG, bool SKY = false>
__global__ void __launch_bounds__(64, VCT_POINT_MIN_WAVES)
k_query_march(const VctTraceParams p, const VctQueryArgs q) {
    __shared__ float4 lds_blk[2][64];
    const int lane = (int)threadIdx.x;
    float4* blk = &lds_blk[0][0];
    const LaneBlock lb = make_lane_block(p, lane);
    MarchStats ms = {};
    const uint32_t nitems = (q.n + 63u) >> 6;          // (the host launches nothing for n = 0)
    unsigned long long wave_steps = 0;
    for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
        const uint32_t e = it * 64u + (uint32_t)lane;
        const bool alive = e < q.n;
        const uint32_t entry = alive ? e : q.n - 1u;
        const size_t i = q.index ? q.index[entry] : entry;          // the caller's index of this lane's point
        int total = 0;
        if constexpr (KIND == VCT_QUERY_GATHER) {
            const VctFloats12 r = *(const VctFloats12*)(q.pts + i * 12);
            F3 start, k0, k1, k2;
            cone_frame(f3(r.v[0], r.v[1], r.v[2]), f3(r.v[3], r.v[4], r.v[5]), f3(r.v[6], r.v[7], r.v[8]),
                       f3(r.v[9], r.v[10], r.v[11]), p.vs, start, k0, k1, k2);
            // (spelt out, not gather_six_cones: through the helper the sorted ambient-cube gather measured 0.8 % slower
            // than the loop, outside the loop's own spread -- profiles/experiments/r13_trace_one_copy_ab.txt)
            F4 ind = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
            for (int c = 0; c < 6; ++c) {
                int st;
                const F4 v = cone_march<WRAP, FASTDIV, march_form(MF_COOP), SKY ? VCT_SKY_INSIDE : VCT_SKY_NONE>(p, alive, start, cone_dir(k0, k1, k2, c), p.steps_diffuse,
                                                                                       p.n_diffuse, blk, lb, st, ms);
                total += st;
                ind = fold_cone(ind, c, v);
                if (DEBUG && alive) {
                    if (q.out_cones) store_vec4(q.out_cones + (i * 6 + (size_t)c) * 4, v);
                    if (q.out_steps) q.out_steps[i * 6 + (size_t)c] = (uint8_t)st;
                }
            }
            if (alive) store_vec4(q.out + i * 4, ind);
        } else {
            const VctTri9 r = *(const VctTri9*)(q.pts + i * 9);
            const F3 start = cone_start(f3(r.v[0], r.v[1], r.v[2]), f3(r.v[3], r.v[4], r.v[5]), p.vs);
            const VctStep* tab = q.specular ? p.steps_specular : p.steps_diffuse;          // (wave-uniform)
            const int nsteps = q.specular ? p.n_specular : p.n_diffuse;
            const F4 v = cone_march<WRAP, FASTDIV, march_form(MF_COOP), SKY ? VCT_SKY_INSIDE : VCT_SKY_NONE>(p, alive, start, f3(r.v[6], r.v[7], r.v[8]), tab, nsteps, blk, lb,
                                                                                   total, ms);
            if (alive) {
                store_vec4(q.out + i * 4, v);
                if (DEBUG) q.out_steps[i] = (uint8_t)total;
            }
        }
        wave_steps += (unsigned long long)wave_sum(total);
    }
    if (lane == 0 && wave_steps) atomicAdd(q.ctr + (blockIdx.x & (VCT_DR_COUNTERS - 1)), wave_steps);
    flush_stats(p, ms, lane);
}

// Sort key of VCT_QUERY_SORT_CELLS: the Morton code of the 4-voxel cell of the point's start position, folded into the grid
// as the sampler folds a coordinate (REPEAT: modulo, else clamped), over the octant of the direction the march leaves in
// (gather: the normal; cone: the direction).  Non-finite points sort last.  The key orders the march and nothing else:
// results do not depend on it.
template <bool WRAP, int KIND>
__global__ void __launch_bounds__(256)
k_query_keys(const VctTraceParams p, const VctQueryArgs q, uint32_t* keys, uint32_t* index) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= q.n) return;
    const float* r = q.pts + (size_t)i * (KIND == VCT_QUERY_GATHER ? 12 : 9);
    const F3 start = cone_start(f3(r[0], r[1], r[2]), f3(r[3], r[4], r[5]), p.vs);
    const F3 d = KIND == VCT_QUERY_GATHER ? f3(r[3], r[4], r[5]) : f3(r[6], r[7], r[8]);
    const int cells = p.V >> 2;          // per axis (V >= 8: at least 2)
    auto cell = [&](float x) {
        const float u = fmaf(x / p.half_G, 0.5f, 0.5f) * (float)cells;
        const int c = (int)fminf(fmaxf(floorf(u), -0x1p30f), 0x1p30f);
        return (uint32_t)(WRAP ? c & (cells - 1) : min(max(c, 0), cells - 1));
    };
    uint32_t key = 1u << (VCT_QUERY_KEY_BITS - 1);
    const float probe = (start.x + start.y + start.z) * 0.0f + (d.x + d.y + d.z) * 0.0f;      // NaN iff something is not finite
    if (probe == probe) {
        const uint32_t oct = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
        key = (vct_morton3(cell(start.x), cell(start.y), cell(start.z)) << 3) | oct;
    }
    keys[i] = key;
    index[i] = i;
}

// One wave per 8x8 tile, lane = pixel.  An anchor copies its quad's sample; any other live pixel tests the four
// candidates of include/vct.h in their order and interpolates, or -- no candidate accepted -- joins the fill list.
__global__ void __launch_bounds__(256)
k_diffuse_resolve(const VctTraceParams p) {
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (tile >= p.tiles_x * p.tiles_y) return;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int x = tx * VCT_TILE + (lane & 7), y = ty * VCT_TILE + (lane >> 3);
    const float* gb = p.gbuf + (size_t)tile * (VCT_GB_NPLANES * VCT_TILE_PIX) + lane;
    const bool in_frame = x < p.width && y < p.height;
    const bool alive = in_frame && !(gb_plane(gb, 18) < 0.5f);
    const int cw = (p.width + 1) >> 1, ch = (p.height + 1) >> 1;
    const size_t pix = (size_t)y * p.width + x;
    bool marched = false, fill = false;
    if (alive) {
        const int qx = x >> 1, qy = y >> 1;
        if ((uint32_t)p.dr_anchor[(size_t)qy * cw + qx] == (uint32_t)(((y & 1) << 1) | (x & 1))) {
            marched = true;
            p.dr_ind[pix] = p.dr_coarse[(size_t)qy * cw + qx];
        } else {
            const F3 Pp = gb_planes3(gb, 0), np_ = gb_planes3(gb, 3);
            const float lp = dot3_rn(np_, np_);
            const float plane_tol = __fmul_rn(__fmul_rn(VCT_DIFFUSE_RATE_PLANE_TOL, __fmul_rn(p.vs, p.vs)), lp);
            const int sx = (x & 1) ? 1 : -1, sy = (y & 1) ? 1 : -1;
            float4 S = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            int W = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {          // own quad 9, horizontal neighbour 3, vertical neighbour 3, diagonal 1
                const int ccx = qx + ((k & 1) ? sx : 0), ccy = qy + ((k & 2) ? sy : 0);
                const float wgt = k == 0 ? 9.0f : (k == 3 ? 1.0f : 3.0f);
                float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);          // a rejected candidate contributes +0
                if (ccx >= 0 && ccx < cw && ccy >= 0 && ccy < ch) {
                    const uint32_t code = p.dr_anchor[(size_t)ccy * cw + ccx];
                    if (code != VCT_DR_NO_ANCHOR) {
                        const float* ga = gb_of_pixel(p, 2 * ccx + (int)(code & 1u), 2 * ccy + (int)(code >> 1));
                        const F3 Pk = gb_planes3(ga, 0), nk = gb_planes3(ga, 3);
                        const float dn = dot3_rn(np_, nk), lk = dot3_rn(nk, nk);
                        const float d = dot3_rn(f3(__fsub_rn(Pk.x, Pp.x), __fsub_rn(Pk.y, Pp.y), __fsub_rn(Pk.z, Pp.z)), np_);
                        if (dn > 0.0f && __fmul_rn(dn, dn) >= __fmul_rn(VCT_DIFFUSE_RATE_NORMAL_COS2, __fmul_rn(lp, lk)) &&
                            __fmul_rn(d, d) <= plane_tol) {
                            const float4 I = p.dr_coarse[(size_t)ccy * cw + ccx];
                            W += k == 0 ? 9 : (k == 3 ? 1 : 3);
                            t = make_float4(__fmul_rn(wgt, I.x), __fmul_rn(wgt, I.y), __fmul_rn(wgt, I.z), __fmul_rn(wgt, I.w));
                        }
                    }
                }
                if (k == 0) S = t;
                else S = make_float4(__fadd_rn(S.x, t.x), __fadd_rn(S.y, t.y), __fadd_rn(S.z, t.z), __fadd_rn(S.w, t.w));
            }
            if (W > 0) {
                const float fW = (float)W;
                p.dr_ind[pix] = make_float4(div_rn(S.x, fW), div_rn(S.y, fW), div_rn(S.z, fW), div_rn(S.w, fW));
            } else {
                marched = fill = true;
            }
        }
    }
    // debug outputs: a pixel that marches nothing of its own shows 0 steps and zero cones 0..5
    if (in_frame && !marched) {
        if (p.dbg_steps)
            for (int i = 0; i < 6; ++i) p.dbg_steps[pix * 7 + i] = 0;
        if (p.dbg_cones && alive)
            for (int i = 0; i < 24; ++i) p.dbg_cones[pix * 28 + i] = 0.0f;
    }
    // the fill list: one reservation per wave
    const unsigned long long m = ballot64(fill);
    if (m != 0ull) {
        uint32_t base = 0u;
        if (lane == 0) base = (uint32_t)atomicAdd(p.dr_ctr + 2 * VCT_DR_COUNTERS, (unsigned long long)__popcll(m));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (fill) p.dr_list[base + lane_rank(m)] = (uint32_t)pix;
    }
}

// Second bounce (oracle/vct_oracle.h vcto_bounce), three kernels:
//   k_bounce_list   one wave per touched 8^3 brick (found through the voxelizer's slot table): copies the brick
//                   into the bounce chain (untouched voxels keep their bounce-0 value), compacts its occupied
//                   voxels (ballot + popcount through LDS) and appends them to a global voxel list, one
//                   reservation per workgroup of 16 bricks -- bricks stay contiguous in the list and follow
//                   each other in Morton order, so neighbouring entries are Morton-adjacent voxels;
//   k_bounce_march  one wave per 64 list entries, lane = voxel, the 6 diffuse cones marched with the
//                   same cone_march as the screen trace (voxels of a locally flat surface trace
//                   near-parallel cones, so the cooperative sampler applies);
//   k_bounce_bricks the same march per brick, only for bricks that did not fit the list.
// DYN (vct_set_dynamic_bounce, include/vct.h "dynamic mesh"): the bounce over a chain the dynamic layer was merged into.
// A voxel the layer occupies -- its radiance pool shows alpha != 0 there -- takes albedo and normal from the layer's
// pools, every other voxel from the static pools as ever; the bricks are the static slots plus the layer's resolved
// bricks that have no static slot.  The layer's brick -> slot table is empty again behind its merge, so
// k_bounce_dyn_map writes one for the bounce from the resolved list.  The extra pointers ride behind VctTraceParams in
// the argument block of the DYN instantiations only.
struct BounceDyn {
    const uint32_t* res_brick;   // [max_bricks] slot -> brick of the last resolved pass, meaningful below *used only
    const uint32_t* used;        // that pass's statistics word: slots in use (capped by max_bricks where it is read)
    const uint32_t* pool_rad;    // [max_bricks][512] the layer's texels before lights: alpha != 0 = the layer owns the voxel
    const uint32_t* pool_alb;
    const uint32_t* pool_nrm;
    const uint32_t* brick_res;   // [nbricks] brick -> resolved slot, VCT_NO_SLOT elsewhere (k_bounce_dyn_map)
    uint32_t max_bricks;
};
template <bool DYN> struct BounceArgs : VctTraceParams {};
template <> struct BounceArgs<true> : VctTraceParams { BounceDyn d; };
static_assert(sizeof(BounceArgs<false>) == sizeof(VctTraceParams), "the static instantiations keep their argument block");

__device__ __forceinline__ uint32_t bounce_dyn_used(const BounceDyn& d) { return min(*d.used, d.max_bricks); }

// brick -> resolved slot of the layer, over a table of VCT_NO_SLOT (the host clears it in front): a thread per used slot
__global__ void __launch_bounds__(256)
k_bounce_dyn_map(const BounceDyn d, uint32_t nbricks, uint32_t* __restrict__ brick_res) {
    const uint32_t used = bounce_dyn_used(d);
    for (uint32_t sl = blockIdx.x * blockDim.x + threadIdx.x; sl < used; sl += gridDim.x * blockDim.x) {
        const uint32_t b = d.res_brick[sl];
        if (b < nbricks) brick_res[b] = sl;
    }
}

template <bool WRAP, int FASTDIV, bool DYN>
__device__ __forceinline__ void bounce_voxels(const BounceArgs<DYN>& p, bool alive, size_t vox, int& total_out,
                                              float4* __restrict__ blk, const LaneBlock& lb, MarchStats& ms) {
    const uint32_t* __restrict__ level0 = p.chain;          // level 0 starts the chain
    const float fV = (float)p.V;
    // attributes are pooled per touched brick; lanes without a voxel (alive == false) may point at a brick that
    // has no slot: they read slot 0 and their result is discarded
    const uint32_t slot = p.brick_slot[vox >> 9];
    const size_t pv = (size_t)(slot == VCT_NO_SLOT ? 0u : slot) * 512 + (vox & 511u);
    const uint32_t src = level0[vox];
    uint32_t nq = p.attr_normal[pv], aq = p.attr_albedo[pv];
    if constexpr (DYN) {      // the owner's attributes: a lane without a slot of the layer reads its slot 0 and keeps the static ones
        const uint32_t ds = p.d.brick_res[vox >> 9];
        const size_t dv = (size_t)(ds == VCT_NO_SLOT ? 0u : ds) * 512 + (vox & 511u);
        const uint32_t dr = p.d.pool_rad[dv], dn = p.d.pool_nrm[dv], da = p.d.pool_alb[dv];
        if (ds != VCT_NO_SLOT && (dr >> 24) != 0u) { nq = dn; aq = da; }
    }
    const uint32_t mi = (uint32_t)vox;
    const int i = (int)vct_compact3(mi), j = (int)vct_compact3(mi >> 1), k = (int)vct_compact3(mi >> 2);
    const F3 P = f3((div_rn((float)i + 0.5f, fV) - 0.5f) * p.G, (div_rn((float)j + 0.5f, fV) - 0.5f) * p.G,
                    (div_rn((float)k + 0.5f, fV) - 0.5f) * p.G);
    const F3 nrm = normalize3(f3((float)((int)(nq & 0xffu) - 128), (float)((int)((nq >> 8) & 0xffu) - 128),
                                 (float)((int)((nq >> 16) & 0xffu) - 128)));
    const F3 helper = fabsf(nrm.y) < 0.9f ? f3(0.0f, 1.0f, 0.0f) : f3(1.0f, 0.0f, 0.0f);
    const F3 t = normalize3(cross3(helper, nrm));
    const F3 bt = cross3(nrm, t);
    const F3 start = cone_start(P, nrm, p.vs);
    int total = 0;
    const F4 ind = gather_six_cones(t, bt, nrm, total,
        [&](F3 dir, int& st) { return cone_march<WRAP, FASTDIV, march_form(MF_COOP)>(p, alive, start, dir, p.steps_diffuse, p.n_diffuse, blk, lb, st, ms); },
        [](int, F4, int) {});
    if (alive) {
        const float occlusion = 1.0f - ind.w;
        const uint32_t r = vct_float_to_unorm8(unorm8(src & 0xffu) + unorm8(aq & 0xffu) * (occlusion * ind.x));
        const uint32_t g = vct_float_to_unorm8(unorm8((src >> 8) & 0xffu) + unorm8((aq >> 8) & 0xffu) * (occlusion * ind.y));
        const uint32_t bl = vct_float_to_unorm8(unorm8((src >> 16) & 0xffu) + unorm8((aq >> 16) & 0xffu) * (occlusion * ind.z));
        p.bounce_out[vox] = r | (g << 8) | (bl << 16) | (src & 0xff000000u);
    } else {
        total = 0;
    }
    total_out = wave_sum(total);
}

#define VCT_BOUNCE_SETUP                                                     \
    __shared__ float4 lds_blk[VCT_WAVES_PER_BLOCK][2][64];                   \
    const int lane = threadIdx.x & 63;                                       \
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); \
    float4* blk = &lds_blk[wave][0][0];                                      \
    const LaneBlock lb = make_lane_block(p, lane);                           \
    MarchStats ms = {};

// compaction of one brick into `list` (LDS); returns the number of occupied voxels
template <bool DYN>
__device__ __forceinline__ int compact_brick(const BounceArgs<DYN>& p, uint32_t b, int lane, uint16_t* list) {
    // a brick without a slot holds nothing of the current mesh (the host refuses the bounce when the attributes
    // are stale, vct_capi.hip attrs_valid; this keeps the index in bounds regardless)
    const uint32_t slot = p.brick_slot[b];
    const bool has = slot != VCT_NO_SLOT;
    const uint32_t* __restrict__ src = p.chain + (size_t)b * 512 + lane;
    const uint32_t* __restrict__ nrm = p.attr_normal + (size_t)(has ? slot : 0u) * 512 + lane;
    // all sixteen loads of the brick in flight before the first ballot (one round trip, not eight)
    uint32_t t[8], a[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) { t[it] = src[it * 64]; a[it] = nrm[it * 64]; }
    if constexpr (DYN) {      // the owner's normal per voxel; a voxel nobody owns counts as one with a zero normal
        const uint32_t ds = p.d.brick_res[b];
        const bool dyn = ds != VCT_NO_SLOT;
        const uint32_t* __restrict__ dr = p.d.pool_rad + (size_t)(dyn ? ds : 0u) * 512 + lane;
        const uint32_t* __restrict__ dn = p.d.pool_nrm + (size_t)(dyn ? ds : 0u) * 512 + lane;
        uint32_t r[8], m[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) { r[it] = dr[it * 64]; m[it] = dn[it * 64]; }
#pragma unroll
        for (int it = 0; it < 8; ++it) a[it] = dyn && (r[it] >> 24) != 0u ? m[it] : (has ? a[it] : 0x808080u);
    }
    int n = 0;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        p.bounce_out[(size_t)b * 512 + it * 64 + lane] = t[it];
        const bool occ = (t[it] >> 24) != 0u && (DYN || has) && (a[it] & 0xffffffu) != 0x808080u;
        const unsigned long long m = ballot64(occ);
        if (occ) list[n + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(it * 64 + lane);
        n += __popcll(m);
    }
    return n;
}

// 16 waves per workgroup: the list positions of a workgroup's 16 bricks are reserved with ONE atomic on the list's
// counter.  One atomic per brick meant ~10^4 returning atomics on one address at 512^3, which the L2 executes one after
// the other (~12 ns each): they, not the bricks, were the 0.12-0.14 ms this kernel took (round 3).
#define VCT_BLIST_WAVES 16
template <bool DYN>
__global__ void __launch_bounds__(64 * VCT_BLIST_WAVES)
k_bounce_list(const BounceArgs<DYN> p) {
    __shared__ uint16_t lds_list[VCT_BLIST_WAVES][512];
    __shared__ uint32_t lds_n[VCT_BLIST_WAVES];
    __shared__ uint32_t lds_base;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint16_t* list = &lds_list[wave][0];
    const uint32_t nwaves = gridDim.x * VCT_BLIST_WAVES;
    // (1) bricks the bounce chain still shows from an older pass and that hold nothing now are cleared.  The flags
    // are scanned 64 bricks at a time, one per lane (a 512^3 grid has 262,144 bricks, 2 % of them touched).
    const uint32_t nchunks = (p.nbricks + 63u) >> 6;
    for (uint32_t c = blockIdx.x * VCT_BLIST_WAVES + wave; c < nchunks; c += nwaves) {
        const uint32_t mine = c * 64u + (uint32_t)lane;
        const bool stale = mine < p.nbricks && p.brick_prev[mine] == 0u && p.bounce_seen[mine] != 0u;
        for (unsigned long long m = ballot64(stale); m != 0ull; m &= m - 1ull) {
            const uint32_t b = c * 64u + (uint32_t)(__ffsll((long long)m) - 1);
            for (int it = 0; it < 8; ++it) p.bounce_out[(size_t)b * 512 + it * 64 + lane] = 0u;
        }
    }
    // (2) the touched bricks, one wave each, found through the voxelizer's slot table (every brick level 0 can show
    // content in has a slot) instead of a scan of the grid.  DYN: behind them the layer's used slots, of which those
    // whose brick has a static slot are passed over -- every brick once.
    uint32_t nlist = p.nslots;
    if constexpr (DYN) nlist += bounce_dyn_used(p.d);
    for (uint32_t s0 = blockIdx.x * VCT_BLIST_WAVES; s0 < nlist; s0 += nwaves) {        // workgroup-uniform trip count
        const uint32_t sl = s0 + (uint32_t)wave;
        uint32_t b = 0u;
        int n = 0;
        if (sl < p.nslots) {
            b = p.slot_brick[sl];
            if (p.brick_prev[b]) n = compact_brick(p, b, lane, list);
        }
        if constexpr (DYN) {
            if (sl >= p.nslots && sl < nlist) {
                const uint32_t db = p.d.res_brick[sl - p.nslots];
                if (db < p.nbricks && p.brick_slot[db] == VCT_NO_SLOT && p.brick_prev[db]) {
                    b = db;
                    n = compact_brick(p, b, lane, list);
                }
            }
        }
        if (lane == 0) lds_n[wave] = (uint32_t)n;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0u;
            for (int w = 0; w < VCT_BLIST_WAVES; ++w) total += lds_n[w];
            lds_base = total ? atomicAdd(p.bounce_list_count, total) : 0u;
        }
        __syncthreads();
        if (n != 0) {
            uint32_t off = lds_base;
            for (int w = 0; w < wave; ++w) off += lds_n[w];
            if (off + (uint32_t)n > p.bounce_list_cap) {
                // does not fit: k_bounce_bricks takes this brick (and resets the flag).  At most one brick straddles the
                // end of the list; it marks the entries it reserved there as empty, so the list needs no clear.
                if (lane == 0) p.brick_over[b] = 1u;
                for (uint32_t i = off + (uint32_t)lane; i < p.bounce_list_cap; i += 64u) p.bounce_list[i] = 0xffffffffu;
            } else {
                for (int i = lane; i < n; i += 64) p.bounce_list[off + i] = b * 512u + list[i];
            }
        }
        __syncthreads();           // lds_n / lds_base / the lists are reused by the next round
    }
}

#ifndef VCT_BOUNCE_MIN_WAVES
#define VCT_BOUNCE_MIN_WAVES 5     // the per-voxel frame + attribute state spills under the trace kernel's budget; A/B at 512^3
                                   // (bounce + mips, ms): 4: 0.495, 5: 0.489, 6: 0.500, 7: 0.504
#endif
template <bool WRAP, int FASTDIV, bool DYN>
__global__ void __launch_bounds__(64 * VCT_WAVES_PER_BLOCK, VCT_BOUNCE_MIN_WAVES)
k_bounce_march(const BounceArgs<DYN> p) {
    VCT_BOUNCE_SETUP
    const uint32_t n = min(*p.bounce_list_count, p.bounce_list_cap);
    const uint32_t nwaves = gridDim.x * VCT_WAVES_PER_BLOCK;
    unsigned long long wave_steps = 0;
    for (uint32_t w = blockIdx.x * VCT_WAVES_PER_BLOCK + wave; w * 64u < n; w += nwaves) {
        const uint32_t e = w * 64u + lane < n ? p.bounce_list[w * 64u + lane] : 0xffffffffu;
        const bool alive = e != 0xffffffffu;               // unwritten slots belong to overflowed bricks
        const uint32_t first = __builtin_amdgcn_readfirstlane(e);
        const size_t vox = alive ? e : (first != 0xffffffffu ? first : 0u);
        int total;
        bounce_voxels<WRAP, FASTDIV, DYN>(p, alive, vox, total, blk, lb, ms);
        wave_steps += (unsigned long long)total;
    }
    if (lane == 0 && wave_steps)
        atomicAdd(p.step_counter + ((blockIdx.x * VCT_WAVES_PER_BLOCK + wave) & (VCT_STEP_COUNTERS - 1)), wave_steps);
}

template <bool WRAP, int FASTDIV, bool DYN>
__global__ void __launch_bounds__(64 * VCT_WAVES_PER_BLOCK, VCT_BOUNCE_MIN_WAVES)
k_bounce_bricks(const BounceArgs<DYN> p) {
    VCT_BOUNCE_SETUP
    __shared__ uint16_t lds_list[VCT_WAVES_PER_BLOCK][512];
    uint16_t* list = &lds_list[wave][0];
    unsigned long long wave_steps = 0;
    const uint32_t nwaves = gridDim.x * VCT_WAVES_PER_BLOCK;
    // flags of the slots scanned 64 at a time, one per lane; a served brick's flag is reset for the next pass
    // DYN: behind them the layer's used slots whose brick has no static slot, as k_bounce_list lists them
    uint32_t nscan = p.nslots;
    if constexpr (DYN) nscan += bounce_dyn_used(p.d);
    const uint32_t nchunks = (nscan + 63u) >> 6;
    for (uint32_t c = blockIdx.x * VCT_WAVES_PER_BLOCK + wave; c < nchunks; c += nwaves) {
        const uint32_t sl = c * 64u + (uint32_t)lane;
        uint32_t mine = sl < p.nslots ? p.slot_brick[sl] : 0u;
        bool over = sl < p.nslots && p.brick_over[mine] != 0u;
        if constexpr (DYN) {
            if (sl >= p.nslots && sl < nscan) {
                const uint32_t db = p.d.res_brick[sl - p.nslots];
                if (db < p.nbricks && p.brick_slot[db] == VCT_NO_SLOT) { mine = db; over = p.brick_over[db] != 0u; }
            }
        }
        if (over) p.brick_over[mine] = 0u;
        for (unsigned long long m = ballot64(over); m != 0ull; m &= m - 1ull) {
            const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)mine, __ffsll((long long)m) - 1);
            const int n = compact_brick(p, b, lane, list);
            wave_sync();
            for (int base = 0; base < n; base += 64) {
                const bool alive = base + lane < n;
                const size_t vox = (size_t)b * 512 + (alive ? list[base + lane] : list[base]);
                int total;
                bounce_voxels<WRAP, FASTDIV, DYN>(p, alive, vox, total, blk, lb, ms);
                wave_steps += (unsigned long long)total;
            }
            wave_sync();
        }
    }
    if (lane == 0 && wave_steps)
        atomicAdd(p.step_counter + ((blockIdx.x * VCT_WAVES_PER_BLOCK + wave) & (VCT_STEP_COUNTERS - 1)), wave_steps);
}

// Live-pixel compaction (experiment, north_star "compact still-active cones"; profiles/experiments/README.md): one wave
// per 16x16-pixel super-tile of the launched rows gathers the live pixels (albedo.a >= 0.5, trace.fs:169-172) of its up
// to four 8x8 tiles into whole waves of 64 -- "virtual tiles" -- and gives the discarded pixels their clear colour
// (VCT.h:156-159) right away.  The trace then runs one workgroup per virtual tile.
__global__ void __launch_bounds__(256)
k_compact_tiles(const VctTraceParams p) {
    const int lane = threadIdx.x & 63;
    const int rows = p.tile_row1 - p.tile_row0;
    const int sx_n = (p.tiles_x + 1) >> 1, sy_n = (rows + 1) >> 1;
    const int st = blockIdx.x * (blockDim.x >> 6) + (int)(threadIdx.x >> 6);
    if (st >= sx_n * sy_n) return;
    const int sy = st / sx_n, sx = st - sy * sx_n;
    unsigned long long m[4];
    int tiles[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tx = 2 * sx + (k & 1), ty = p.tile_row0 + 2 * sy + (k >> 1);
        const bool have = tx < p.tiles_x && ty < p.tile_row1;
        tiles[k] = have ? ty * p.tiles_x + tx : -1;
        bool live = false;
        if (have) {
            const int x = tx * VCT_TILE + (lane & 7), y = ty * VCT_TILE + (lane >> 3);
            const bool in_frame = x < p.width && y < p.height;
            const float a = p.gbuf[(size_t)tiles[k] * (VCT_GB_NPLANES * VCT_TILE_PIX) + 18 * VCT_TILE_PIX + lane];
            live = in_frame && !(a < 0.5f);
            if (in_frame && !live) {
                const float cc = clear_colour(p);
                uint2 pk;
                pk.x = pack_half2(cc, cc);
                pk.y = pack_half2(cc, 1.0f);
                *reinterpret_cast<uint2*>(p.out + ((size_t)y * p.width + x) * 4) = pk;
            }
        }
        m[k] = ballot64(live);
    }
    const int total = (int)(__popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]));
    const int nvt = (total + 63) >> 6;
    uint32_t base = 0u;
    if (lane == 0 && nvt) base = atomicAdd(p.vt_count, (uint32_t)nvt);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((m[k] >> lane) & 1ull)
            p.vt_pix[(size_t)base * 64 + n + __popcll(m[k] & ((1ull << lane) - 1ull))] = ((uint32_t)tiles[k] << 6) | (uint32_t)lane;
        n += (int)__popcll(m[k]);
    }
    for (int i = total + lane; i < nvt * 64; i += 64) p.vt_pix[(size_t)base * 64 + i] = 0xffffffffu;
}

// ---- launch dispatch: run-time parameters to template arguments, written once -----------------------------------------
// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a type, so that a generic lambda can name the
// instantiation it launches (decltype(tag)::value)
template <class F>
auto with_flag(bool flag, F f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }
// f(WRAP tag, FASTDIV tag) of a launch: GL_REPEAT or clamp (p.wrap_repeat), and the division form of the march the step
// tables were built for -- 1 the verified two-term product (p.fast_div), 0 the IEEE divide (div_const)
template <class F>
auto with_march_mode(const VctTraceParams& p, F f) {
    return with_flag(p.wrap_repeat != 0, [&](auto wrap) {
        return with_flag(p.fast_div != 0, [&](auto fast) { return f(wrap, std::integral_constant<int, decltype(fast)::value ? 1 : 0>{}); });
    });
}

template <bool WRAP, int FASTDIV, bool COOP>
hipError_t launch(const VctTraceParams& p, int blocks, hipStream_t s) {
    hipLaunchKernelGGL((k_trace_tile<WRAP, FASTDIV, COOP>), dim3(blocks),
                       dim3(64 * VCT_WAVES_PER_BLOCK), 0, s, p);
    return hipGetLastError();
}

// The default kernel in the form the plan names (vct_trace_forms.h vct_plan_launch): a fold over the table of the forms
// that exist, which launches the entry that equals `form` -- so the instantiated set is the table, under this WRAP.  A form
// the table does not hold (under this WRAP) has no kernel: an error, never another kernel.
template <bool WRAP, int FASTDIV, size_t... I>
hipError_t launch_split_form(VctSplitForm form, const VctTraceParams& p, int blocks, hipStream_t s, std::index_sequence<I...>) {
    bool launched = false;
    auto entry = [&](auto i) {
        constexpr VctSplitForm FORM = kVctSplitForms[decltype(i)::value];
        if constexpr (split_form_exists(WRAP, FORM)) {
            if (FORM == form) {
                hipLaunchKernelGGL((k_trace_tile_split<WRAP, FASTDIV, FORM>), dim3(blocks), dim3(64 * VCT_SPLIT), 0, s, p);
                launched = true;
            }
        }
    };
    (entry(std::integral_constant<size_t, I>{}), ...);
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}
template <bool WRAP, int FASTDIV>
hipError_t launch_split_kernel(const VctLaunchPlan& plan, const VctTraceParams& p, int blocks, hipStream_t s) {
    if (plan.fastdiv == 2) {      // variant 3's kernel: one form, on top of the table
        hipLaunchKernelGGL((k_trace_tile_split<WRAP, 2, split_form(SF_PLAIN)>), dim3(blocks), dim3(64 * VCT_SPLIT), 0, s, p);
        return hipGetLastError();
    }
    return launch_split_form<WRAP, FASTDIV>(plan.form, p, blocks, s, std::make_index_sequence<(size_t)kVctSplitFormCount>{});
}

// the four launches of a half-rate pass (p.dr_ind set: whole frame, default kernel, p.comp on); marks: see vct_launch_trace
template <bool WRAP, int FASTDIV, int WAVES>
void launch_point_march(const VctTraceParams& p, bool listed, int blocks, hipStream_t s) {
    if (p.sky) {          // sky light: the marches of a half-rate pass add it as rate 1's do
        if (listed) hipLaunchKernelGGL((k_point_march<WRAP, FASTDIV, true, WAVES, true>), dim3(blocks), dim3(64 * WAVES), 0, s, p);
        else hipLaunchKernelGGL((k_point_march<WRAP, FASTDIV, false, WAVES, true>), dim3(blocks), dim3(64 * WAVES), 0, s, p);
        return;
    }
    if (listed) hipLaunchKernelGGL((k_point_march<WRAP, FASTDIV, true, WAVES>), dim3(blocks), dim3(64 * WAVES), 0, s, p);
    else hipLaunchKernelGGL((k_point_march<WRAP, FASTDIV, false, WAVES>), dim3(blocks), dim3(64 * WAVES), 0, s, p);
}
template <bool WRAP, int FASTDIV>
hipError_t launch_half_rate(const VctLaunchPlan& plan, const VctTraceParams& p, int blocks, hipStream_t s, const hipEvent_t* marks) {
    auto mark = [&](int i) { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    hipError_t e = hipMemsetAsync(p.dr_ctr, 0, VCT_DR_CTR_WORDS * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const int cw = (p.width + 1) >> 1, ch = (p.height + 1) >> 1;
    const int coarse_blocks = ((cw + 7) >> 3) * ((ch + 7) >> 3);
    if (p.dr_waves == 2) launch_point_march<WRAP, FASTDIV, 2>(p, false, coarse_blocks, s);
    else launch_point_march<WRAP, FASTDIV, 1>(p, false, coarse_blocks, s);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark(0)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_diffuse_resolve, dim3((p.tiles_x * p.tiles_y + 3) / 4), dim3(256), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark(1)) != hipSuccess) return e;
    // over the list's device-side count: enough workgroups for a frame of fill pixels, at most the bounce's grid
    const long long full = ((long long)p.width * p.height + 63) / 64;
    const int listed_blocks = (int)(full < 256 * 24 ? full : 256 * 24);
    if (p.dr_waves == 2) launch_point_march<WRAP, FASTDIV, 2>(p, true, listed_blocks, s);
    else launch_point_march<WRAP, FASTDIV, 1>(p, true, listed_blocks, s);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark(2)) != hipSuccess) return e;
    return launch_split_kernel<WRAP, FASTDIV>(plan, p, blocks, s);
}

// what the plan names, launched
template <bool WRAP, int FASTDIV>
hipError_t launch_plan(const VctLaunchPlan& plan, const VctTraceParams& p, hipStream_t s, const hipEvent_t* marks) {
    const int ntiles = p.ntiles;
    if (plan.family == VCT_FAMILY_TILE) {
        const int nblocks = (ntiles + VCT_WAVES_PER_BLOCK - 1) / VCT_WAVES_PER_BLOCK;
        const int blocks = ((nblocks + 7) / 8) * 8;     // whole rounds of the 8 XCDs
        return with_flag(plan.coop, [&](auto coop) { return launch<WRAP, FASTDIV, decltype(coop)::value>(p, blocks, s); });
    }
    const int blocks = ((ntiles + 7) / 8) * 8;
    if (p.vt_pix) {         // variant 4: compaction pre-pass (the counter was zeroed by the caller)
        const int rows = p.tile_row1 - p.tile_row0;
        const int nst = ((p.tiles_x + 1) >> 1) * ((rows + 1) >> 1);
        hipLaunchKernelGGL(k_compact_tiles, dim3((nst + 3) / 4), dim3(256), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (plan.family == VCT_FAMILY_HALF_RATE) return launch_half_rate<WRAP, FASTDIV>(plan, p, blocks, s, marks);
    return launch_split_kernel<WRAP, FASTDIV>(plan, p, blocks, s);
}

// every fp32 bit pattern: div_const<true> against the IEEE divide
__global__ void __launch_bounds__(256)
k_divide_selftest(float d, float r, float aux, unsigned long long* mismatches) {
    unsigned long long bad = 0;
    const unsigned long long total = 1ull << 32;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = __uint_as_float((uint32_t)i);
        if (!(fabsf(x) <= 3.0e38f)) continue;                 // inf / nan
        if (fabsf(x) < VCT_DIV_TINY && (uint32_t)i != 0u) continue;   // outside the documented domain
        const float want = x / d;
        if (want != 0.0f && fabsf(want) < 1.17549435e-38f) continue;   // subnormal quotient
        if (fabsf(want) > 3.0e38f) continue;
        const float got = div_const<1>(x, aux, r);
        if (__float_as_uint(got) != __float_as_uint(want)) { ++bad; mismatches[1] = i; }
    }
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(mismatches, bad);
}

// The texel buffer's conversion against the exact decode, texel by texel: out[0] = channels that differ, out[1] = the
// first offending texel word (vct_selftest_texel_buffer; vct_create runs it once per process)
// ... and the chain form of the samplers' loads: `buf` = [lead][n][n] texels, `lead` texels of anything and the n test
// texels twice -- two levels of a chain that starts at buf, read through ONE resource over buf with their byte offsets
// (both non-zero) as the scalar offset operand, the first up to its last texel below the second's start.  out[2] =
// channels whose bits differ from the zero-offset load's of the same texel, out[3] = an offending texel word.
__global__ void __launch_bounds__(256)
k_texel_buffer_selftest(const uint32_t* buf, uint32_t lead, uint32_t n, unsigned long long* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* texels = buf + lead;
    const float4 d = texel_f32(level_texel_buffer(texels), i);
    const uint32_t t = texels[i];
    const float want[4] = {vct_unorm8_to_float(t & 0xffu), vct_unorm8_to_float((t >> 8) & 0xffu),
                           vct_unorm8_to_float((t >> 16) & 0xffu), vct_unorm8_to_float(t >> 24)};
    const float got[4] = {d.x, d.y, d.z, d.w};
    for (int ch = 0; ch < 4; ++ch)
        if (__float_as_uint(got[ch]) != __float_as_uint(want[ch])) { atomicAdd(&out[0], 1ull); out[1] = t; }
    const vct_v4i32 chain = level_texel_buffer(buf);
    const float4 o1 = texel_f32(chain, i, lead * 4u), o2 = texel_f32(chain, i, (lead + n) * 4u);
    const float via[8] = {o1.x, o1.y, o1.z, o1.w, o2.x, o2.y, o2.z, o2.w};
    for (int k = 0; k < 8; ++k)
        if (__float_as_uint(via[k]) != __float_as_uint(got[k & 3])) { atomicAdd(&out[2], 1ull); out[3] = t; }
}

}  // namespace

hipError_t vct_launch_texel_buffer_selftest(const uint32_t* buf, uint32_t lead, uint32_t n, unsigned long long* out, hipStream_t s) {
    hipLaunchKernelGGL(k_texel_buffer_selftest, dim3((n + 255u) / 256u), dim3(256), 0, s, buf, lead, n, out);
    return hipGetLastError();
}

hipError_t vct_launch_divide_selftest(float d, unsigned long long* mismatches, hipStream_t s) {
    const float r = 1.0f / d;
    hipLaunchKernelGGL(k_divide_selftest, dim3(256 * 16), dim3(256), 0, s, d, r, vct_div_aux(d, r), mismatches);
    return hipGetLastError();
}

// Point queries: always the exact march (FASTDIV 0 or 1 as the step tables were built), isotropic chain, no footprint records.
template <bool WRAP, int FASTDIV>
hipError_t launch_query(const VctTraceParams& p, const VctQueryArgs& q, int kind, hipStream_t s) {
    const uint32_t nitems = (q.n + 63u) >> 6;
    const dim3 grid(nitems < 256u * 24u ? nitems : 256u * 24u), block(64);          // at most the bounce's grid
    with_flag(kind == VCT_QUERY_GATHER, [&](auto gather) {
        with_flag(q.out_cones || q.out_steps, [&](auto debug) {
            constexpr int KIND = decltype(gather)::value ? VCT_QUERY_GATHER : VCT_QUERY_CONE;
            if (p.sky) hipLaunchKernelGGL((k_query_march<WRAP, FASTDIV, KIND, decltype(debug)::value, true>), grid, block, 0, s, p, q);
            else hipLaunchKernelGGL((k_query_march<WRAP, FASTDIV, KIND, decltype(debug)::value>), grid, block, 0, s, p, q);
        });
    });
    return hipGetLastError();
}

hipError_t vct_launch_query(const VctTraceParams& p, const VctQueryArgs& q, int kind, hipStream_t s) {
    if (q.n == 0u) return hipSuccess;
    if (p.aniso || p.cells_biased || (kind != VCT_QUERY_GATHER && kind != VCT_QUERY_CONE)) return hipErrorInvalidValue;
    return with_march_mode(p, [&](auto wrap, auto fastdiv) {
        return launch_query<decltype(wrap)::value, decltype(fastdiv)::value>(p, q, kind, s);
    });
}

hipError_t vct_launch_query_keys(const VctTraceParams& p, const VctQueryArgs& q, int kind, uint32_t* keys, uint32_t* index, hipStream_t s) {
    if (q.n == 0u) return hipSuccess;
    const dim3 grid((q.n + 255u) / 256u), block(256);
    with_flag(p.wrap_repeat != 0, [&](auto wrap) {     // (the keys divide by no table constant: one kernel for both forms)
        with_flag(kind == VCT_QUERY_GATHER, [&](auto gather) {
            constexpr int KIND = decltype(gather)::value ? VCT_QUERY_GATHER : VCT_QUERY_CONE;
            hipLaunchKernelGGL((k_query_keys<decltype(wrap)::value, KIND>), grid, block, 0, s, p, q, keys, index);
        });
    });
    return hipGetLastError();
}

template <bool WRAP, int FASTDIV, bool DYN>
hipError_t launch_bounce(const BounceArgs<DYN>& p, uint32_t list_slots, hipStream_t s) {
    uint32_t blocks = (p.nbricks + VCT_WAVES_PER_BLOCK - 1) / VCT_WAVES_PER_BLOCK;
    if (blocks > 256u * 64u) blocks = 256u * 64u;
    const dim3 block(64 * VCT_WAVES_PER_BLOCK);
    uint32_t lblocks = (list_slots + VCT_BLIST_WAVES - 1) / VCT_BLIST_WAVES;             // one wave per touched brick
    if (lblocks > 256u * 8u) lblocks = 256u * 8u;
    if (lblocks < 64u) lblocks = 64u;
    hipLaunchKernelGGL(k_bounce_list<DYN>, dim3(lblocks), dim3(64 * VCT_BLIST_WAVES), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_bounce_march<WRAP, FASTDIV, DYN>), dim3(256 * 24), block, 0, s, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_bounce_bricks<WRAP, FASTDIV, DYN>), dim3(blocks), block, 0, s, p);
    return hipGetLastError();
}

hipError_t vct_launch_bounce(const VctTraceParams& p, hipStream_t s, const VctBounceDynArgs* dyn) {
    if (p.nbricks == 0) return hipSuccess;
    if (dyn) {
        BounceArgs<true> q;
        static_cast<VctTraceParams&>(q) = p;
        q.d.res_brick = dyn->res_brick; q.d.used = dyn->used;
        q.d.pool_rad = dyn->pool_rad; q.d.pool_alb = dyn->pool_alb; q.d.pool_nrm = dyn->pool_nrm;
        q.d.brick_res = dyn->brick_res; q.d.max_bricks = dyn->max_bricks;
        hipLaunchKernelGGL(k_bounce_dyn_map, dim3((dyn->max_bricks + 255u) / 256u), dim3(256), 0, s, q.d, p.nbricks, dyn->brick_res);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        return with_march_mode(p, [&](auto wrap, auto fastdiv) {
            return launch_bounce<decltype(wrap)::value, decltype(fastdiv)::value, true>(q, dyn->list_slots, s);
        });
    }
    BounceArgs<false> q;
    static_cast<VctTraceParams&>(q) = p;
    return with_march_mode(p, [&](auto wrap, auto fastdiv) {
        return launch_bounce<decltype(wrap)::value, decltype(fastdiv)::value, false>(q, p.nslots, s);
    });
}

// The screen trace of tile rows [tile_row0, tile_row1) (every row_stride-th of them).  variant = config.trace_variant
// (include/vct.h): 0 (default) the cooperative sampler with each tile split over 3 waves; 1 the per-lane sampler only and
// 2 the cooperative sampler, one wave per tile (k_trace_tile; with anisotropic chains both run the default kernel);
// 3 the default kernel with reciprocal-multiply divisions and the one-multiply decode, not bit-exact (with anisotropic
// chains: the default kernel); 4 the default kernel over the live-pixel compaction (p.vt_pix set by the caller).
// Which kernel that is, and which combinations have none (hipErrorInvalidValue): vct_trace_forms.h vct_plan_launch, from
// the facts gathered below; this function executes the plan.
// p.ntiles, p.tile_mul, p.tile_shift and p.light_unit are set here.  *march_form (optional) receives the division form of the launch as vct_get_stage_counts reports
// it -- 1 IEEE, 2 the verified product, 3 variant 3's x * r; bits 8-9: how the launch's typed loads reach a level, 2 one
// resource per wave (the CHAIN forms), 1 one per level -- also for an empty row range, which launches nothing.
// p.dr_ind set: a half-rate pass (vct_set_diffuse_rate(ctx, 2)) -- coarse march, resolve, listed march, then the trace
// kernel that composites; whole frames of the default kernel with p.comp on only.  marks (optional): three events
// recorded between those four launches.
hipError_t vct_launch_trace(const VctTraceParams& params, int variant, hipStream_t s, int* march_form, const hipEvent_t* marks) {
    VctTraceParams p = params;
    const int rstride = p.row_stride > 1 ? p.row_stride : 1;
    p.ntiles = ((p.tile_row1 - p.tile_row0 + rstride - 1) / rstride) * p.tiles_x;
    // what else is the same for every tile of the launch (vct_tilediv.h): the division by tiles_x as a multiplier and a
    // shift -- (0, 0) where the host cannot certify them: the kernels divide -- and the composite's unit light vector
    const VctTileDiv td = vct_tilediv_make(p.tiles_x > 0 ? (uint32_t)p.tiles_x : 0u);
    p.tile_mul = td.mul;
    p.tile_shift = td.shift;
    vct_light_unit(p.light, p.light_unit);
    VctLaunchFacts f = {};
    f.variant = variant;
    f.wrap = p.wrap_repeat != 0; f.fast_div = p.fast_div != 0;
    f.aniso = p.aniso != nullptr; f.cells = p.cells_biased != nullptr;
    f.comp = p.comp != 0; f.sky = p.sky != nullptr;
    f.gloss_plane = p.pix_gloss != nullptr; f.gloss_table = p.gloss != nullptr;
    f.half_rate = p.dr_ind != nullptr; f.compact_list = p.vt_pix != nullptr;
    f.spec_prio = p.spec_prio != 0; f.chain_form = p.chain_form != 0;
    f.strided = rstride > 1; f.packed = p.pack_rows != 0;
    f.whole_frame = p.tile_row0 == 0 && p.tile_row1 == p.tiles_y;
    const VctLaunchPlan plan = vct_plan_launch(f);
    if (march_form) *march_form = plan.reported_form;
    if (p.ntiles <= 0) return hipSuccess;
    if (plan.refused) return hipErrorInvalidValue;
    return with_march_mode(p, [&](auto wrap, auto fastdiv) {
        return launch_plan<decltype(wrap)::value, decltype(fastdiv)::value>(plan, p, s, marks);
    });
}
