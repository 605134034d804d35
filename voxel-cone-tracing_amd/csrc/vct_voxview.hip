// vct_voxview.hip -- the voxel view: every pixel's ray walked cell by cell through one level of the Morton brick chain
// (or a per-voxel attribute), composited front to back with the march's own rule (S/VoxelConeTracing.fs:100,102).
//
// No reference counterpart: the reference has no "show me the voxels" mode.  The definition is this build's and is
// written out in include/vct.h ("voxel view"); tests/voxel_view_ref.py restates it in numpy.  All of it is fp32 in the
// written order (compile with -ffp-contract=off), divisions are IEEE, and every plane parameter t_a is a pure function of
// an integer plane index -- never accumulated -- so that the walk below and a plain walk visit the same cells.
//
// Kernels: k_voxview_occupancy (one bit per 8^3 block of the viewed level: "some texel word != 0") and k_voxview (one
// wave per 8x8 pixel tile, lane = pixel, like the trace).
//
// Empty space.  A zero parent texel does not prove zero children (the mip requantises: one child byte of 1 rounds to a
// parent 0) and the voxelizer's brick flags know nothing of uploaded chains, so the walk has an occupancy structure of
// its own, derived from the texels it would fetch: bit (bz, by, bx) of word (sz, sy, sx) is set when block
// (4 sx + bx, 4 sy + by, 4 sz + bz) of 8^3 texels holds a non-zero word; a 64-bit word covers 32^3 texels.  1024^3:
// 32,768 words = 256 KiB, resident in L2 beside any chain.  Inside a block whose bit is clear the walk keeps stepping
// cells with ALU only -- a visit of a zero texel adds oma * 0 to sums that are never -0 and leaves A as it was, so
// leaving the fetch out changes no bit -- and fetches the next word when it crosses into another 32^3 region.
#include "../../include/vct.h"
#include "vct_internal.h"
#include "vct_texel.h"

namespace {

// linear bit of block (bx, by, bz) in its word, from the block's Morton index inside the 4x4x4 group
__device__ __forceinline__ uint32_t group_bit(uint32_t i) {
    return vct_compact3(i) | (vct_compact3(i >> 1) << 2) | (vct_compact3(i >> 2) << 4);
}

// One wave per occupancy word.  The 64 blocks of a word are 64 consecutive Morton blocks (32 KiB of texels, or of pooled
// attribute slots); a block is two 16-byte loads per lane.
__global__ void __launch_bounds__(64)
k_voxview_occupancy(VctVoxViewParams p) {
    const int lane = threadIdx.x;
    const uint32_t S = (uint32_t)p.occ_dim;
    const uint32_t word = blockIdx.x;                       // linear (sz * S + sy) * S + sx
    const uint32_t sx = word % S, sy = (word / S) % S, sz = word / (S * S);
    const uint32_t nb = (uint32_t)p.N >> 3;                 // blocks per side (0: the level is smaller than a block)
    const uint32_t btex = nb ? 512u : (uint32_t)(p.N * p.N * p.N);
    unsigned long long bits = 0ull;
    for (uint32_t i = 0; i < 64u; ++i) {
        const uint32_t bx = 4u * sx + (vct_compact3(i)), by = 4u * sy + vct_compact3(i >> 1), bz = 4u * sz + vct_compact3(i >> 2);
        if (bx >= max(nb, 1u) || by >= max(nb, 1u) || bz >= max(nb, 1u)) continue;      // (wave-uniform)
        const uint32_t mb = vct_morton3(bx, by, bz);
        const uint32_t* src = p.texels + (size_t)mb * 512;
        if (p.brick_slot) {
            const uint32_t slot = p.brick_slot[mb];
            if (slot == VCT_NO_SLOT) continue;
            src = p.texels + (size_t)slot * 512;
        }
        uint32_t v = 0u;
        if (btex == 512u) {
            const uint4 a = reinterpret_cast<const uint4*>(src)[lane], b = reinterpret_cast<const uint4*>(src)[64 + lane];
            v = a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w;
        } else if ((uint32_t)lane < btex) {
            v = src[lane];
        }
        if (__builtin_amdgcn_ballot_w64(v != 0u) != 0ull) bits |= 1ull << group_bit(i);
    }
    if (lane == 0) p.occ[word] = bits;
}

struct Axis {
    float g, e, inv;     // grid-unit origin, direction, 1 / e (unused where e == 0)
    int c, plane, step;  // cell, 1 where the next plane is the cell's upper one, +-1
};

__device__ __forceinline__ float plane_t(const Axis& a, int c) {
    return a.e != 0.0f ? ((float)(c + a.plane) - a.g) * a.inv : __builtin_inff();
}

template <bool SKIP>
__global__ void __launch_bounds__(64)
k_voxview(VctVoxViewParams p) {
    const int lane = threadIdx.x;
    const int tile = blockIdx.x;
    const int x = (tile % p.tiles_x) * VCT_TILE + (lane & 7), y = (tile / p.tiles_x) * VCT_TILE + (lane >> 3);
    if (x >= p.width || y >= p.height) return;
    const float N = (float)p.N, G = p.G;

    // ray of the pixel
    const float nx = (2.0f * ((float)x + 0.5f)) / (float)p.width - 1.0f;
    const float ny = (2.0f * ((float)y + 0.5f)) / (float)p.height - 1.0f;
    float r[2][4];
    for (int k = 0; k < 2; ++k) {
        const float nz = k ? 1.0f : -1.0f;
        for (int i = 0; i < 4; ++i) r[k][i] = ((p.m[i] * nx + p.m[4 + i] * ny) + p.m[8 + i] * nz) + p.m[12 + i];
    }
    Axis ax[3];
    bool hit = true, any_d = false;
    for (int a = 0; a < 3; ++a) {
        const float o = r[0][a] / r[0][3], f = r[1][a] / r[1][3];
        const float d = f - o;
        hit = hit && isfinite(o) && isfinite(d);
        any_d = any_d || d != 0.0f;
        ax[a].g = (o / G + 0.5f) * N;
        ax[a].e = (d / G) * N;
        ax[a].inv = ax[a].e != 0.0f ? 1.0f / ax[a].e : 0.0f;
        ax[a].plane = ax[a].e > 0.0f ? 1 : 0;
        ax[a].step = ax[a].e > 0.0f ? 1 : -1;
    }
    hit = hit && any_d;

    // entry
    float t_in = 0.0f, t_out = __builtin_inff();
    for (int a = 0; a < 3; ++a) {
        if (ax[a].e != 0.0f) {
            const float t0 = (0.0f - ax[a].g) * ax[a].inv, t1 = (N - ax[a].g) * ax[a].inv;
            const float lo = t1 < t0 ? t1 : t0, hi = t1 < t0 ? t0 : t1;
            t_in = lo > t_in ? lo : t_in;
            t_out = hi < t_out ? hi : t_out;
        } else {
            hit = hit && ax[a].g >= 0.0f && ax[a].g < N;
        }
    }
    hit = hit && t_in < t_out;

    float cr = 0.0f, cg = 0.0f, cb = 0.0f, A = 0.0f;
    if (hit) {
        for (int a = 0; a < 3; ++a) {
            float f = floorf(ax[a].g + t_in * ax[a].e);
            f = f > 0.0f ? f : 0.0f;
            f = f < N - 1.0f ? f : N - 1.0f;
            ax[a].c = (int)f;
        }
        int cx = ax[0].c, cy = ax[1].c, cz = ax[2].c;
        float tx = plane_t(ax[0], cx), ty = plane_t(ax[1], cy), tz = plane_t(ax[2], cz);
        const vct_v4i32 tb = level_texel_buffer(p.texels);
        const int Ni = p.N;
        int blk = -1, reg = -1;                 // block / 32^3 region of the last occupancy look-up
        unsigned long long word = 0ull;
        bool occupied = true;
        uint32_t base = 0u;                     // pooled attributes: first texel of the block's slot
        for (;;) {
            // visit
            const int b = (cx >> 3) | ((cy >> 3) << 8) | ((cz >> 3) << 16);
            if (b != blk) {
                blk = b;
                if (SKIP) {
                    const int rg = (cx >> 5) | ((cy >> 5) << 8) | ((cz >> 5) << 16);
                    if (rg != reg) {
                        reg = rg;
                        word = p.occ[((size_t)(cz >> 5) * p.occ_dim + (cy >> 5)) * p.occ_dim + (cx >> 5)];
                    }
                    occupied = (word >> ((((cz >> 3) & 3) << 4) | (((cy >> 3) & 3) << 2) | ((cx >> 3) & 3))) & 1ull;
                }
                if (p.brick_slot && occupied) {
                    const uint32_t slot = p.brick_slot[vct_morton3((uint32_t)cx >> 3, (uint32_t)cy >> 3, (uint32_t)cz >> 3)];
                    occupied = slot != VCT_NO_SLOT;      // a block without a slot holds zeros
                    base = slot << 9;
                }
            }
            if (occupied) {
                const uint32_t mi = vct_morton3((uint32_t)cx, (uint32_t)cy, (uint32_t)cz);
                const float4 T = texel_f32(tb, p.brick_slot ? base | (mi & 511u) : mi);
                const float oma = 1.0f - A;
                cr = cr + oma * T.x;
                cg = cg + oma * T.y;
                cb = cb + oma * T.z;
                A = A + oma * T.w;
            }
            if (A >= p.max_alpha) break;
            // step along the axis with the smallest t; ties go x before y before z
            int axis = 0;
            float tm = tx;
            if (ty < tm) { axis = 1; tm = ty; }
            if (tz < tm) axis = 2;
            if (axis == 0) {
                cx += ax[0].step;
                if ((unsigned)cx >= (unsigned)Ni) break;
                tx = plane_t(ax[0], cx);
            } else if (axis == 1) {
                cy += ax[1].step;
                if ((unsigned)cy >= (unsigned)Ni) break;
                ty = plane_t(ax[1], cy);
            } else {
                cz += ax[2].step;
                if ((unsigned)cz >= (unsigned)Ni) break;
                tz = plane_t(ax[2], cz);
            }
        }
    }
    uint2 pk;
    pk.x = pack_half2(cr, cg);
    pk.y = pack_half2(cb, A);
    *reinterpret_cast<uint2*>(p.out + ((size_t)y * p.width + x) * 4) = pk;
}

}  // namespace

hipError_t vct_launch_voxview_occupancy(const VctVoxViewParams& p, hipStream_t s) {
    const unsigned words = (unsigned)p.occ_dim * p.occ_dim * p.occ_dim;
    hipLaunchKernelGGL(k_voxview_occupancy, dim3(words), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t vct_launch_voxview(const VctVoxViewParams& p, bool skip, hipStream_t s) {
    const unsigned tiles = (unsigned)p.tiles_x * p.tiles_y;
    if (skip) hipLaunchKernelGGL(k_voxview<true>, dim3(tiles), dim3(64), 0, s, p);
    else hipLaunchKernelGGL(k_voxview<false>, dim3(tiles), dim3(64), 0, s, p);
    return hipGetLastError();
}
