// vct_texel.h -- what the kernels that read the chain and write a frame share (vct_trace.hip, vct_voxview.hip): a level
// of the chain as an RGBA8 UNORM texel buffer, and the frame's f32 -> f16 rounding.  Device code only.
#ifndef VCT_TEXEL_H_
#define VCT_TEXEL_H_

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vct_layout.h"

typedef int vct_v4i32 __attribute__((ext_vector_type(4)));
typedef float vct_v4f32 __attribute__((ext_vector_type(4)));
__device__ vct_v4f32 vct_struct_buffer_load_format_v4f32(vct_v4i32 rsrc, int vindex, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.struct.buffer.load.format.v4f32");

// A level of the chain as a TEXEL BUFFER: buffer resource with stride 4 and format 8_8_8_8 UNORM; the structured load takes
// the texel's Morton INDEX (a 4 GiB level -- 1024^3 level 0 -- is addressed in full; the raw byte-offset form fails its
// range check on that level's last texel) and returns the four channels converted by the texture path.  Declared like
// composable_kernel declares its buffer loads, so that the compiler tracks the load's completion itself.
// The same resource over the chain's first texel serves every level of a chain whose levels all start below 4 GiB: the
// load's scalar offset operand takes the level's byte offset (texel_f32's `soffset`), which the range check leaves out.
// Records: the check compares the INDEX alone, so one bound holds for a resource whichever level it is read at -- no
// level has more than 2^30 texels, which is vct_create's bound on voxel_dim (vct_layout.h):
#define VCT_TEXEL_RECORDS 0x40000000
static_assert((unsigned long long)VCT_MAX_VOXEL_DIM * VCT_MAX_VOXEL_DIM * VCT_MAX_VOXEL_DIM <= VCT_TEXEL_RECORDS,
              "the records bound of the texel buffers covers the largest level 0");
__device__ __forceinline__ vct_v4i32 level_texel_buffer(const uint32_t* level_base) {
    const uint64_t a = (uint64_t)level_base;
    vct_v4i32 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    r.y = __builtin_amdgcn_readfirstlane((int)(((uint32_t)(a >> 32) & 0xffffu) | (4u << 16)));     // base[47:32] | stride 4
    r.z = VCT_TEXEL_RECORDS;
    r.w = 0x50fac;                      // DST_SEL x,y,z,w = R,G,B,A | NUM_FORMAT_UNORM << 12 | DATA_FORMAT_8_8_8_8 << 15
    return r;
}
// `soffset`: wave-uniform bytes added to the resource's base (0: the resource starts at the level)
__device__ __forceinline__ float4 texel_f32(vct_v4i32 rsrc, uint32_t index, uint32_t soffset = 0u) {
    const vct_v4f32 v = vct_struct_buffer_load_format_v4f32(rsrc, (int)index, 0, (int)soffset, 0);
    return make_float4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ uint32_t pack_half2(float a, float b) {
    const __half ha = __float2half_rn(a), hb = __float2half_rn(b);
    return (uint32_t)__half_as_ushort(ha) | ((uint32_t)__half_as_ushort(hb) << 16);
}

#endif
