/*
 * vct.h -- C ABI of the MI355X-native voxel-cone-tracing GI path (libvct_amd.so).
 *
 * This is the drop-in boundary.  The reference has no plugin / FFI interface: its boundary is
 * the header-only `struct Voxel_Cone_Tracing` (R/Voxel_Cone_Tracing.h:11-252) that main.cpp
 * calls directly (R/main.cpp:66,68,90).  The C++ facade of the same name in
 * voxel-cone-tracing_amd/host/Voxel_Cone_Tracing.h keeps those member names and forwards to the
 * entry points below; each entry point cites the reference code it replaces
 * (R = Voxel_Cone_Tracing_Final, S = R/Shader).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a
 * negative vct_status; vct_last_error() returns the message of the last failure (per context,
 * or the creation failure when ctx == NULL).  Host pointers are caller-owned; all HBM is
 * context-owned and released by vct_destroy().  One host thread per context, one context per
 * GPU; every kernel runs on the context's HIP stream.  There is no CPU fallback: creation
 * fails if no gfx950 device is usable.
 */
#ifndef VCT_H_
#define VCT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VCT_ABI_VERSION 8

typedef enum vct_status {
    VCT_OK = 0,
    VCT_ERR_INVALID = -1,     /* bad argument / call order */
    VCT_ERR_DEVICE = -2,      /* HIP runtime error (message in vct_last_error) */
    VCT_ERR_NO_DEVICE = -3,   /* no usable GPU */
    VCT_ERR_NOMEM = -4
} vct_status;

/* G-buffer: 23 fp32 planes per pixel (92 B) -- the per-fragment varyings and material fetches of
 * S/VoxelConeTracing.vs:10-15 and S/VoxelConeTracing.fs:3-9,167,209 made explicit. */
enum {
    VCT_GB_POSITION = 0,   /* Position_world xyz            trace.vs:27 */
    VCT_GB_NORMAL = 3,     /* Normal_world xyz (raw)        trace.vs:31 */
    VCT_GB_TANGENT = 6,    /* Tangent_world xyz (raw)       trace.vs:32 */
    VCT_GB_BITANGENT = 9,  /* BiTangent_world xyz (raw)     trace.vs:33 */
    VCT_GB_BUMP_N = 12,    /* bump normal N (unit)          trace.fs:177 */
    VCT_GB_ALBEDO = 15,    /* matColor rgba                 trace.fs:167 */
    VCT_GB_SPECULAR = 19,  /* specColor rgb                 trace.fs:209-210 */
    VCT_GB_SHADOW = 22,    /* shadow_value                  trace.fs:186 */
    VCT_GB_PLANES = 23
};

typedef enum vct_gb_layout {
    VCT_GB_LINEAR = 0,     /* planes[k][y*width + x] */
    VCT_GB_TILED = 1       /* device layout: [tile][plane][64], tile = 8x8 px, lane = (y&7)*8+(x&7),
                              tiles row-major over ceil(w/8) x ceil(h/8) */
} vct_gb_layout;

typedef enum vct_mem {
    VCT_MEM_HOST = 0,
    VCT_MEM_DEVICE = 1
} vct_mem;

/* G-buffer contract (what vct_trace and its kin accept in `planes`; nothing validates it -- a pass over the planes would
 * cost a frame's worth of reads).
 *
 * Position bound.  For every pixel that is not discarded and whose planes 0-5 are finite, on every axis c, evaluated in
 * exact arithmetic with vs = grid_world_size / voxel_dim:
 *     |Position_c| + |Normal_world_c| * vs + config.max_distance <= VCT_GBUFFER_LIMIT_GRIDS * config.grid_world_size.
 * Where the bound comes from: a cone samples the positions p = Position + Normal_world * vs + dir * d with |dir| = 1 and
 * d < max_distance (trace.fs:92,98), the left side bounds |p_c|, and the sampler turns p into the texel coordinate
 * u = (p / G + 0.5) * N - 0.5 of a level of N <= voxel_dim <= 2^10 texels and takes (int)floorf(u) (csrc/vct_trace.hip
 * sample_level, oracle/vct_oracle.cpp tri_sample).  That conversion is only defined for |u| < 2^31 (the GPU saturates,
 * C++ on the host does not: with GL_REPEAT the two would read texel N - 1 and texel 0, with clamp opposite edges):
 * |p_c| / G <= 2^20 gives |u| <= (2^20 + 0.5) * 2^10 + 0.5 < 2^31 with a factor 2 to spare for the fp32 roundings on
 * the way -- the figure of the vertex contract (VCT_VERTEX_LIMIT_GRIDS), here with the cone's reach inside it.  Inside the
 * bound frame, per-cone steps and raw cones are the CPU oracle's; outside it the result of that pixel is unspecified
 * (no address leaves the chain: every texel index is masked or clamped).
 *
 * Otherwise every plane may hold any fp32 value, NaN and +-inf included:
 *   - a tangent frame whose determinant dot(T, B x N) is 0, underflows, overflows or is not finite, a camera position
 *     equal to Position (trace.fs:181 normalises cam - Position) and NaN or infinite inputs give NaN cone directions.
 *     Such a cone takes one step (trace.fs:94 holds once, then its alpha is NaN) and returns NaN; the pixel's rgb is
 *     NaN or inf, ITS rgb only: no other pixel of the frame, of the step counts or of the debug outputs changes.
 *     max(x, 0) in trace.fs:188,213 is C's fmaxf: a NaN dot product gives 0 there.
 *   - albedo.a = NaN counts as NOT discarded: trace.fs:171 discards on `albedo.a < 0.5`, which NaN fails.  The pixel is
 *     traced and its output alpha is NaN.  -0.0 and the float below 0.5 are discarded, 0.5 is not.
 *   - colours and the shadow term are plain factors: negative values, values above 1 and values whose product leaves
 *     fp16 (|x| >= 65520 rounds to inf) are composited as the shader's arithmetic has them.
 *   - lanes of a TILED buffer outside the frame (ragged width / height) may hold anything: they are never read into a
 *     result and never steer the sampler. */
#define VCT_GBUFFER_LIMIT_GRIDS 1048576.0f

typedef struct vct_gbuffer {
    const float* planes;
    int32_t width, height;
    int32_t layout;        /* vct_gb_layout */
    int32_t location;      /* vct_mem */
} vct_gbuffer;

/* Configuration = the reference's compile-time constants and public fields
 * (R/Voxel_Cone_Tracing.h:14-53, S/VoxelConeTracing.fs:43-46), runtime-settable. */
typedef struct vct_config {
    int32_t abi_version;       /* VCT_ABI_VERSION */
    int32_t device;            /* HIP device ordinal; -1 = current device */
    int32_t voxel_dim;         /* VoxelDimensions: power of two in [8,1024]   VCT.h:16 */
    float grid_world_size;     /* VoxelGridWorldSize = 150                     VCT.h:17 */
    int32_t width, height;     /* screen_width/height                          VCT.h:24-25 */
    int32_t shadow_map_size;   /* ShadowMapSize = 4096                         VCT.h:35 */
    float model_scale;         /* ModelMatrix = scale(0.05)                    VCT.h:183,240 */
    float ambient_factor;      /* AmbientFactor = 0.1                          VCT.h:53 */
    float shininess;           /* Shininess = 20                               Mesh.h:86 */
    float max_distance;        /* MAX_DISTANCE = 75                            trace.fs:43 */
    float max_alpha;           /* MAX_ALPHA = 0.95                             trace.fs:44 */
    float tan_diffuse;         /* 0.577                                        trace.fs:198 */
    float tan_specular;        /* 0.07                                         trace.fs:218 */
    int32_t wrap_repeat;       /* 1 = GL_REPEAT (VCT.h:110-113 leaves the GL default) */
    int32_t debug_outputs;     /* 1 = also keep per-cone step counts and raw cone vec4s */
    int32_t trace_variant;     /* 0 = default (cooperative sampler, tile split over 3 waves); A/B variants with
                                  identical results: 1 = per-lane sampler, 2 = one wave per tile.  3 = the default
                                  kernel with a one-multiply unorm8 decode and reciprocal-multiply divisions: NOT
                                  bit-exact (within the 1e-3 frame tolerance), never a default -- it exists to
                                  measure what the exactness costs (bench.py exactness_tax).  4 = the
                                  default kernel over a live-pixel compaction of 16x16 super-tiles (identical
                                  results; experiment, profiles/experiments/README.md) */
    int32_t voxel_attributes;  /* 1 = the voxelizer also keeps per-voxel mean albedo + face normal
                                  (needed by vct_bounce; 24 B/voxel of extra accumulators) */
    int32_t anisotropic_mips;  /* 1 = also keep six directional (pre-integrated) mip chains and sample
                                  levels >= 1 from them by cone direction (north-star option; the
                                  reference has one isotropic chain -- VCT.h:248 -- so the default 0 is
                                  what matches the shader transliteration) */
    int32_t texture_mipmaps;   /* 1 (default) = material textures get mip chains (glGenerateMipmap, Model.h:168) and are
                                  sampled LINEAR_MIPMAP_LINEAR with the implicit derivatives of texture() (Model.h:172;
                                  trace.fs:114-116,167,209, vox.fs:56); 0 = level 0, bilinear (rounds 1-2) */
} vct_config;

typedef struct vct_ctx vct_ctx;

typedef enum vct_voxelize_mode {
    VCT_VOX_CONSERVATIVE_AVG = 0,   /* north-star: conservative overlap + atomic integer average */
    VCT_VOX_REFERENCE = 1           /* S/Voxelization.*: pixel-centre raster, last triangle wins */
} vct_voxelize_mode;

int vct_default_config(vct_config* cfg);

/* Replaces the ctor + resource creation of init_voxel_cone_tracing (VCT.h:57-65,107-126):
 * allocates the brick mip chain (zero-filled, like VCT.h:115-119) and frame buffers in HBM. */
int vct_create(const vct_config* cfg, vct_ctx** out_ctx);
void vct_destroy(vct_ctx* ctx);
const char* vct_last_error(const vct_ctx* ctx);
int vct_get_config(const vct_ctx* ctx, vct_config* cfg);

/* Per-frame uniforms (VCT.h:167-168,171). */
int vct_set_camera_position(vct_ctx* ctx, const float pos[3]);
int vct_set_light_direction(vct_ctx* ctx, const float dir[3]);
int vct_set_ambient_factor(vct_ctx* ctx, float ambient);
int vct_set_cone_apertures(vct_ctx* ctx, float tan_diffuse, float tan_specular);
/* config.trace_variant of the following traces (0 .. 4, see vct_config).  No reference counterpart: the variants are
 * measurement alternatives of the one cone trace of S/VoxelConeTracing.fs:82-107,165-228; 0 is the exact default. */
int vct_set_trace_variant(vct_ctx* ctx, int32_t variant);
/* Footprint records (no reference counterpart; a layout option of the 8^3-brick Morton chain for HBM-bound volumes):
 * on != 0 keeps, beside the chain, one 32-byte record per texel of the levels >= 1 holding the 8 texels of the
 * trilinear footprint anchored there (GL_REPEAT folded in), so that an incoherent (per-lane) level sample is one
 * 32-byte fetch instead of eight 4-byte ones from two to four cache lines.  Costs 8 x the bytes of those levels
 * (1.14 x level 0: 77 MB at 256^3, 4.9 GB at 1024^3) and a dense rebuild after every mip build.  Same frame, bit for
 * bit.  Pays where the chain does not fit the caches (dense random 1024^3 chain: trace 5.61 -> 2.86 ms); a scene that
 * touches a thin shell of its grid stays cache-resident and gains nothing (street at 1024^3 / 4K: 2.72 -> 2.70 ms).
 * Default off (VCT_FOOTPRINT_RECORDS=1 in the environment turns it on at vct_create).  The clamp-to-edge sampler,
 * the anisotropic chains and the second-bounce chain keep per-texel gathers. */
int vct_set_footprint_records(vct_ctx* ctx, int32_t on);

/* Scene upload -- replaces Model/Mesh VBO setup (R/Mesh.h:49-82) for the two attributes the
 * voxelizer reads (vox.vs:3-4).  pos: [ntri][3][3] model-space fp32; material: [ntri];
 * albedo: [nmat][4] flat per-material albedo (stands in for DiffuseTexture, vox.fs:56).
 *
 * Vertex contract.  Every coordinate v of pos must be finite and satisfy, with the product formed in fp32,
 *     |v * config.model_scale| <= VCT_VERTEX_LIMIT_GRIDS * config.grid_world_size        (2^20 grid widths).
 * Where the bound comes from: the voxelizer turns a scaled coordinate x into the voxel coordinate
 * g = (x / G + 0.5) * V and takes (int)floorf(g) for its bounding boxes before clamping to the grid (csrc/vct_voxelize.hip
 * setup_tri, ref_setup).  That conversion is only defined for |g| < 2^31 (the GPU saturates, C++ on the host does
 * not), and V <= 1024 = 2^10: |x| / G <= 2^20 gives |g| <= (2^20 + 0.5) * 2^10 < 2^31 with a factor 2 to spare for
 * the fp32 roundings on the way.  Inside the bound every stage (voxelizer, shadow and G-buffer raster) computes,
 * bit for bit, what the CPU checkers of oracle/ compute; a mesh outside it is refused here with VCT_ERR_INVALID and
 * a message (vct_last_error), and the context keeps the mesh it had.  The raster stages have no bound of their own
 * on the vertices: their integer conversions happen after the near clip, on doubles, are clamped to the frame, and
 * saturate, for any finite clip coordinates the caller's matrix produces from an in-contract vertex. */
#define VCT_VERTEX_LIMIT_GRIDS 1048576.0f
int vct_upload_triangles(vct_ctx* ctx, const float* pos, const int32_t* material, int32_t ntri,
                         const float* albedo, int32_t nmat);
/* Shadow map produced by the depth pass (VCT.h:192-211): size*size fp32 depths in [0,1] plus the
 * column-major DepthViewProjectionMatrix (VCT.h:84-86).  depth == NULL detaches it (PCF = 1). */
int vct_upload_shadow_map(vct_ctx* ctx, const float* depth, int32_t size, const float light_vp[16]);

/* ---- raster input stages on the GPU ------------------------------------------
 * Per-vertex frame of the uploaded triangles (R/Mesh.h:12-19 normal / tangent / bitangent, attribs
 * 1,3,4 of S/VoxelConeTracing.vs) and the per-material specular colour (trace.fs:209): normal,
 * tangent, bitangent [ntri][3][3] model space, specular [nmat][3].  Call after vct_upload_triangles. */
int vct_upload_mesh_attributes(vct_ctx* ctx, const float* normal, const float* tangent,
                               const float* bitangent, const float* specular);
/* Texture coordinates of the uploaded triangles (attribute 2, R/Mesh.h:72-73): uv [ntri][3][2]. */
int vct_upload_mesh_uvs(vct_ctx* ctx, const float* uv);
/* Material textures (R/Model.h:126-136,141-226; bound per draw at R/Mesh.h:91-108): ntex RGBA8 images
 * (rgba8[i]: height[i] * width[i] * 4 bytes, row 0 at v = 0) and, per material, the index of its
 * DiffuseTexture / SpecularTexture / HeightTexture or -1 (mat_tex [nmat][3]; -1 keeps the flat colour of
 * vct_upload_triangles / vct_upload_mesh_attributes, resp. a flat height map).  texture(sampler, uv) is
 * restated as GL_REPEAT, mip-mapped (config.texture_mipmaps: box-filtered chain built on the GPU at upload,
 * LINEAR_MIPMAP_LINEAR / LINEAR, lambda from the differences of uv inside the fragment's 2x2 quad; the rules an
 * OpenGL implementation is free to choose are written down in oracle/vct_oracle.h) or level 0 bilinear.  Used by
 * vct_voxelize (albedo fetch, vox.fs:56) and vct_render_gbuffer (matColor + alpha test trace.fs:167-172,
 * CalcBumpNormal :110-128, specColor :209-210) once vct_upload_mesh_uvs has been called too.  ntex = 0
 * detaches them.  Call after vct_upload_triangles. */
int vct_upload_textures(vct_ctx* ctx, const uint8_t* const* rgba8, const int32_t* width, const int32_t* height,
                        int32_t ntex, const int32_t* mat_tex);
/* DrawDepthTexture (VCT.h:192-211, S/Shadow.vs/.fs): rasterises the uploaded triangles from the light
 * (column-major DepthViewProjectionMatrix, VCT.h:84-86) into the context's shadow map of
 * config.shadow_map_size^2 24-bit depths -- the map vct_voxelize and vct_render_gbuffer then read. */
int vct_render_shadow_map(vct_ctx* ctx, const float light_vp[16]);
int vct_download_shadow_map(vct_ctx* ctx, float* depth);
/* The vertex + fixed-function part of Render (VCT.h:161-189, S/VoxelConeTracing.vs, depth test LESS,
 * back faces culled) and the non-cone per-fragment inputs of S/VoxelConeTracing.fs (bump normal,
 * material colours, PCF shadow term): fills the resident tiled G-buffer from the uploaded mesh for
 * the column-major view-projection matrix (VCT.h:161-163).  Follow with vct_trace_resident or
 * vct_trace_current. */
int vct_render_gbuffer(vct_ctx* ctx, const float view_proj[16]);
/* The same for tile rows [tile_row0, tile_row1) only (scissored raster + shading of those tiles): what a
 * multi-GPU rank runs for its slab.  Other rows of the resident G-buffer keep their old content. */
int vct_render_gbuffer_rows(vct_ctx* ctx, const float view_proj[16], int32_t tile_row0, int32_t tile_row1);
/* Linear planes [23][h*w] of the resident G-buffer. */
int vct_download_gbuffer(vct_ctx* ctx, float* planes);
/* Trace the resident G-buffer (vct_render_gbuffer, or the last vct_trace upload) and return the frame
 * like vct_trace. */
int vct_trace_current(vct_ctx* ctx, void* out_rgba16f, int32_t out_location);

/* DrawVoxelTexture (VCT.h:213-245) -> vox.vs / vox.gs / vox.fs: voxelize the uploaded triangles
 * into per-voxel integer accumulators (mode selects coverage + resolve rule).  In the north-star mode only the light
 * is evaluated per pass: the fragment list, every fragment's barycentrics and -- with textures -- its albedo depend on
 * mesh, grid and textures alone and are kept per context (12-24 B per fragment); the first pass after
 * vct_upload_mesh_uvs / vct_upload_textures rebuilds the albedo (and may return VCT_ERR_NOMEM for it). */
int vct_voxelize(vct_ctx* ctx, int32_t mode);
/* vox.fs:88: resolve the accumulators into radiance level 0 (rgb = albedo * PCF shadow, a = 1). */
int vct_inject_light(vct_ctx* ctx);
/* glGenerateMipmap (VCT.h:126,248): 2x2x2 box, requantised per level, over the brick chain. */
int vct_build_mips(vct_ctx* ctx);

/* Second bounce (north-star, BASELINE.json config 3; the reference's README claims 2 bounces but its
 * code injects once -- VCT.h:138-139 -- so the definition is this build's, oracle/vct_oracle.h):
 * every occupied voxel gathers 6 diffuse cones from the current (bounce-0) chain along its stored
 * normal and adds albedo * occlusion-weighted irradiance; the result becomes level 0 of a second
 * chain, its mips are built, and vct_trace reads that chain until the next vct_inject_light.
 * Needs config.voxel_attributes = 1 and vct_voxelize + vct_inject_light + vct_build_mips first. */
int vct_bounce(vct_ctx* ctx);
/* Per-voxel attributes of the last resolve (config.voxel_attributes = 1): V^3 * 4 bytes each, linear
 * voxel order; albedo rgb (a = 255 where occupied), normal xyz biased by +128 (w = 255 where occupied). */
int vct_download_voxel_attributes(vct_ctx* ctx, uint8_t* albedo, uint8_t* normal);

/* Volumes built elsewhere (fixtures, oracle-built volumes).  Linear layout: level k has
 * N = V>>k texels per side, texel (x,y,z) at ((z*N+y)*N+x)*4, levels concatenated. */
int vct_upload_volume_rgba8(vct_ctx* ctx, const uint8_t* level0_linear);
int vct_upload_chain_rgba8(vct_ctx* ctx, const uint8_t* chain_linear);
int vct_download_chain_rgba8(vct_ctx* ctx, uint8_t* chain_linear);
/* config.anisotropic_mips = 1: the six directional chains built by the last vct_build_mips / vct_bounce,
 * [6][chain_texels - V^3][4] bytes, direction = 2*axis + (0: towards +axis, 1: towards -axis), level k
 * of a direction at texel offset level_offset(k) - V^3, linear layout. */
int vct_download_aniso_rgba8(vct_ctx* ctx, uint8_t* aniso_linear);
size_t vct_chain_texels(int32_t voxel_dim);

/* Render (VCT.h:146-190) -> trace.fs:165-228.  Traces the G-buffer through the brick chain and
 * writes the frame as RGBA16F, row-major width*height*4 halves (8 B / px).  out location follows
 * out_location (vct_mem).  A HOST G-buffer is uploaded (and tiled) first. */
int vct_trace(vct_ctx* ctx, const vct_gbuffer* gb, void* out_rgba16f, int32_t out_location);
/* Screen-tile slab [tile_row0, tile_row1) of the same frame (multi-GPU sharding): only those
 * 8-pixel tile rows are traced; out addresses the full frame and only the slab's rows are
 * written. */
int vct_trace_slab(vct_ctx* ctx, const vct_gbuffer* gb, int32_t tile_row0, int32_t tile_row1,
                   void* out_rgba16f, int32_t out_location);
/* Re-run the trace kernel on the G-buffer already resident from the last vct_trace (no upload,
 * no download); used for timing.  stream work only, asynchronous. */
int vct_trace_resident(vct_ctx* ctx);
/* Same for the tile-row slab [tile_row0, tile_row1) of the resident G-buffer; later
 * vct_trace_resident calls repeat this slab. */
int vct_trace_resident_rows(vct_ctx* ctx, int32_t tile_row0, int32_t tile_row1);
/* every `stride`-th tile row of [tile_row0, tile_row1), starting with tile_row0 (the rows rank tile_row0 of `stride`
 * ranks traces under interleaved slabs, vct_comm_set_interleaved); the pixels land at their own place in the frame.
 * (No reference counterpart: the reference draws one full-screen quad on one GPU, R/main.cpp:77-94.) */
int vct_trace_resident_strided(vct_ctx* ctx, int32_t tile_row0, int32_t tile_row1, int32_t stride);
/* One whole GI pass for a light AND a camera that moved -- init_voxel_cone_tracing's DrawDepthTexture +
 * DrawVoxelTexture (VCT.h:138-139) followed by Render (VCT.h:146-190) -- issued as one call:
 *   { shadow map -> voxelize(mode) -> inject -> mips }  ||  { G-buffer visibility -> (shadow map ready) -> shade }  -> trace.
 * The main draw's visibility raster needs nothing of this pass and its shading kernel only READS the shadow map, so
 * the G-buffer stage runs on a second HIP stream beside the shadow pass and the voxel stages (none of them fills the
 * GPU on its own; the two raster passes have their own work lists); the trace waits for both.  The
 * frame is bit-identical to vct_render_shadow_map, vct_voxelize, vct_inject_light, vct_build_mips,
 * vct_render_gbuffer, vct_trace_resident called in that order.  Asynchronous (vct_synchronize).
 * On a rank of a multi-GPU frame (after vct_comm_init) the same call runs the rank's share: the G-buffer stream is
 * scissored to the rank's slab (vct_render_gbuffer_rows) and the pass ends with vct_frame_step -- slab trace + the
 * frame's one gather -- instead of the full-frame trace; collective like vct_frame_step (vct_comm_sync to wait). */
int vct_gi_pass(vct_ctx* ctx, const float light_vp[16], const float view_proj[16], int32_t voxelize_mode);
/* Redirect the trace kernel's RGBA16F output to caller-owned HBM (full-frame addressing: pixel (x,y)
 * at ((y*width + x) * 4) halves from `rgba16f_dev`); NULL restores the context-owned frame.  A slab
 * rank passes its gather buffer minus the slab's first row so the kernel writes the gather buffer
 * directly (no device-to-device copy per frame).  The caller keeps the memory alive. */
int vct_set_frame_target(vct_ctx* ctx, void* rgba16f_dev);
/* Host copy of the frame the trace kernels write (the context-owned frame, or the target set above with
 * full-frame addressing): width*height*4 halves.  Rows no trace has written keep their old content. */
int vct_download_frame(vct_ctx* ctx, void* out_rgba16f_host);
int vct_synchronize(vct_ctx* ctx);

/* ---- lighting components and per-component outputs --------------------------------------------------
 * The reference's orchestrator declares ShowDiffuse, ShowIndirectDiffuse, ShowSpecular, ShowIndirectSpecular and
 * ShowAmbientOcclusion (R/Voxel_Cone_Tracing.h:51), the shader the matching uniforms (S/VoxelConeTracing.fs:36-39)
 * and the ternaries that would apply them (fs:190,203,215, commented out there).  Here the mask applies them; with
 * ind = the weighted 6-cone gather (fs:194-199) and sc = the specular cone (fs:218) the composite (fs:188-227) is
 *   dd   = SHOW_DIFFUSE           ? shadow * cos_theta : 0       fs:190
 *   occ  = SHOW_AMBIENT_OCCLUSION ? 1 - ind.a          : 1       fs:201
 *   ird  = SHOW_INDIRECT_DIFFUSE  ? ind.rgb            : 0       fs:203 (after occlusion is formed)
 *   D    = (dd + occ * ird) * albedo.rgb                         fs:205
 *   ds   = SHOW_SPECULAR          ? spec * shadow      : 0       fs:215
 *   socc = SHOW_AMBIENT_OCCLUSION ? 1 - sc.a           : 1       fs:221
 *   irs  = SHOW_INDIRECT_SPECULAR ? sc.rgb             : 0       (the rule of fs:203)
 *   S    = (irs + socc * ds) * specColor.rgb                     fs:223
 *   A    = ambient * albedo.rgb * occ                            fs:225
 *   out  = (A + D + S, albedo.a)                                 fs:227; discarded pixels keep the clear colour
 * VCT_SHOW_ALL (the default) is the unmasked arithmetic in the same order: the same bits as before the mask existed.
 * A cone group is marched only when something reads it: the six diffuse cones when INDIRECT_DIFFUSE or
 * AMBIENT_OCCLUSION is shown or the indirect-diffuse output is on; the specular cone when INDIRECT_SPECULAR is shown,
 * or AMBIENT_OCCLUSION and SPECULAR both are, or the indirect-specular output is on.  A skipped cone adds no steps
 * to the step counts and leaves 0 steps and a zero vec4 in the debug outputs.
 * The mask is host state like the ambient factor: it applies from the next trace launch of any kind on (screen
 * traces, resident traces, the GI pass, a rank's frame step).  Bits above VCT_SHOW_ALL are VCT_ERR_INVALID, and so
 * is a mask other than VCT_SHOW_ALL with config.trace_variant 1 .. 4 (measurement kernels without the mask). */
enum {
    VCT_SHOW_DIFFUSE = 1,
    VCT_SHOW_INDIRECT_DIFFUSE = 2,
    VCT_SHOW_SPECULAR = 4,
    VCT_SHOW_INDIRECT_SPECULAR = 8,
    VCT_SHOW_AMBIENT_OCCLUSION = 16,
    VCT_SHOW_ALL = 31
};
int vct_set_lighting_components(vct_ctx* ctx, uint32_t mask);
int vct_get_lighting_components(const vct_ctx* ctx, uint32_t* mask);

/* Per-component outputs (no reference counterpart; for renderers that denoise, accumulate or composite the GI terms
 * apart): RGBA16F full frames beside the frame, same addressing and the same f32 -> f16 rounding, raw values (the
 * mask does not change them):
 *   VCT_AOV_INDIRECT_DIFFUSE   inDirectDiffuse of fs:194-199 (the weighted gather of cones 0..5, rgba)
 *   VCT_AOV_INDIRECT_SPECULAR  inDirectSpecular of fs:218 (the specular cone, rgba)
 *   VCT_AOV_DIRECT             (shadow * cos_theta, spec * shadow, shadow, 1)
 * Discarded pixels (albedo.a < 0.5) are (0,0,0,0) in every output; rows no trace has written keep their old
 * content.  The set call allocates (which = 0: frees) the requested buffers for every frame slot, so launches
 * allocate nothing; a second frame slot gets its own set.  Refused (VCT_ERR_INVALID) with config.trace_variant
 * 1 .. 4 and on a context of a multi-GPU frame (after the communicator's init: outputs are not gathered). */
enum {
    VCT_AOV_INDIRECT_DIFFUSE = 1,
    VCT_AOV_INDIRECT_SPECULAR = 2,
    VCT_AOV_DIRECT = 4
};
int vct_set_aov_outputs(vct_ctx* ctx, uint32_t which);
/* One output of the selected frame slot (one_bit: exactly one VCT_AOV_* bit): a host copy of width*height*4 halves
 * (waits for the slot's stream), or its device pointer and size for zero-copy consumers. */
int vct_download_aov(vct_ctx* ctx, uint32_t one_bit, void* out_rgba16f_host);
int vct_get_aov_device(vct_ctx* ctx, uint32_t one_bit, void** rgba16f_dev, size_t* bytes);

/* ---- half-rate diffuse gather -------------------------------------------------------------------------
 * No reference counterpart (S/VoxelConeTracing.fs:194-199 marches the six diffuse cones of every fragment), so the
 * definition is this build's.  The six diffuse cones are most of a frame's steps, their aperture is 60 degrees and they
 * start one voxel off the surface: their gather varies slowly over a surface.  rate = 2 marches them for one pixel per
 * 2x2 quad and reconstructs the others with a depth- and normal-aware filter; rate = 1 (default) is the trace as it was,
 * bit for bit.  The specular cone stays at full rate.  Rate 2, all of it fp32, plain multiplies, adds and compares in
 * the written order, nothing fused, one IEEE division at the end:
 *   Coarse grid  cw = ceil(w / 2) by ch = ceil(h / 2); coarse sample (cx, cy) covers the pixels (2 cx + i, 2 cy + j).
 *   Anchor       of a quad: the first pixel in the order (0,0), (1,0), (0,1), (1,1) = (i, j) that is inside the frame
 *                and not discarded (albedo.a >= 0.5).  No such pixel: no sample.  The anchor's six cones are marched as
 *                rate 1 marches them for that pixel and ind is their gather (fs:194-199): the same bits as at rate 1.
 *   Candidates   of a live pixel p = (x, y) that is no anchor, in this order, with integer weights:
 *                  0  its own quad (x >> 1, y >> 1)                                   9
 *                  1  the horizontal neighbour, (x >> 1) + (x & 1 ? +1 : -1)          3
 *                  2  the vertical neighbour, chosen the same way in y                3
 *                  3  the diagonal of the two                                         1
 *                A candidate outside the coarse grid or without a sample is rejected.
 *   Acceptance   with n_p, n_k the raw VCT_GB_NORMAL planes of p and of candidate k's anchor, P_p, P_k their positions,
 *                vs = grid_world_size / voxel_dim, dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z and
 *                  dn = dot(n_p, n_k)   d = dot(P_k - P_p, n_p)   l_p = dot(n_p, n_p)   l_k = dot(n_k, n_k):
 *                  dn > 0
 *                  dn*dn >= VCT_DIFFUSE_RATE_NORMAL_COS2 * (l_p * l_k)                 normals within ~25.7 degrees
 *                  d*d  <= (VCT_DIFFUSE_RATE_PLANE_TOL * (vs*vs)) * l_p                anchor within vs / 2 of p's tangent plane
 *   Interpolate  w_k = the weight of an accepted candidate, else 0; W = sum w_k (0 .. 16).  W > 0: per channel
 *                  S = ((w_0*I_0 + w_1*I_1) + w_2*I_2) + w_3*I_3   (a rejected term is +0),   ind_p = S / (float)W.
 *   Fill         W == 0: p marches its own six cones, like an anchor.
 * The composite above runs per pixel with ind_p in place of the pixel's own gather; VCT_AOV_INDIRECT_DIFFUSE holds
 * ind_p.  The skip rule is unchanged: when nothing reads the diffuse group, no coarse or fill cone is marched.
 * vct_set_diffuse_rate is host state like the lighting mask: it applies from the next vct_trace, vct_trace_current,
 * vct_trace_resident (at rate 2: the whole frame) or vct_gi_pass on.  Rate 2 allocates its buffers (24 B per pixel +
 * 17 B per quad) for every frame slot and rate 1 frees them, so launches allocate nothing.  VCT_ERR_INVALID: a rate
 * other than 1 or 2; rate 2 with config.trace_variant 1 .. 4, config.anisotropic_mips, footprint records or on a context of
 * a multi-GPU frame (and each of those while rate 2 is set); at rate 2 vct_trace_slab, vct_trace_resident_rows,
 * vct_trace_resident_strided and vct_last_row_steps.  vct_last_step_count counts every executed step (coarse, fill,
 * specular), vct_last_trace_ms brackets all launches of the pass.  With config.debug_outputs, steps and cones 0..5 of
 * a pixel hold its own march if it is an anchor or a fill pixel and zeros if it was interpolated.
 * vct_get_diffuse_rate (either pointer may be NULL): the rate, and the pixels whose diffuse cones the selected slot's last
 * trace marched (anchors + fill pixels; 0 after a rate-1 trace or when the group was skipped).  Waits for the slot's stream. */
#define VCT_DIFFUSE_RATE_NORMAL_COS2 0.8125f    /* 13/16 */
#define VCT_DIFFUSE_RATE_PLANE_TOL 0.25f        /* (1/2)^2 */
int vct_set_diffuse_rate(vct_ctx* ctx, int32_t rate);
int vct_get_diffuse_rate(const vct_ctx* ctx, int32_t* rate, uint64_t* marched_pixels);
/* Device time of the four launches of the selected slot's last rate-2 pass -- coarse march, resolve, fill march, specular
 * trace + composite -- in milliseconds.  Needs trace timing on (vct_set_trace_timing) and a pass that marched the
 * diffuse group; waits for it. */
int vct_last_diffuse_rate_ms(vct_ctx* ctx, float ms[4]);

/* ---- voxel view -----------------------------------------------------------------------------------------
 * No reference counterpart (the reference has no way to look at its VoxelTexture), so the definition is this build's.
 * Every pixel's ray is walked cell by cell through ONE level of a chain -- or through a per-voxel attribute -- and
 * composited front to back with the march's own rule (S/VoxelConeTracing.fs:100,102): at level 0 of an injected chain
 * alpha is 0 or 1 and the view shows the first occupied voxel, at coarse levels it shows what the cones see.  It is how
 * one picks grid_world_size and voxel_dim, sees light leaking through thin walls, a mesh falling out of the grid, a
 * bounce that did nothing or a level that has gone opaque -- without a 4.57 GiB download at 1024^3.
 * All of it fp32, multiplies, adds and compares in the written order, nothing fused, IEEE divisions.  w x h the frame,
 * V the grid, L the level, N = V >> L, G = grid_world_size, m = inv_view_proj (column-major), row 0 the bottom row:
 *   Ray      of pixel (x, y): nx = (2 (x + 0.5)) / w - 1, ny likewise with h; for nz = -1 and nz = +1
 *              r_i = ((m[i] nx + m[4 + i] ny) + m[8 + i] nz) + m[12 + i],  i = 0 .. 3,     point = r_xyz / r_w.
 *            o = the near point (nz = -1), d = far - near (not normalised).  A non-finite o or d, or d = 0: a miss.
 *   Grid     units: g_a = (o_a / G + 0.5) N,  e_a = (d_a / G) N,  inv_a = 1 / e_a where e_a != 0.
 *   Entry    per axis with e_a != 0 the pair (0 - g_a) inv_a, (N - g_a) inv_a, smaller first; t_in = max(0, the smaller
 *            ones), t_out = min(the larger ones) -- folded over x, y, z in that order from 0 and +inf, each step keeping
 *            what it has unless the next value compares greater (smaller).  An axis with e_a = 0 gives no pair and is a
 *            miss unless 0 <= g_a < N.  A miss unless t_in < t_out.
 *            Start cell c_a = (int)min(max(floor(g_a + t_in e_a), 0), N - 1), the clamps taken on the float.
 *   Walk     the next plane of axis a is b_a = c_a + (e_a > 0 ? 1 : 0) and its parameter t_a = ((float)b_a - g_a) inv_a
 *            (+inf for e_a = 0): a function of the integer plane index alone, never accumulated.  Visit the cell; step
 *            the axis with the smallest t_a by +1 (e_a > 0) or -1 (start with x; y replaces it if t_y < t_x; z replaces
 *            that if t_z is smaller still: ties go x before y before z); stop when the cell leaves [0, N)^3.
 *   Visit    T = the texel of cell (c_x, c_y, c_z), each byte c as c / 255.0f;  oma = 1 - A;
 *            C_rgb = C_rgb + oma T_rgb;  A = A + oma T_a;  stop after a visit that leaves A >= config.max_alpha.
 *            (A texel with alpha 0 and rgb != 0 -- uploaded volumes can hold them -- still adds its colour.)
 *   Output   (C_r, C_g, C_b, A) from C = 0, A = 0; a miss is (0, 0, 0, 0).
 * The kernel skips empty space and still writes this frame bit for bit.  A zero parent texel proves nothing about its
 * children (the mips requantise) and the voxelizer's brick flags know nothing of uploaded chains, so it keeps one bit per
 * 8^3 block of the viewed level, "some texel word != 0" (a 64-bit word per 32^3 region: 256 KiB at 1024^3), rebuilt by
 * a small kernel in front of the first view after the chain or the attributes changed; inside an empty block it walks
 * the cells with no fetch.  VCT_VOXVIEW_SKIP=0 in the environment takes the instantiation without it (A/B).
 * vct_render_voxels writes the selected frame slot's RGBA16F frame -- same addressing and f32 -> f16 rounding as the
 * trace, vct_set_frame_target honoured -- so vct_download_frame and vct_get_frame_device show it.  Asynchronous on the
 * slot's stream; ordered against the stages that write the chain exactly as a resident trace is (it reads shared state
 * and writes slot state only: the frame and the slot's occupancy words).  It leaves the G-buffer, the step counts, the
 * per-component outputs and vct_last_trace_ms alone, works with every config.trace_variant, with two frame slots, with
 * config.anisotropic_mips (it shows the isotropic chain) and with footprint records (it ignores them).
 * inv_view_proj: the column-major fp32 inverse of the matrix vct_render_gbuffer takes (the caller inverts; the facade
 * and the Python binding invert in double and round once).
 * VCT_ERR_INVALID: a NULL context or matrix; a non-finite matrix element; an unknown source; a level outside
 * [0, levels); ALBEDO / NORMAL without config.voxel_attributes, with level != 0 or before a mesh was uploaded; a level
 * >= 1 of a chain whose level 0 changed since the last vct_build_mips (the rule of the trace); a context of a multi-GPU
 * frame. */
enum {
    VCT_VOXVIEW_CURRENT = 0,    /* the chain the trace reads now (the bounce chain after vct_bounce, else radiance) */
    VCT_VOXVIEW_RADIANCE = 1,   /* the bounce-0 radiance chain, whatever the trace reads */
    VCT_VOXVIEW_ALBEDO = 2,     /* per-voxel mean albedo   (config.voxel_attributes = 1, level 0 only) */
    VCT_VOXVIEW_NORMAL = 3      /* per-voxel biased normal (config.voxel_attributes = 1, level 0 only) */
};
int vct_render_voxels(vct_ctx* ctx, const float inv_view_proj[16], int32_t source, int32_t level);
/* Device time of the walk kernel of the selected slot's last view in milliseconds (the occupancy rebuild, when one was
 * due, runs in front of the bracket).  Needs trace timing on (vct_set_trace_timing) when the view was issued; waits. */
int vct_last_voxel_view_ms(vct_ctx* ctx, float* ms);

/* ---- point queries: gathers and single cones at caller-given points ------------------------------------------
 * No reference counterpart (the reference lights only what its one camera sees).  What light arrives at a point that is
 * no pixel of the G-buffer -- a light probe, a lightmap texel, a particle, another camera's reflection point, a caller's
 * own AO cone -- is the march of S/VoxelConeTracing.fs with the point's values in place of the fragment's:
 *   Gather  (vct_gather_points) point i is a fragment with Position_world = position, Normal_world = normal (as planes
 *           3-5 hold it: model-scaled, not normalised), Tangent_world = tangent, BiTangent_world = bitangent.
 *           out_gather[i] = the vec4 inDirectDiffuse of fs:194-199 before fs:201: the frame of fs:175
 *           (inverse(transpose(mat3(T, B, N))), as the screen trace forms it), six Voxel_Cone_Tracing calls at
 *           config.tan_diffuse along normalize(frame * ConeVectors[k]), folded as ind = fma(Weights[k], cone_k, ind)
 *           over k = 0 .. 5 from 0.  out_cones[i][k] / out_steps[i][k] (either may be NULL): the six raw vec4s and their
 *           executed step counts, as vct_download_cones / vct_download_steps hold columns 0-5 of a pixel.
 *   Cone    (vct_cone_points) out_cone[i] = Voxel_Cone_Tracing(direction, tan) of fs:82-107 with
 *           startPos = position + normal * voxelWorldSize (fs:92) and tan = config.tan_diffuse (aperture 0) or
 *           config.tan_specular (aperture 1), the two apertures of vct_set_cone_apertures and their step tables.
 *           direction is used as given: normalising is the caller's job (fs:196,217 normalise before the call).
 * Bit for bit what the CPU oracle computes for the same values, and what the screen trace computes for a pixel that holds
 * them.  A query reads the chain the trace reads at that moment (GL_REPEAT or clamp; the bounce chain after vct_bounce)
 * and always takes the exact march: config.trace_variant does not apply, footprint records are not used (same bits).
 * Point contract: the G-buffer contract restated.  Per axis c, in exact arithmetic, vs = grid_world_size / voxel_dim,
 *     |position_c| + |normal_c| * vs + config.max_distance * max(1, |direction|) <= VCT_GBUFFER_LIMIT_GRIDS * grid_world_size
 * (|direction| = 1 for a gather).  Otherwise every field may hold any fp32 value: a point whose start or direction is
 * not finite (NaN or inf fields, a tangent frame with determinant 0) gets the oracle's result -- one step, NaN -- and
 * changes no other point; no address is formed from a coordinate that was not masked or clamped.
 * pts and every out pointer live where `location` (vct_mem) says and need 4-byte alignment only.  VCT_MEM_DEVICE: the
 * work is queued on the selected frame slot's stream and the call returns at once (vct_synchronize); the memory must stay
 * valid until then.  VCT_MEM_HOST: the call returns when the outputs are written.  A query reads shared state only, so
 * with two frame slots it is ordered against the stages that write the chain exactly as a resident trace is.
 * flags: VCT_QUERY_SORT_CELLS -- results are a pure function of each point, so the library may march the points in any
 * order: with the flag it marches them ordered by the 4-voxel cell of their start point (non-finite points last) and
 * writes every result at the caller's index.  Same outputs, bit for bit; it pays when neighbouring points are far apart
 * in the list (a shuffled lightmap, particles), because 64 consecutive points share their texel fetches only when
 * they are neighbours in space.  Points already in spatial order (probe grids, lightmap rows) need no flag.
 * n = 0 succeeds and does nothing.  VCT_ERR_INVALID, nothing touched: n < 0 or n > VCT_POINT_QUERY_MAX; NULL pts or
 * out_gather / out_cone with n > 0; a location or aperture that is not one of the above; unknown flag bits; step counts
 * wanted with an aperture of more than 255 steps; config.anisotropic_mips (out of scope: queries read the isotropic chain
 * only); a chain whose level 0 changed since the last vct_build_mips (the rule of the trace). */
typedef struct vct_gather_point { float position[3], normal[3], tangent[3], bitangent[3]; } vct_gather_point; /* 48 B */
typedef struct vct_cone_point { float position[3], normal[3], direction[3]; } vct_cone_point;                 /* 36 B */
#define VCT_QUERY_SORT_CELLS 1u
#define VCT_POINT_QUERY_MAX (1 << 26)
int vct_gather_points(vct_ctx* ctx, const vct_gather_point* pts, int32_t n, int32_t location, float* out_gather,
                      float* out_cones, uint8_t* out_steps, uint32_t flags);
int vct_cone_points(vct_ctx* ctx, const vct_cone_point* pts, int32_t n, int32_t location, int32_t aperture,
                    float* out_cone, uint8_t* out_steps, uint32_t flags);
/* The selected slot's last query: out[0] points, out[1] executed steps, out[2] kind (0 gather, 1 cone), out[3] 1 if the
 * points were marched in sorted order.  Waits for the slot's stream. */
int vct_last_point_query(vct_ctx* ctx, uint64_t out[4]);
/* Device time of that query's march kernel alone (not the sort, not the copies) in milliseconds, from the library's
 * events; needs trace timing on (vct_set_trace_timing) when the query was issued and n > 0.  Waits for it. */
int vct_last_point_query_ms(vct_ctx* ctx, float* ms);

/* ---- emissive materials: area lights in the voxel chain and the frame -------------------------------------------------
 * No reference counterpart (the reference's only light is the directional one behind the shadow map: S/Voxelization.fs:88
 * stores albedo * PCF, S/VoxelConeTracing.fs:188-227 adds ambient + direct + cones), so the definition is this build's.
 * A surface that emits is written into radiance level 0 and becomes an area light for everything that reads the chain --
 * screen trace, half-rate gather, vct_bounce, voxel view, point queries, anisotropic chains, footprint records, all
 * unchanged -- and is added to the frame for the pixels that see it.
 *   Material emission  emission[nmat][3], fp32 RGB, one per material of the uploaded mesh; flat (no emission textures).
 *   Level 0            (VCT_VOX_CONSERVATIVE_AVG) for a voxel with at least one conservative fragment:
 *                        L  = the texel the voxelizer produces without emission: the rounded mean of
 *                             unorm8(albedo * PCF / 25) over the voxel's fragments;
 *                        Em = the same rounded mean over the same fragments of unorm8(emission[material] * 1.0f): no shadow
 *                             term, no texture; the clamping float -> unorm8 conversion saturates values above 1;
 *                        texel.rgb = min(255, L.rgb + Em.rgb) per byte, texel.a = 255.
 *                      Voxels without fragments stay 0.  The two terms are quantised apart and added with saturation -- not
 *                      unorm8(albedo * shadow + emission) -- because Em depends on neither the light, the shadow map nor
 *                      the textures: like the fragments' barycentrics it is computed once per (mesh, table), into an
 *                      EMISSION POOL of one staged RGBA8 brick (2 KiB) per brick slot, by the voxelize pass's own kernel
 *                      with the table in place of the albedo; vct_inject_light adds the pool's brick to every brick it
 *                      copies (one more coalesced 2 KiB read per touched brick).  The voxel attributes are unchanged.
 *   Frame              every frame slot has three fp32 PIXEL-EMISSION PLANES E[3][h*w].  For a pixel that is not discarded
 *                      out.rgb = ((A + D) + S) + E: one fp32 add per channel, last, A, D, S formed as above; out.a, discarded
 *                      pixels (clear colour) and the per-component outputs are unchanged; the VCT_SHOW_* mask does not gate
 *                      E.  E may hold any fp32 value: a NaN changes its own pixel's rgb only.  No planes: no add, the
 *                      frame as it was, bit for bit (and the trace kernels without lighting components are launched).
 * vct_upload_emission: call after vct_upload_triangles, with the nmat of that call.  NULL detaches, so does a new
 * vct_upload_triangles, and so does a table whose values are all zero: no pool, no planes, no cost.  VCT_ERR_INVALID,
 * the context keeping the table it had: no mesh uploaded; a value that is NaN, infinite or below 0; config.trace_variant
 * 1 .. 4 (the rule of the lighting components: those kernels have no planes; and vct_set_trace_variant refuses 1 .. 4
 * while planes are attached).  Allocates the pool (2 KiB per brick slot) and zeroed planes (12 B per pixel) for every
 * frame slot -- a later second slot gets its own -- so that a launch allocates nothing; a detach frees them.  It takes effect
 * with the next vct_voxelize + vct_inject_light (+ vct_build_mips), exactly as a moved light does ("level 0 changed since
 * the last vct_build_mips" applies unchanged); a pass voxelized before a detach and injected after it is injected without
 * emission.  vct_voxelize(ctx, VCT_VOX_REFERENCE) with emission attached is VCT_ERR_INVALID: that mode is the shaders as
 * written.  With emission attached vct_render_gbuffer, vct_render_gbuffer_rows and vct_gi_pass also write the selected
 * slot's planes (both visibility forms): emission[material of the visible triangle] where a surface is visible, 0 where
 * none is; the rows form touches its tile rows only.
 * vct_set_pixel_emission: planes of the selected frame slot for callers that bring their own G-buffer; layout
 * VCT_GB_LINEAR [3][h*w] or VCT_GB_TILED [tile][3][64], location a vct_mem.  The planes are copied into the slot's own
 * (HOST: done when the call returns; DEVICE: on the slot's stream).  NULL detaches them (with material emission attached
 * the slot keeps planes, zeroed until the next G-buffer pass writes them; a G-buffer pass overwrites a caller's planes too).
 * Every launch that composites takes the selected slot's planes: vct_trace and its slab, resident, row and strided forms,
 * vct_trace_current, a rank's vct_frame_step, the half-rate pass and vct_gi_pass.  Point queries and the voxel view
 * need none.
 * An emitter-only scene needs no switch: a shadow map of all-zero depths (vct_upload_shadow_map) puts every fragment and
 * every pixel in shadow, level 0 is then Em exactly and the direct terms of the frame are 0. */
int vct_upload_emission(vct_ctx* ctx, const float* emission /* [nmat][3] */);
int vct_set_pixel_emission(vct_ctx* ctx, const float* planes, int32_t layout, int32_t location);
int vct_download_pixel_emission(vct_ctx* ctx, float* planes /* linear [3][h*w] */);

/* ---- per-material gloss: specular cone aperture and shininess by class ------------------------------------------------
 * The reference hard-codes one gloss for every surface (S/VoxelConeTracing.fs:213 pow(.., 20), :218 aperture 0.07, with
 * 0.105 left in a comment); config.tan_specular / config.shininess are that pair, one per context.  With gloss classes a
 * polished floor, a brushed rail and a plaster wall reflect differently in ONE frame.
 *   Gloss class        vct_gloss_class { tan_specular, shininess }, at most VCT_GLOSS_CLASSES_MAX = 8 per context.  For a
 *                      pixel of class k the specular cone is Voxel_Cone_Tracing(reflect dir, classes[k].tan_specular) of
 *                      fs:82-107,217-218 and `spec` of fs:213 is pow(max(dot(E,R),0), classes[k].shininess).  Nothing else
 *                      of fs:165-227 changes, nor do the VCT_SHOW_* ternaries, the per-component outputs or the emission
 *                      add.  The six diffuse cones, the voxel chain and the bounce know nothing of gloss.
 *   Class of a pixel   every frame slot has a PIXEL-GLOSS PLANE of one byte per pixel, tiled [tile][64] on the device like
 *                      the emission planes.  A byte b means class (b < nclasses ? b : 0): the plane is never used unclamped
 *                      to form an address, lanes outside a ragged frame may hold anything, and discarded pixels keep the
 *                      clear colour whatever their byte.
 * A small set of classes (not a per-pixel float aperture) keeps what the march is built on: one wave-uniform step table
 * per aperture.  The specular wave of a tile marches once per class present among its live pixels, the other lanes
 * masked off; a pixel is marched exactly once, with its class's table, so its cone is the oracle's cone for that
 * aperture bit for bit and does not depend on its neighbours' classes.
 * vct_set_gloss_classes: builds one step table per class with the builder of config.tan_specular's table (VCT_MAX_STEPS
 * applies; with config.debug_outputs a table of more than 255 steps is refused) and allocates a zeroed plane for every
 * frame slot -- a later second slot gets its own.  NULL or nclasses = 0 detaches: tables and planes are freed and the
 * frame is again the frame of config.tan_specular / config.shininess, bit for bit, from the kernels launched today.
 * While classes are attached those two config values are not used by screen traces (they still serve vct_cone_points
 * aperture 1).  The context's one division verdict (vct_get_stage_counts [2]) covers the diffuse table, the specular
 * table and every class table: one unverifiable divisor in any of them puts all march launches on the IEEE divide.  The
 * first use of a new divisor pays the existing device check (about 2 ms, synchronous, cached per process).
 * Contract: tan_specular finite and > 0, shininess finite and >= 0, 1 <= nclasses <= 8.  VCT_ERR_INVALID, the context
 * keeping what it had: a value outside the contract; config.trace_variant 1 .. 4 (and vct_set_trace_variant refuses
 * 1 .. 4 while classes are attached); config.anisotropic_mips; footprint records on (and vct_set_footprint_records(on)
 * while classes are attached) -- the rule of the half-rate gather, so only the default kernel has a gloss form.
 * vct_get_gloss_classes: the attached table (*nclasses = 0: none) and the march steps of each class's table; any of the
 * three outputs may be NULL.
 * vct_upload_material_gloss: mat_class[nmat], one class byte per material of the uploaded mesh; call after
 * vct_upload_triangles, with the nmat of that call.  NULL detaches, and so does a new vct_upload_triangles.  With it
 * attached (and classes attached, so that the slot has a plane) vct_render_gbuffer, vct_render_gbuffer_rows and
 * vct_gi_pass write the selected slot's plane, in both visibility forms and in the flat and textured shade kernels:
 * mat_class[material of the visible triangle] where a surface is visible, 0 where none is; the rows form touches its
 * tile rows only.  A value >= nclasses is stored as given and read under the clamp rule above.
 * vct_set_pixel_gloss / vct_download_pixel_gloss: the selected slot's plane for callers that bring their own G-buffer;
 * layout VCT_GB_LINEAR [h*w] or VCT_GB_TILED [tile][64], location a vct_mem; copy semantics and stream ordering are
 * those of vct_set_pixel_emission.  NULL zeroes the plane.  Both need classes attached (there is no plane otherwise).
 * Every launch that marches the specular cone of a G-buffer takes the selected slot's plane: vct_trace and its slab,
 * resident, rows and strided forms, vct_trace_current, the last launch of a half-rate pass, vct_gi_pass and a rank's
 * vct_frame_step (each rank's G-buffer pass fills its own rows: nothing new travels between ranks).
 * Point queries: vct_cone_points accepts aperture = VCT_APERTURE_GLOSS(k), k < nclasses, and marches with class k's
 * table; any other value above 1 is VCT_ERR_INVALID.  Gathers are unchanged.
 * vct_last_step_count, vct_last_row_steps and the debug outputs count and hold what was executed: column 6 of a pixel
 * is its own class's march.
 * Out of scope, both follow-ups: mapping an MTL file's Ns to an aperture and quantising a scene's materials into eight
 * classes (that needs a definition nothing here can be checked against), and gloss textures. */
#define VCT_GLOSS_CLASSES_MAX 8
#define VCT_APERTURE_GLOSS(k) (2 + (k))
typedef struct vct_gloss_class { float tan_specular, shininess; } vct_gloss_class;
int vct_set_gloss_classes(vct_ctx* ctx, const vct_gloss_class* classes, int32_t nclasses);
int vct_get_gloss_classes(const vct_ctx* ctx, vct_gloss_class out[8], int32_t* nclasses, int32_t steps[8]);
int vct_upload_material_gloss(vct_ctx* ctx, const uint8_t* mat_class /* [nmat] */);
int vct_set_pixel_gloss(vct_ctx* ctx, const uint8_t* classes, int32_t layout, int32_t location);
int vct_download_pixel_gloss(vct_ctx* ctx, uint8_t* out /* linear [h*w] */);

/* ---- sky light: open cones gather a spherical-harmonic environment ------------------------------------------------------
 * The march of S/VoxelConeTracing.fs:94-104 drops the unoccluded remainder 1 - alpha of a cone: a cone that reaches open
 * air returns black, and the flat ambientFactor term is all that stands in for the sky.  With a SKY attached that
 * remainder gathers the sky's radiance along the cone.
 *   Sky                a context holds at most one: nine real spherical-harmonic coefficients per colour channel,
 *                      float sh[9][3], in the orthonormal real basis in WORLD axes.  Index i = l(l+1)+m goes with the
 *                      polynomials 1, y, z, x, xy, yz, 3z^2-1, xz, x^2-y^2 of the unit direction d = (x, y, z).
 *   Folding            on the host, poly[i][c] = (float)(K_i * (double)sh[i][c]) with K_0 = sqrt(1/4pi) =
 *                      0.28209479177387814, K_1..3 = sqrt(3/4pi) = 0.4886025119029199, K_4,5,7 = sqrt(15/4pi) =
 *                      1.0925484305920792, K_6 = sqrt(5/16pi) = 0.31539156525252005, K_8 = sqrt(15/16pi) =
 *                      0.5462742152960396.  The device sees only poly.
 *   Radiance           of a direction, per channel, in fp32, in exactly this order:
 *                        s = p0; s = fmaf(p1,y,s); s = fmaf(p2,z,s); s = fmaf(p3,x,s);
 *                        s = fmaf(p4,x*y,s); s = fmaf(p5,y*z,s); s = fmaf(p6,fmaf(3.0f*z,z,-1.0f),s);
 *                        s = fmaf(p7,x*z,s); s = fmaf(p8,fmaf(x,x,-(y*y)),s);   sky = fmaxf(s, 0.0f)
 *                      (a second-order series can dip below zero where the sky it approximates does not: the clamp).
 *   A marched cone     with alpha the value the loop test of fs:94 saw last and d the normalised direction the march
 *                      used, becomes   T = fmaxf(1.0f - alpha, 0.0f);   rgb_c = fmaf(T, sky_c(d), rgb_c).
 * The occlusion component and the step count do not change.  This holds however the loop ended: alpha bound, distance
 * bound, or a table of zero steps -- then the cone is the sky.  A pixel or point that is not alive keeps the zero cone; a
 * cone group that the lighting-component mask skips is not marched and gets no sky; a cone whose march is NaN stays NaN.
 * Nothing else of the fragment shader changes: the gather, both occlusion factors, the composite and the per-component
 * outputs read the cones as they now are.  The sky is context state, not frame-slot state.
 * It applies to the screen trace at diffuse rate 1 and 2, with and without gloss classes, in slab, rows and strided
 * launches, and to vct_gather_points and vct_cone_points (every aperture; the caller's direction is used as given).
 * It does NOT apply to vct_bounce (the bounce chain is pinned by its own reference), to the voxel view, or to discarded
 * pixels: they keep the clear colour, the trace has no ray for them.
 * vct_set_sky: NULL detaches; a table whose values are all +0 or -0 counts as detached.  Detached, the frame is the
 * frame without this section, bit for bit, from the kernels launched before it existed.  A NaN or infinite value gives
 * VCT_ERR_INVALID and leaves the state as it was.  Also VCT_ERR_INVALID, the context keeping what it had:
 * config.trace_variant 1 .. 4 (and vct_set_trace_variant refuses 1 .. 4 while a sky is attached);
 * config.anisotropic_mips; footprint records on (and vct_set_footprint_records(on) while a sky is attached) -- the rule
 * of gloss classes and the half-rate gather, so only the default kernel has a sky form.  The call waits for work in
 * flight; the next launch of either frame slot sees the new sky.
 * vct_get_sky: the coefficients as given, their folded form, and whether a sky is attached (zeros and 0 when none is);
 * any of the three outputs may be NULL. */
int vct_set_sky(vct_ctx* ctx, const float sh[9][3]);
int vct_get_sky(const vct_ctx* ctx, float sh[9][3], float poly[9][3], int32_t* attached);

/* ---- G-buffer import: a renderer's depth, normal and colour buffers --------------------------------------------------
 * A deferred renderer keeps a depth or position target, one or two normal targets, RGBA8 colours and perhaps a
 * material-id target; the trace reads 23 fp32 planes, tiled.  The import is the conversion between the two as a stage
 * of the library: one kernel reads the caller's compact buffers and writes the selected frame slot's resident tiled
 * G-buffer; vct_trace_current / vct_trace_resident and their rows forms follow as after vct_render_gbuffer.
 *   Inputs             linear, row-major, tightly packed, of the context's width x height, every non-NULL pointer where
 *                      `location` (a vct_mem) says.  Each needs the alignment of its scalar only: 4 B, or 2 B for the
 *                      F16 and SNORM16 formats.  Frame pixel (x, y), row 0 at the bottom, reads element
 *                      (FLIP_Y ? h-1-y : y) * w + x of every input.
 *   Arithmetic         all fp32: multiplies, adds and compares in the written order, nothing fused, IEEE / and sqrtf.
 *   Surface            DEPTH_F32: none iff depth == depth_clear or depth is NaN.  POSITION_F32X4: none iff w == 0 (w is
 *                      otherwise unused).  POSITION_F32X3: always.  A pixel without a surface gets +0 in all 23 planes
 *                      (the trace discards it) and, with `material`, emission 0 and class 0.
 *   Position           planes 0-2.  F32X3 / F32X4 as given.  DEPTH_F32, with the frame's x and y whatever FLIP_Y says:
 *                        nx = (2(x + 0.5))/w - 1;  ny = (2(y + 0.5))/h - 1;  nz = DEPTH_ZERO_TO_ONE ? depth : 2*depth - 1;
 *                        r_i = ((m[i] nx + m[4+i] ny) + m[8+i] nz) + m[12+i];   P = r_xyz / r_w
 *                      with m = inv_view_proj, column-major: the voxel view's formula.
 *   Decode             F16 to fp32 is exact; UNORM8 is c / 255.0f; SNORM16 is max(s, -32767) / 32767.0f.  Octahedral
 *                      e = (ex, ey): v = (ex, ey, (1 - |ex|) - |ey|), and if v.z < 0 then
 *                      v.x = (1 - |ey|) * (ex >= 0 ? 1 : -1), v.y = (1 - |ex|) * (ey >= 0 ? 1 : -1).
 *   unit(v)            l = sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z);  l > 0 ? v * (1.0f / l) : 0.
 *   Frame              u = unit(normal);  k = (|u.y| >= |u.x| and |u.y| >= |u.z|) ? (0, -u.z, u.y) : (u.z, 0, -u.x);
 *                      t = unit(k);  b = (u.y*t.z - u.z*t.y, u.z*t.x - u.x*t.z, u.x*t.y - u.y*t.x): the construction of
 *                      vcth_frame_from_normal in fp32.  Planes 3-5 = u * normal_scale, 6-8 = t * normal_scale,
 *                      9-11 = b * normal_scale, 12-14 = unit(shading normal), or u without one.  A zero or non-finite
 *                      normal flows through as this arithmetic has it; the G-buffer contract above says what the trace
 *                      does with such a pixel.
 *   Colours            planes 15-17 = albedo rgb; 18 = albedo a, or 1.0f with OPAQUE; 19-21 = specular rgb as given, or
 *                      specular_constant (the .rrra rule of trace.fs:210 is a texture quirk and is not applied).
 *   Shadow             plane 22 = shadow[element] where given.  Otherwise, with a shadow map in the context, the value
 *                      the G-buffer pass writes for a fragment at this Position under the map's stored light matrix (PCF
 *                      count * 0.111f; the same device function) -- except that a pixel for which any of the four
 *                      light-space coordinates is NaN or infinite gets 0 and fetches nothing; every other coordinate
 *                      reaches a texel index only through the PCF's clamps.  Without a map: 25.0f * 0.111f.
 *   Material ids       with `material` and a material emission table attached, the slot's pixel-emission planes get
 *                      emission[id], and 0 for id >= nmat or no surface; with `material`, gloss classes and a material
 *                      gloss map attached, the slot's pixel-gloss plane gets mat_class[id] under the same rule.  Without
 *                      `material` both are left exactly as they are.
 * The import writes the selected slot's OWN tiled buffer and makes it the resident G-buffer, also where the last
 * vct_trace had bound a caller's tiled buffer zero-copy.  The rows form writes tile rows [tile_row0, tile_row1) only
 * (a rank of a multi-GPU frame imports its slab); other rows keep what that buffer held.  VCT_MEM_DEVICE: queued on
 * the slot's stream, returns at once, the inputs must stay valid until the stream has passed it.  VCT_MEM_HOST: staged
 * through buffers the slot owns; returns when the planes are written.  The import reads shared state only (the shadow
 * map, the tables) and is ordered against their writers as the G-buffer pass is.
 * vct_last_gbuffer_import_ms: device time of the import kernel alone; needs vct_set_trace_timing on when the import was
 * issued (VCT_ERR_INVALID otherwise, and before the slot's first import); waits.
 * VCT_ERR_INVALID, nothing touched: NULL ctx or descriptor; NULL position, normal or albedo; an unknown format (of
 * specular only with a specular buffer), location or flag bit; DEPTH_F32 with a non-finite inv_view_proj element;
 * normal_scale not finite or <= 0; specular NULL with a non-finite specular_constant; a tile-row range outside the frame.
 * Out of scope: pitched or tiled inputs and graphics-API interop handles, UNORM8 and 10:10:10:2 normals, sRGB decode
 * (pass linear colours), velocity and history buffers. */
enum { VCT_IMPORT_POSITION_F32X3 = 0, VCT_IMPORT_POSITION_F32X4 = 1, VCT_IMPORT_DEPTH_F32 = 2 };
enum { VCT_IMPORT_NORMAL_F32X3 = 0, VCT_IMPORT_NORMAL_F16X4 = 1, VCT_IMPORT_NORMAL_OCT_SNORM16X2 = 2 };
enum { VCT_IMPORT_COLOR_UNORM8X4 = 0, VCT_IMPORT_COLOR_F16X4 = 1, VCT_IMPORT_COLOR_F32X4 = 2 };
#define VCT_IMPORT_FLIP_Y 1u             /* row 0 of every input is the TOP row (the library's row 0 is the bottom row) */
#define VCT_IMPORT_DEPTH_ZERO_TO_ONE 2u  /* nz = depth (D3D / Vulkan clip space) instead of 2 * depth - 1 (GL) */
#define VCT_IMPORT_OPAQUE 4u             /* plane 18 = 1.0f wherever there is a surface; albedo.a is not read as alpha */
typedef struct vct_gbuffer_import {
    const void* position;        /* required */
    const void* normal;          /* required: the geometric normal (planes 3-11 are derived from it) */
    const void* shading_normal;  /* optional, normal_format too: plane 12-14; NULL = normal */
    const void* albedo;          /* required */
    const void* specular;        /* optional; NULL = specular_constant */
    const float* shadow;         /* optional fp32 [h*w]; NULL = the library's PCF (above) */
    const uint16_t* material;    /* optional [h*w] */
    int32_t position_format, normal_format, albedo_format, specular_format;
    int32_t location;            /* vct_mem: where EVERY non-NULL pointer above lives */
    uint32_t flags;
    float inv_view_proj[16];     /* DEPTH_F32 only: column-major, as vct_render_voxels takes it */
    float depth_clear;           /* DEPTH_F32 only */
    float normal_scale;          /* length given to planes 3-11; 1 = the cone starts one voxel off the surface */
    float specular_constant[3];
} vct_gbuffer_import;
int vct_import_gbuffer(vct_ctx* ctx, const vct_gbuffer_import* in);
int vct_import_gbuffer_rows(vct_ctx* ctx, const vct_gbuffer_import* in, int32_t tile_row0, int32_t tile_row1);
int vct_last_gbuffer_import_ms(vct_ctx* ctx, float* ms);

/* ---- local lights: point and spot lights in the chain and the frame ---------------------------------------------------
 * No reference counterpart (its only light is the directional one), so the definition is this build's.  A context holds
 * up to VCT_LIGHTS_MAX point and spot lights.  They add a direct diffuse term to radiance level 0 -- and so light
 * everything that reads the chain: screen trace at both diffuse rates, vct_bounce, voxel view, point queries,
 * anisotropic chains, footprint records, all unchanged -- and a direct diffuse and specular term to the frame.  They cast
 * NO shadows: a light is bounded by its radius and gated by the surface normal.
 * All arithmetic is fp32; multiplies, adds and compares in the written order, nothing fused; / and sqrtf are IEEE, fmaxf
 * and fminf are C's (a NaN operand gives the other one); dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *   Folding            on the host, once per vct_set_lights; the device sees  R2 = radius*radius,
 *                      S2 = source_radius*source_radius,  a = unit(direction) (the import's unit(v)),
 *                      inv_cone = 1.0f / (cos_inner - cos_outer).
 *   Light j            at a point P with unit normal n:
 *                        d = position - P;  r2 = dot(d, d);  in = r2 < R2   (false for NaN)
 *                        l = d / sqrtf(r2)   (per component; r2 = 0 gives NaN, which the fmaxf below turn into 0)
 *                        q = r2 / R2;  w = fmaxf(1.0f - q*q, 0.0f);  att = (w*w) / fmaxf(r2, S2)
 *                        spot = 1.0f for a point light; for a SPOT: c = dot(a, l) * -1.0f;
 *                               t = fminf(fmaxf((c - cos_outer) * inv_cone, 0.0f), 1.0f);  spot = t*t
 *                        nl = fmaxf(dot(n, l), 0.0f);   k_j = in ? (att * spot) * nl : +0.0f
 *                        Dsum_c = Dsum_c + color_c * k_j      over j = 0 .. n-1 in order, from +0
 *                      A light out of range adds exactly +0, so the kernels skip lights for a whole brick or tile when
 *                      `in` is false for every point of it; the bits are those of the plain loop.
 *   Level 0            (config.voxel_attributes = 1, VCT_VOX_CONSERVATIVE_AVG) after vct_inject_light has written a brick
 *                      -- the saturating emission add included -- for every voxel whose attribute-albedo alpha byte is 255:
 *                      P = the voxel centre (((float)i + 0.5f) / V - 0.5f) * G per axis, as vct_bounce forms it; n = the
 *                      stored normal's bytes - 128, normalised as vct_bounce does; alb_c = the attribute albedo byte / 255;
 *                        texel_c = unorm8 of (texel_c / 255 + alb_c * Dsum_c)   for c = r, g, b (round to nearest,
 *                      clamped: the form of the bounce's write-back); alpha untouched.  A voxel whose stored normal is zero
 *                      (thin geometry whose face normals cancel) has n = NaN, nl = 0 and takes no local light.  Voxels
 *                      without fragments stay 0; the voxel attributes are unchanged.  The term does not depend on the
 *                      shadow map.
 *   Frame              every frame slot gets three fp32 LIT PLANES, tiled [tile][3][64] like the emission planes.  Right
 *                      before every launch that composites a G-buffer -- vct_trace and its slab, resident, rows and strided
 *                      forms, vct_trace_current, the last launch of a half-rate pass, vct_gi_pass, a rank's vct_frame_step --
 *                      one kernel fills them for the tile rows [row0, row1) of that launch (a strided launch: every row of
 *                      the range) from the G-buffer that launch reads.  For a pixel that is not discarded, with P = planes
 *                      0-2, N = planes 12-14, Ev = normalize(camera - P) as the composite forms E, Dsum as above with n = N,
 *                      and per light with the same in, att, spot:
 *                        R = (2.0f * dot(N, l)) * N - l;   sp = powf(fmaxf(dot(Ev, R), 0.0f), shin)
 *                        Ssum_c = Ssum_c + color_c * (in ? (att * spot) * sp : +0)
 *                      (shin = config.shininess, or the pixel's gloss class's under the clamp rule of the gloss plane),
 *                        Lit_c = (SHOW_DIFFUSE ? Dsum_c * albedo_c : 0) + (SHOW_SPECULAR ? Ssum_c * specColor_c : 0)
 *                        plane_c = E_c + Lit_c      (E the slot's pixel-emission plane; Lit_c alone when there is none)
 *                      with the VCT_SHOW_* mask of that launch.  Discarded pixels and lanes outside a ragged frame get +0.
 *                      The launch takes the lit planes in the place of the pixel-emission planes: the composite's last add
 *                      reads ((A + D) + S) + (E + Lit).  The per-component outputs are unchanged.
 * vct_set_lights: NULL or n = 0 detaches.  Waits for work in flight; allocates the device table and zeroed lit planes
 * (12 B per pixel) for every frame slot -- a later second slot gets its own -- so that a launch allocates nothing.  The
 * voxel side takes effect with the next vct_voxelize + vct_inject_light (+ vct_build_mips), exactly as a moved
 * directional light does; the frame side with the next composite launch.  Detached, every kernel launched is the one
 * launched without this section and every frame, chain and plane is bit for bit what it was.  VCT_ERR_INVALID, the
 * context keeping what it had: n < 0 or n > VCT_LIGHTS_MAX; a non-finite field; radius <= 0, source_radius <= 0 or a
 * negative colour; for a SPOT a zero-length axis or not -1 <= cos_outer < cos_inner <= 1; unknown flag bits;
 * config.voxel_attributes = 0; config.trace_variant 1 .. 4 (and vct_set_trace_variant refuses 1 .. 4 while lights are
 * attached).  direction, cos_outer and cos_inner of a point light are checked for finiteness only.
 * vct_voxelize(ctx, VCT_VOX_REFERENCE) with lights attached is VCT_ERR_INVALID, as with emission.
 * vct_get_lights: the attached lights as given (*n = 0: none); either output may be NULL.
 * vct_download_pixel_lights: the lit planes of the selected slot's last composite launch with lights attached;
 * VCT_ERR_INVALID before one.  Rows outside that launch's range hold what earlier launches left (zero at first).
 * vct_last_lights_ms: device time of [0] the voxel kernel of the last vct_inject_light and [1] the pixel kernel of the
 * selected slot's last composite launch; needs lights attached and vct_set_trace_timing on when both were issued
 * (VCT_ERR_INVALID otherwise, and before either has run); waits.
 * Out of scope: shadows of local lights (cube or spot shadow maps, occlusion cones through the chain); two-sided voxels
 * for thin cards whose stored normals cancel; area and tube lights other than through emission; IES profiles; more than
 * 64 lights or clustered light lists; lights in VCT_VOX_REFERENCE mode. */
#define VCT_LIGHTS_MAX 64
#define VCT_LIGHT_SPOT 1u
typedef struct vct_light {            /* 56 B */
    float position[3];  float radius;         /* world units; the light reaches nothing at distance >= radius */
    float color[3];     float source_radius;  /* the factor at distance 1; inverse-square falloff is clamped below source_radius */
    float direction[3]; float cos_outer;      /* SPOT only: axis (need not be unit), cosines of the outer / inner half angle */
    float cos_inner;    uint32_t flags;       /* 0 = point light, VCT_LIGHT_SPOT */
} vct_light;
int vct_set_lights(vct_ctx* ctx, const vct_light* lights, int32_t n);      /* NULL or n = 0 detaches */
int vct_get_lights(const vct_ctx* ctx, vct_light out[VCT_LIGHTS_MAX], int32_t* n);
int vct_download_pixel_lights(vct_ctx* ctx, float* planes /* linear [3][h*w] */);
int vct_last_lights_ms(vct_ctx* ctx, float ms[2]);   /* [0] voxel kernel of the last inject, [1] pixel kernel of the slot's last composite launch */

/* ---- dynamic mesh: moving objects voxelized into the chain per pass ----------------------------------------------------
 * No reference counterpart (its scene never moves), so the definition is this build's.  Beside the uploaded (static)
 * mesh a context may hold ONE dynamic mesh: ntri triangles, model-space fp32 positions [ntri][3][3], a material index per
 * triangle and a flat albedo table [nmat][4] (rgb used), under the same config.model_scale, grid and vertex contract as the
 * static mesh.  It has NO textures and NO emission of its own until vct_set_dynamic_emission attaches a table (below).
 * vct_upload_triangles rebuilds the static plan (allocations, host
 * sorts, synchronisations); the dynamic mesh has no plan: every pass voxelizes it anew on the stream.
 *   A pass             vct_voxelize(VCT_VOX_CONSERVATIVE_AVG) + vct_inject_light, or vct_gi_pass, voxelizes the dynamic
 *                      mesh BY ITSELF exactly as the static one: conservative overlap; per fragment the clamped
 *                      barycentrics, the 25-tap PCF against the context's shadow map and unorm8(albedo * shadow); per voxel
 *                      the rounded integer mean; with config.voxel_attributes the mean albedo and the quantised face normal.
 *                      Bit for bit what the static voxelizer gives for the dynamic mesh alone under the same shadow map.
 *   Merge              the dynamic mesh wins per voxel.  After the static resolve every voxel the dynamic layer occupies
 *                      (fragment count > 0) takes the dynamic texel, every other voxel keeps the static result:
 *                        level0 = D.a > 0 ? D : S
 *                      Order inside vct_inject_light: static resolve (+ emission pool), the static voxels' local lights,
 *                      the merge, the local lights over the dynamic layer's own attributes.  With lights the chain is
 *                      D.a > 0 ? lit(D, Da, Dn) : lit(S', Sa, Sn), S' the static level 0 including emission.
 *   Everything else    reads the chain and follows unchanged: sparse mip build, directional chains, footprint records,
 *                      voxel view (radiance sources), point queries, screen trace, a rank's frame step.  The bricks the
 *                      object left are clean after the next pass, mips included.
 *   Positions          a pass uses those of the last vct_update_dynamic_positions issued before its vct_voxelize.
 *   Vertex contract    a triangle with any coordinate v for which !(fabsf(v * model_scale) <= VCT_VERTEX_LIMIT_GRIDS *
 *                      grid_world_size) -- product in fp32; NaN and the infinities included -- contributes no fragment,
 *                      disturbs no other triangle and is counted (vct_get_dynamic [6]).  The rule is applied on the device
 *                      and is the same for host and device positions: a device pointer cannot be checked on the host.
 *   Capacity           the layer owns max_bricks 8^3 brick slots (26 KiB of device memory each with voxel attributes,
 *                      10 KiB without).  A pass that touches more leaves the WHOLE dynamic layer out -- that pass is the
 *                      static chain, deterministically; never "some" bricks -- and reports its need (vct_get_dynamic [3],
 *                      [7]) so that the caller can attach again with more.  No error is raised.
 * vct_set_dynamic_mesh attaches (replacing an attached one) or, with pos == NULL or ntri == 0, detaches.  It waits for
 * work in flight and allocates everything the per-frame path needs.  max_bricks == 0: the library counts the bricks
 * these positions touch and reserves twice that, at least 64; either way at most the grid's (V/8)^3.  The state survives
 * vct_upload_triangles of a new static mesh.  After a detach the next pass clears what the object left; detached, every
 * kernel launched is the one launched without this section.  Attached, replaced or detached between vct_voxelize and
 * vct_inject_light, the fresh (or no) layer has no pass to resolve: that vct_inject_light gives the static chain, what the
 * previous layer left is cleared, vct_get_dynamic of the fresh layer reports no resolved pass, and the next full pass merges it.
 * vct_update_dynamic_positions: new positions for the same triangles, host or device memory (vct_mem), copied into the
 * context's own buffer on the selected slot's stream; asynchronous; ordered against the other slot like vct_voxelize.
 * Device memory -- and host memory, to be safe -- must stay valid until the stream has passed the copy.
 * With a dynamic mesh attached vct_update_dynamic_positions, vct_voxelize, vct_inject_light and vct_gi_pass allocate
 * nothing, never wait for the stream and copy nothing to the host: the statistics are read by vct_get_dynamic only.
 * vct_get_dynamic: out[0..2] = ntri, nmat, max_bricks; of the last resolved pass out[3] = bricks needed, [4] = bricks used
 * (0 if left out), [5] = conservative fragments, [6] = triangles skipped by the vertex contract, [7] = 1 if the layer was
 * left out for capacity.  Waits for the stream.  Nothing attached: all zero.
 * vct_download_dynamic_voxels: the dynamic layer of the last resolved pass alone -- radiance before local lights, mean
 * albedo, mean normal (the last two need config.voxel_attributes) -- dense linear V^3 * 4 bytes each, zero elsewhere; any
 * pointer may be NULL.
 * vct_last_dynamic_ms: device time of [0] the dynamic kernels of the last vct_voxelize and [1] the merge of the last
 * vct_inject_light; needs vct_set_trace_timing on when they were issued (VCT_ERR_INVALID otherwise and before both ran).
 * VCT_ERR_INVALID, nothing touched: ntri outside 1 .. VCT_DYNAMIC_TRIS_MAX, nmat < 1, max_bricks < 0, a material index
 * out of range, a NULL table, an unknown location, an update without an attached mesh; and while a dynamic mesh is attached
 * vct_voxelize(ctx, VCT_VOX_REFERENCE) (as with emission and lights) and, unless vct_set_dynamic_bounce is on, vct_bounce
 * -- the plain bounce walks the static slots and their attributes only.
 * The second bounce (vct_set_dynamic_bounce; off by default).  With the layer's three volumes D, Da, Dn
 * (vct_download_dynamic_voxels) and the static resolve's S, Sa, Sn, vct_bounce with a mesh attached and the switch on
 * gives, bit for bit, the oracle's
 *   vcto_bounce(chain0 = the merged bounce-0 chain the context holds,
 *               attr_albedo = where(D.a > 0, Da, Sa),  attr_normal = where(D.a > 0, Dn, Sn))
 * with a mip build of the result behind it as ever.  A voxel the layer occupies -- D.a > 0 in the last resolved pass -- is
 * shaded with the layer's albedo and normal, every other voxel with the static ones; both kinds gather their six cones
 * from the merged chain, so static voxels pick up the mover's light and occlusion.  The rule "alpha != 0 and stored normal
 * != zero" applies to the owner's normal.  level0, the bounce's src, is the lit merged texel (local lights, emission);
 * ownership is decided by the layer's own radiance, which is stored before lights.  vct_get_stage_counts reports the
 * oracle's steps.  A pass the layer was left out of (Capacity) bounces as the static chain alone, and so does a pass that
 * had no layer to resolve (attached, replaced or detached between vct_voxelize and vct_inject_light).  Everything else
 * vct_bounce does is unchanged: the second chain's sparse mips, the directional chains, and the return to bounce 0 at the
 * next vct_inject_light.  The switch is context state: it survives attach, replace and detach of the mesh and
 * vct_upload_triangles, does nothing while no mesh is attached, and waits for nothing; the first bounce that needs it
 * allocates one word per 8^3 brick of the grid.  Off, the refusal above stands; detached, or on with nothing attached,
 * every kernel vct_bounce launches, and its argument block, is the one launched without this paragraph.  A value other
 * than 0 or 1: VCT_ERR_INVALID, nothing touched.  vct_get_dynamic_bounce: the state as set.
 * Drawing (vct_set_dynamic_draw; off by default): with VCT_DYNAMIC_DRAW_SHADOW vct_render_shadow_map, with
 * VCT_DYNAMIC_DRAW_GBUFFER vct_render_gbuffer / _rows (and both stages inside vct_gi_pass and a rank's frame step) give,
 * bit for bit -- shadow-map words, all 23 planes, pixel-emission and pixel-gloss planes -- what they would give for ONE
 * static mesh that is the static triangles followed by the dynamic triangles, the appended triangles carrying
 *   positions   those of the last vct_update_dynamic_positions issued before the stage (the rule of a voxelize pass);
 *   frame       one normal, tangent and bitangent per triangle, the same at all three vertices: with p0, p1, p2 the
 *               model-space fp32 positions, e1 = p1 - p0, e2 = p2 - p0,
 *                 n = (e1.y * e2.z - e1.z * e2.y,  e1.z * e2.x - e1.x * e2.z,  e1.x * e2.y - e1.y * e2.x)
 *               each component a * b - c * d with every product and the difference rounded to fp32 (unfused), then
 *               (normal, tangent, bitangent) = the (u, t, b) of the G-buffer import's frame construction from n ("G-buffer
 *               import": u = unit(n), t, b as there).  They are interpolated and inverted like static attributes;
 *   material    albedo rgb of the dynamic table, alpha plane 1.0 whatever the table's fourth value, no alpha test, the
 *               specular colour `specular` (NULL: 0, 0, 0) for every triangle, no textures, gloss class 0, emission 0
 *               unless vct_set_dynamic_emission attached a table (Emission, below).
 * Depth ties resolve as in that one mesh: the lower id wins, so the static mesh wins a tie against the dynamic one.  A
 * triangle outside the vertex contract (the rule above, applied on the device) draws nothing and disturbs nothing.
 * With VCT_DYNAMIC_DRAW_SHADOW the object casts into the map and every PCF reader sees it: the voxelizer (static mesh and
 * dynamic layer), the G-buffer shade and the import's PCF -- the dynamic layer then shadows itself under the 0.002 bias
 * like any static surface.  The flags and the constant are context state: they survive attach, replace and detach of
 * the mesh and vct_upload_triangles, and do nothing while no mesh is attached.  vct_set_dynamic_draw is ordered like
 * vct_update_dynamic_positions and waits for nothing; it allocates (four [ntri][9] arrays) when a flag first goes on for
 * the attached mesh, the stages allocate their scratch for the dynamic triangles in the first pass that draws them (per
 * frame slot a second visibility buffer, 8 bytes per pixel).  Unknown flag bits or a non-finite specular value:
 * VCT_ERR_INVALID, nothing touched.  vct_get_dynamic_draw: the state as set.
 * Emission (vct_set_dynamic_emission; none by default): fp32 rgb per material of the ATTACHED dynamic mesh, flat
 * [nmat][3], every value finite and >= 0 (values above 1 saturate in the chain, as with vct_upload_emission).  NULL or an
 * all-zero table detaches.  The table belongs to the mesh: vct_set_dynamic_mesh drops it on attach, on replace and on
 * detach; vct_upload_triangles of a new static mesh leaves it alone.
 *   Level 0    DEm is, per voxel with at least one dynamic fragment, the rounded integer mean over the same fragments of
 *              unorm8(emission[material] * 1.0f) -- (sum + (c >> 1)) / c per channel, no shadow term: the static emission
 *              rule applied to the dynamic mesh alone.  With D the layer as above,
 *                D'.rgb = min(255, D.rgb + DEm.rgb) per byte,  D'.a = D.a,  level0 = D.a > 0 ? D' : S'
 *              and with local lights D.a > 0 ? lit(D', Da, Dn) : lit(S', Sa, Sn), in the order above.
 *              vct_download_dynamic_voxels' radiance is D' -- still before local lights, its alpha unchanged, so the
 *              second bounce's ownership rule is untouched; the bounce's src is the lit merged texel as ever.
 *   The pass   carries the table that was attached when its vct_voxelize was issued.  Attached or detached between
 *              vct_voxelize and vct_inject_light, that pass has no dynamic emission; replaced in between, it resolves
 *              with the table it was voxelized under.  A pass left out for capacity adds nothing.
 *   Frame      the table attaches zeroed pixel-emission planes to every frame slot as vct_upload_emission does, under the
 *              same rule (refused with config.trace_variant 1 .. 4; a later second slot gets its own); the planes live
 *              while either table is attached.  With VCT_DYNAMIC_DRAW_GBUFFER the G-buffer stages write them as for the
 *              ONE static mesh of "Drawing": the static table (zeros where none is attached) followed by the dynamic
 *              table, the dynamic material indices offset by the static material count.  With the flag off the planes
 *              hold the static table's values, or 0.
 * vct_set_dynamic_emission waits for work in flight and allocates everything (the emission sums, 8 KiB per brick slot),
 * so that a pass with the table attached still allocates nothing, never waits and copies nothing to the host.  With no
 * table attached every kernel launched, and its argument block, is the one launched without this paragraph.
 * VCT_ERR_INVALID, the context keeping what it had: no dynamic mesh attached; a NaN, infinite or negative value (the
 * message names material and channel); the trace_variant conflict.  vct_get_dynamic_emission: the table as set and its
 * material count (*nmat = 0: none attached; emission may be NULL).
 * Parts (vct_set_dynamic_parts; none by default): the attached dynamic mesh may carry part[ntri], one int32 per triangle
 * in 0 .. nparts-1 with 1 <= nparts <= VCT_DYNAMIC_PARTS_MAX, and is then moved by one 3 x 4 matrix per part -- 48 bytes
 * per part and frame instead of 36 per triangle.  Parts need not be contiguous in triangle order; a part may own no
 * triangle.  All arithmetic below is fp32, multiplies and adds in the written order, nothing fused.
 *   Rest       vct_set_dynamic_parts snapshots the layer's CURRENT positions as the REST positions: what the last
 *              vct_set_dynamic_mesh, vct_update_dynamic_positions or vct_update_dynamic_transforms issued before it put
 *              there -- a device-to-device copy on the selected slot's stream, ordered like a position update.  The
 *              current positions are left as they are.
 *   Transform  vct_update_dynamic_transforms(ctx, m, location) takes m[nparts][12], the top three rows of each part's
 *              model matrix, row after row, in host or device memory (vct_mem).  For every vertex (x, y, z) of a rest
 *              triangle of part k, with M = m[k], it writes into the layer's current positions, for r = 0, 1, 2,
 *                p'_r = ((M[4r] * x + M[4r+1] * y) + M[4r+2] * z) + M[4r+3]
 *              Everything downstream follows from these positions exactly as from a vct_update_dynamic_positions of
 *              the same bits: the per-pass voxelization, the device-side vertex contract and its skipped count, the
 *              draw copy and the face frames.
 *   Matrices   ANY fp32 matrix is accepted -- NaN, infinities, singular, mirroring, huge scales: a device pointer cannot
 *              be checked on the host, and the rule is the same for both locations.  Whatever the product gives goes
 *              through the vertex contract on the device: a triangle with a coordinate outside it contributes nothing,
 *              disturbs nothing and is counted.  A mirroring matrix flips the winding; the drawn stages then cull as
 *              they would for the ONE static mesh of "Drawing".  An identity matrix reproduces the rest bits except
 *              that -0 becomes +0 (1 * -0 + 0 * y is +0 when 0 * y is).
 *   Positions  vct_update_dynamic_positions while parts are attached: the given positions become BOTH the rest and the
 *              current positions -- a deforming mesh whose parts are then moved rigidly.  With no parts attached the
 *              call does exactly what it did without this paragraph: the same copy, the same kernel.
 *   Ownership  the parts belong to the mesh: vct_set_dynamic_mesh drops them on attach, replace and detach, as it
 *              drops the emission table.  vct_set_dynamic_parts(ctx, NULL, 0) detaches: the current positions stay as
 *              they are, the rest copy is freed.
 *   Capacity   max_bricks == 0 at attach still counts the bricks of the positions handed to vct_set_dynamic_mesh; a
 *              caller whose parts spread out passes max_bricks itself.  A pose beyond capacity leaves the layer out
 *              and reports its need, as above.
 * vct_set_dynamic_parts waits for work in flight and allocates everything -- the rest copy [ntri][9], the part indices, a
 * 16-byte-aligned matrix table [nparts][12], a timer pair -- so that vct_update_dynamic_transforms allocates nothing,
 * never waits for the stream and copies nothing to the host.  It is ordered like vct_update_dynamic_positions (the
 * positions and the table are shared by both frame slots): it copies the matrices into the context's table on the
 * selected slot's stream, then runs the kernel.  m needs 4-byte alignment only and must stay valid until the stream has
 * passed the copy.  With no parts attached every kernel launched, and its argument block, is the one launched without
 * this paragraph.  vct_get_dynamic_parts: the count (*nparts = 0: none) and, if part is not NULL, the indices as set.
 * vct_download_dynamic_positions: the layer's current positions [ntri][9], with or without parts; waits for the stream.
 * vct_last_dynamic_transform_ms: device time of the last transform kernel; needs vct_set_trace_timing on when the update
 * was issued (VCT_ERR_INVALID otherwise and before any transform has run).
 * VCT_ERR_INVALID, nothing touched: a NULL context; no dynamic mesh attached; nparts outside 1 ..
 * VCT_DYNAMIC_PARTS_MAX, or a NULL part with nparts > 0; a part index outside 0 .. nparts-1 (the message names the
 * triangle); vct_update_dynamic_transforms without parts attached, with NULL m, with an unknown location, or with m not
 * 4-byte aligned.
 * Skin (vct_set_dynamic_skin; none by default): the attached dynamic mesh may carry, per triangle CORNER, four bone
 * indices bone[ntri][3][4] in 0 .. nbones-1 and four fp32 weights weight[ntri][3][4], with 1 <= nbones <=
 * VCT_DYNAMIC_BONES_MAX, and is then moved by one 3 x 4 matrix per BONE: an animated character, cloth on bones, a bending
 * pipe.  The mesh is a triangle soup, so influences are per corner; corners that share a vertex simply carry the same
 * values.  The frame call is vct_update_dynamic_transforms(ctx, m, location) with m[nbones][12], the caller's final
 * skinning matrices (bone x inverse bind): the same table, the same copy, the same ordering, the same 4-byte alignment
 * rule and the same "ANY fp32 matrix is accepted" rule as for Parts.  All arithmetic is fp32, products and sums in the
 * written order, nothing fused.  For a corner with rest position (x, y, z), bones b0 .. b3, weights w0 .. w3 and
 * Mk = m[bk]:
 *                B[j]  = ((w0 * M0[j] + w1 * M1[j]) + w2 * M2[j]) + w3 * M3[j]        j = 0 .. 11
 *                p'_r  = ((B[4r] * x + B[4r+1] * y) + B[4r+2] * z) + B[4r+3]          r = 0, 1, 2
 *   Zero weights  all four terms are ALWAYS evaluated: a weight of 0 does not skip its bone, and 0 * inf is NaN.  A corner
 *              that names a bone whose matrix is not finite therefore takes its triangle out of the vertex contract
 *              even where that bone's weight is 0: the triangle contributes nothing and is counted.  Point unused slots
 *              at a bone that is in use (with weight 0), not at a spare one.
 *   Weights    are used as given: the library does not normalise them.  Each must be finite (checked on the host at
 *              attach); negative values and sums other than 1 are accepted.
 *   Rest, Positions, Ownership, Capacity  as for Parts: vct_set_dynamic_skin snapshots the layer's current positions
 *              as the rest positions; vct_update_dynamic_positions while a skin is attached sets rest and current
 *              positions; vct_set_dynamic_mesh drops the skin, vct_set_dynamic_skin(ctx, NULL, NULL, 0) detaches it and
 *              the current positions stay; max_bricks == 0 counts the bricks of the attached positions only.
 *   Exclusion  parts and a skin exclude each other: attaching one while the other is attached is VCT_ERR_INVALID with
 *              nothing touched (detach the other first).  vct_get_dynamic_parts reports 0 while a skin is attached
 *              and vct_get_dynamic_skin reports 0 while parts are.
 * vct_set_dynamic_skin waits for work in flight and allocates everything -- the rest copy, the indices (stored packed as
 * uint16, 24 bytes per triangle: the last admissible index is 65535), the weights, the 16-byte-aligned matrix table
 * [nbones][12], a timer pair -- so that an update allocates nothing, never waits for the stream and copies nothing to the
 * host.  vct_last_dynamic_transform_ms then reports the skin kernel.  vct_get_dynamic_skin: the count (*nbones = 0: none)
 * and, where not NULL, the indices and the weights as set.  With no skin attached every kernel launched, and its argument
 * block, is the one launched without this paragraph.
 * VCT_ERR_INVALID, nothing touched: a NULL context; no dynamic mesh attached; nbones outside 1 ..
 * VCT_DYNAMIC_BONES_MAX; a NULL array (unless both are NULL and nbones is 0); a bone index outside 0 .. nbones-1 or a
 * weight that is NaN or infinite (the message names triangle, corner and slot); parts attached.
 * Normals (vct_set_dynamic_normals; none by default): the attached dynamic mesh may carry one fp32 normal per triangle
 * CORNER, nrm[ntri][3][3]; the mesh is a triangle soup, so corners that share a vertex simply carry the same values.  The
 * drawn mesh then shades smooth: each corner gets a frame of its own in place of the face frame of "Drawing".  All
 * arithmetic below is fp32, operations in the written order, nothing fused.
 *   Moved normal  of a corner with given normal n.  No mover attached: n' = n.  Parts: with M the triangle's part matrix
 *              and A_r = (M[4r], M[4r+1], M[4r+2]) its rows,
 *                C_0 = A_1 x A_2,  C_1 = A_2 x A_0,  C_2 = A_0 x A_1
 *              each component a * b - c * d in the component order of the face normal n of "Drawing", and
 *                n'_r = ((C_r.x * n.x + C_r.y * n.y) + C_r.z * n.z)                    r = 0, 1, 2
 *              C is the cofactor matrix, not an inverse: cross(A a, A b) = C cross(a, b), so the moved corner normal
 *              stays on the side of the face normal of the moved positions under ANY matrix, mirrors and non-uniform
 *              scales included, with no division and no determinant test.  Skin: the same with the corner's blended B
 *              (Skin, above) in place of M.  A mover whose rest positions have not been moved yet -- between
 *              vct_set_dynamic_parts / _skin or a vct_update_dynamic_positions and the next
 *              vct_update_dynamic_transforms, while the current positions ARE the rest positions -- moves nothing: n' = n.
 *   Frame      of a corner.  (u_f, t_f, b_f) is the face frame exactly as in "Drawing": the face normal of the draw-copy
 *              positions, then the import's frame construction.  With unit() that construction's unit,
 *                u_c = unit(n');   d_f = (u_c.x * u_f.x + u_c.y * u_f.y) + u_c.z * u_f.z
 *              if !(d_f > 0) the corner takes the face frame (u_f, t_f, b_f): NaN, zero, a length that overflows, a
 *              normal 90 degrees or more from its face and anything else that is not a usable normal.  Nothing is an
 *              error.  Otherwise
 *                d = (u_c.x * t_f.x + u_c.y * t_f.y) + u_c.z * t_f.z;   k_i = t_f_i - u_c_i * d;   t_c = unit(k)
 *              and if t_c is all zero the corner takes the face frame; else
 *                b_c = (u_c.y * t_c.z - u_c.z * t_c.y,  u_c.z * t_c.x - u_c.x * t_c.z,  u_c.x * t_c.y - u_c.y * t_c.x)
 *              and the corner's frame is (u_c, t_c, b_c).  The tangent is the FACE's, re-orthogonalised per corner, not a
 *              fresh frame construction per corner: that one chooses its axis on the largest component, the three
 *              corners of a triangle can choose differently, and the shade kernel's (T x B) / det over the interpolated
 *              vectors would pass through det = 0 inside the triangle.  A triangle outside the vertex contract keeps
 *              nine zero positions and the frames the face rule gives for them.
 *   Stages     "Drawing" holds unchanged: the stages equal, bit for bit, the ONE static mesh whose appended triangles
 *              carry these per-corner frames.  Normals have no effect on the shadow map, on any pass with
 *              VCT_DYNAMIC_DRAW_GBUFFER off, or on the voxel layer: Dn stays the quantised face normal, as for the
 *              static voxelizer.
 *   Ownership  the normals belong to the mesh: vct_set_dynamic_mesh drops them on attach, replace and detach.  They
 *              survive attaching, replacing and detaching a mover; they are in the space of the rest positions while a
 *              mover is attached and are used as given while none is -- a caller who detaches a mover in a moved pose
 *              hands over new normals itself.  vct_set_dynamic_normals(ctx, NULL) detaches: the face frames return.
 * vct_set_dynamic_normals waits for work in flight and allocates everything (one [ntri][9] array), so that an update
 * allocates nothing, never waits for the stream and copies nothing to the host.  vct_update_dynamic_normals is for
 * deforming meshes: ordered, and copied on the selected slot's stream, like vct_update_dynamic_positions, with the same
 * 4-byte alignment and pointer-lifetime rules (vct_mem location).  With a draw flag on, the frames are rebuilt behind
 * either call, behind every position or transform update, an attach and a flag going on -- in the launch that makes the
 * draw copy; with no flag on the normals are stored and nothing is launched.  ANY fp32 value is accepted as a normal, host
 * or device: the accept test on the device decides, the stance of "ANY fp32 matrix is accepted".  With no normals
 * attached every kernel launched, and its argument block, is the one launched without this paragraph.
 * vct_get_dynamic_normals: *attached (0: none) and, where nrm is not NULL, the normals as last given.
 * vct_download_dynamic_frames: the draw frames [ntri][9] each as the shade kernel will read them, with or without
 * normals attached; waits for the stream; VCT_ERR_INVALID while no draw flag is on for an attached mesh (the arrays do not
 * exist then).  VCT_ERR_INVALID, nothing touched: a NULL context; no dynamic mesh attached; an update with no normals
 * attached, a NULL pointer, an unknown location or a pointer that is not 4-byte aligned.
 * Known limits: the drawn mesh has no textures, no gloss class and flat (per-face) normals unless
 * vct_set_dynamic_normals attached corner normals (Normals, above).  With a flag off
 * the limit of the stage it names remains: vct_render_shadow_map / vct_render_gbuffer then draw the static mesh only and
 * every kernel launched is the one launched without this paragraph.  The voxel view's albedo / normal sources and
 * vct_download_voxel_attributes show the static pools. */
#define VCT_DYNAMIC_TRIS_MAX (1 << 20)
#define VCT_DYNAMIC_DRAW_SHADOW  1
#define VCT_DYNAMIC_DRAW_GBUFFER 2
int vct_set_dynamic_mesh(vct_ctx* ctx, const float* pos, const int32_t* material, int32_t ntri,
                         const float* albedo, int32_t nmat, int32_t max_bricks);
int vct_update_dynamic_positions(vct_ctx* ctx, const float* pos, int32_t location);
int vct_get_dynamic(vct_ctx* ctx, int32_t out[8]);
int vct_download_dynamic_voxels(vct_ctx* ctx, uint8_t* radiance, uint8_t* albedo, uint8_t* normal);
int vct_last_dynamic_ms(vct_ctx* ctx, float ms[2]);
int vct_set_dynamic_draw(vct_ctx* ctx, int32_t flags, const float specular[3] /* NULL: 0,0,0 */);
int vct_get_dynamic_draw(vct_ctx* ctx, int32_t* flags, float specular[3]);
int vct_set_dynamic_bounce(vct_ctx* ctx, int32_t on);      /* 0 (default) or 1 */
int vct_get_dynamic_bounce(vct_ctx* ctx, int32_t* on);
int vct_set_dynamic_emission(vct_ctx* ctx, const float* emission /* [nmat][3] of the ATTACHED dynamic mesh */);
int vct_get_dynamic_emission(vct_ctx* ctx, float* emission /* [nmat][3], may be NULL */, int32_t* nmat /* 0: none */);
#define VCT_DYNAMIC_PARTS_MAX (1 << 16)
int vct_set_dynamic_parts(vct_ctx* ctx, const int32_t* part /* [ntri], host */, int32_t nparts);
int vct_get_dynamic_parts(vct_ctx* ctx, int32_t* nparts /* 0: none */, int32_t* part /* [ntri], may be NULL */);
int vct_update_dynamic_transforms(vct_ctx* ctx, const float* m /* [nparts][12] */, int32_t location);
int vct_download_dynamic_positions(vct_ctx* ctx, float* pos /* [ntri][9], host */);
int vct_last_dynamic_transform_ms(vct_ctx* ctx, float* ms);
#define VCT_DYNAMIC_BONES_MAX (1 << 16)
int vct_set_dynamic_skin(vct_ctx* ctx, const int32_t* bone /* [ntri][3][4], host */, const float* weight /* [ntri][3][4], host */,
                         int32_t nbones);
int vct_get_dynamic_skin(vct_ctx* ctx, int32_t* nbones /* 0: none */, int32_t* bone, float* weight /* may be NULL */);
int vct_set_dynamic_normals(vct_ctx* ctx, const float* nrm /* [ntri][3][3], host; NULL detaches */);
int vct_update_dynamic_normals(vct_ctx* ctx, const float* nrm, int32_t location);  /* vct_mem */
int vct_get_dynamic_normals(vct_ctx* ctx, int32_t* attached, float* nrm /* may be NULL */);
int vct_download_dynamic_frames(vct_ctx* ctx, float* nrm, float* tan, float* bit /* [ntri][9] each, any may be NULL */);

/* ---- two frames in flight (round 6) -----------------------------------------------------------------
 * The reference's Render() (VCT.h:146-190) issues GL commands; the driver starts frame k + 1 while frame k
 * drains -- nothing in R/main.cpp:77-94 waits for a frame.  A HIP stream does wait: each whole-frame trace
 * launch pays ~20 us of ramp + drain and a dispatch gap before the next kernel of its stream (4-5 % of a
 * 0.61 ms frame).  With n = 2 the context owns two FRAME SLOTS -- stream, G-buffer, RGBA16F frame, step
 * counts, timing events each (190 MB + 17 MB more at 1080p) -- and vct_select_frame_slot(ctx, k & 1) before
 * frame k's vct_render_gbuffer / vct_trace_resident puts consecutive frames on alternate streams: frame
 * k + 1's raster and trace start while frame k's trace drains.  Every entry point works on the selected
 * slot (its G-buffer, its frame, its raster scratch, its vct_last_* values); the chain, shadow map and mesh are
 * shared and ordered by events inside the library:
 * a stage that writes shared state (uploads, vct_render_shadow_map, vct_inject_light, vct_build_mips,
 * vct_bounce, vct_gi_pass) first waits for everything the other slot has in flight, and the other slot's
 * next work waits for it (one cross-stream wait per slot selection: later producers of the same selection
 * skip theirs).  So passes that REWRITE the chain every frame -- vct_gi_pass with a moving light -- run one after
 * the other whatever the slot, and pay the cross-queue hand-over: 0.818 ms per pass on one slot, 0.842 on two
 * (configs[1]; configs[4] equal) -- two slots are for frames that share a chain (Render(): raster + trace).
 * Frames are bit-identical to the one-slot frames.  vct_synchronize waits for both
 * slots.  n = 1 (default) releases the second slot.  Not with config.debug_outputs or trace_variant 4.  A rank of a
 * multi-GPU frame may use it too: vct_frame_step traces on the selected slot's stream, so slab k + 1 starts while slab k
 * drains (a slab launch pays the same ~20 us as a whole frame: a third of an 8-way slab); vct_comm_sync waits for both.
 * Measured: with the round-5 kernel and the timing events of vct_last_trace_ms around every launch, configs[1] trace
 * 0.617 -> 0.591 ms per step, Render() 0.752 -> 0.725.  Most of that turned out to be the events themselves (~7 us of
 * dispatch gaps per launch, which a second stream hides): with vct_set_trace_timing(ctx, 0) one stream runs a
 * trace-only step in the kernel's own time (0.540 ms against 0.548 on two slots; a 1/8 slab step 0.112 either way) and
 * two slots keep 1-2 % only where frames are long (configs[4] trace 2.64 -> 2.58, configs[2] 2.42 -> 2.39, Render()
 * 0.70 -> 0.69) -- opt-in, default 1. */
int vct_set_frames_in_flight(vct_ctx* ctx, int32_t n);
/* streams_overlap: 1 when the second slot's stream was seen to run beside the first at set-up (HIP shares a few hardware
 * queues between a process' streams; the library probes candidates until one overlaps), 0: no such stream was found --
 * results are the same, there is just nothing gained. */
int vct_get_frames_in_flight(const vct_ctx* ctx, int32_t* n, int32_t* selected_slot, int32_t* streams_overlap);
int vct_select_frame_slot(vct_ctx* ctx, int32_t slot);

/* ---- multi-GPU: screen-tile slabs + ONE RCCL gather per frame (BASELINE.json config 4) -------------
 * No reference counterpart (R/main.cpp:77-94 drives one GL context).  One process and one context per
 * GPU; every rank holds the whole scene + chain (voxelize / inject / mips are replicated: cheaper than
 * broadcasting the chain), rasterises and traces only its slab of 8-pixel tile rows, and rank 0 receives
 * the frame through a single ncclGather of padded equal slabs (RCCL over xGMI; rccl.h ncclGather, in
 * place on the root).  Slab r = tile rows [r*per, min((r+1)*per, tiles_y)), per = ceil(tiles_y / world). */
#define VCT_COMM_ID_BYTES 128
int vct_slab_partition(int32_t height, int32_t world, int32_t rank, int32_t* tile_row0, int32_t* tile_row1,
                       int32_t* rows_per_rank);
/* ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to every rank out of band (file, pipe, MPI ...). */
int vct_comm_get_unique_id(void* id128);
/* ncclCommInitRank on the context's device; allocates the two gather buffers (the root's are whole
 * frames), a communication stream and events.  Collective: every rank must call it. */
/* All or nothing: on any failure (allocation, ncclCommInitRank) nothing stays attached to the context and the call
 * may be repeated.
 * VCT_COMM_MODE=direct in the environment (EXPERIMENTAL, default off; no reference counterpart): "direct slabs" -- no
 * RCCL.  The root publishes hipIpc handles of its two frame buffers in a POSIX shared-memory block named after the id,
 * every other rank maps them and its trace kernel stores its slab straight into the root's frame (8 B per pixel over
 * xGMI); the frame's exchange step is a pair of flags in that block (mapped into every rank's GPU) instead of a
 * collective: rank: wait "root is past frame f - 2" -> trace -> "slab f done"; root: trace -> wait for every slab.
 * Every wait has the communicator's deadline (counted in the device's own wall-clock rate) and polls the process' abort
 * word: vct_comm_destroy raises it, drains the streams that still hold queued waits / peer stores and only then closes
 * the mappings.  The root's frame buffers are fine-grained allocations (peers write them, the root's next kernel reads
 * them).  All other vct_comm_* / vct_frame_step calls work unchanged (equal,
 * load-aware and interleaved slabs); vct_comm_get_unique_id then returns 128 random bytes and vct_comm_info reports
 * version 0.  Ranks must be processes of one host.  Tested with several ranks on ONE GPU (tests/test_gpu_multi.py);
 * never run across GPUs -- no multi-GPU box was available to this build. */
int vct_comm_init(vct_ctx* ctx, const void* id128, int32_t rank, int32_t world);
int vct_comm_destroy(vct_ctx* ctx);
int vct_comm_slab(vct_ctx* ctx, int32_t* tile_row0, int32_t* tile_row1);
/* One frame, asynchronous: trace this rank's slab of the resident G-buffer straight into gather buffer k
 * (k alternates), then ONE ncclGather on the communication stream.  Two buffers let frame k+1 be traced while frame
 * k is gathered; measured on one GPU the two do NOT overlap (the gather's kernels queue behind the trace's waves), so
 * budget slab trace + ~23 us dependent dispatch + wire time per frame.  With two frame slots (vct_set_frames_in_flight)
 * the trace runs on the selected slot's stream: slab k + 1 starts while slab k drains (1/8-slab step on one GPU
 * 0.131 -> 0.120 ms).  Collective: every rank calls it once per frame. */
int vct_frame_step(vct_ctx* ctx);
/* Waits for this rank's trace and gather.  Compute still queued in front of the last step's exchange gets the
 * timeout to itself first (its "slab traced" event); then: a peer that died or hangs would keep every other rank inside the
 * collective forever: after the communicator's timeout (default 60 s; VCT_COMM_TIMEOUT_MS in the environment or
 * vct_comm_set_timeout_ms) or on an asynchronous RCCL error the communicator is ABORTED (ncclCommAbort) and the call
 * returns VCT_ERR_DEVICE; afterwards only vct_comm_destroy (then a new vct_comm_init) is accepted on it. */
int vct_comm_sync(vct_ctx* ctx);
int vct_comm_set_timeout_ms(vct_ctx* ctx, int32_t milliseconds);
/* Diagnostics (bench lines of N > 1 runs explain themselves with these): what RCCL reports about the communicator --
 * out[0] ncclCommCount, out[1] ncclCommUserRank, out[2] ncclCommCuDevice, out[3] ncclGetVersion (-1 where the loaded
 * RCCL lacks the entry point) -- and the device time of the last frame's exchange step alone (waits for it). */
int vct_comm_info(vct_ctx* ctx, int32_t out[4]);
int vct_comm_last_gather_ms(vct_ctx* ctx, float* ms);
/* Load-aware slabs (SURVEY.md 8e offers unequal assignment as an option): equal ROWS are not equal WORK -- rows
 * showing sky or near walls march fewer steps.  vct_last_row_steps returns the executed cone steps per 8-pixel tile
 * row of the last screen trace (rows outside a slab trace are 0; nrows = ceil(height / 8)); after summing the
 * ranks' histograms (any out-of-band reduction) vct_slab_partition_weighted cuts [0, tile_rows) into `world`
 * contiguous slabs of near-equal cost (starts[world + 1]), and vct_comm_set_slab_rows installs those boundaries on a
 * communicator (collective; NULL restores the equal partition).  Unequal slabs travel as one fused group of
 * ncclSend / ncclRecv, each slab straight to its rows of the root's frame -- still one exchange step per frame. */
int vct_last_row_steps(vct_ctx* ctx, uint64_t* rows, int32_t nrows);
int vct_slab_partition_weighted(const uint64_t* row_cost, int32_t tile_rows, int32_t world, int32_t* starts);
int vct_comm_set_slab_rows(vct_ctx* ctx, const int32_t* starts);
/* Collective: interleaved slabs -- tile row r belongs to rank r % world, so every rank samples the whole frame and the
 * slabs cost the same by construction (SURVEY.md 8e "interleaved tile assignment ... with a de-interleave after the
 * gather").  The frame still travels as ONE equal-count ncclGather; the root de-interleaves behind it.  on = 0 returns
 * to contiguous equal slabs.  A rank's G-buffer must cover the whole frame (vct_render_gbuffer; vct_gi_pass does). */
int vct_comm_set_interleaved(vct_ctx* ctx, int32_t on);
/* One-GPU check of the interleaved data path for any world size: strided + packed traces of every emulated rank, the
 * root's de-interleave, compared with the frame of one launch; *mismatches = differing pixels. */
int vct_selftest_interleaved(vct_ctx* ctx, int32_t world, uint64_t* mismatches);
/* Root only: the last gathered frame (device pointer valid until the next-but-one vct_frame_step) / a host copy. */
int vct_comm_frame(vct_ctx* ctx, void** rgba16f_dev, size_t* bytes);
int vct_comm_download_frame(vct_ctx* ctx, void* out_rgba16f_host);

/* Debug outputs of the last trace (config.debug_outputs = 1): steps [npix][7] uint8, cones
 * [npix][7][4] fp32, linear pixel order. */
int vct_download_steps(vct_ctx* ctx, uint8_t* steps);
int vct_download_cones(vct_ctx* ctx, float* cones);
/* Executed cone steps of the last trace (always counted). */
int vct_last_step_count(vct_ctx* ctx, uint64_t* steps);
/* Wave-level statistics of the last trace launch -- instrumented builds only (-DVCT_STATS=1; the
 * production library returns VCT_ERR_INVALID): [0] march-loop iterations executed by waves, [1] live
 * lanes summed over them (= executed cone steps), [2] level samples whose cooperative 4x4x4 block was
 * all zero (skipped), [3] served through the cooperative block, [4] served by the per-lane gather,
 * [5] live lanes in [4], [6] those of [4] whose live footprints would fit one block anchored at their minimum,
 * [7] blocks a greedy multi-anchor cover of [4] needs in total, [8..10] those of [4] it covers with <= 2 / 3 / 4
 * blocks, [11..15] quad / quadrant sharing statistics of [4] (tools/trace_stats.py).
 * [16..31] block reuse of the default trace kernel, four counters per (kind of wave, level of the step) in the order
 * diffuse first level, diffuse second, specular first, specular second: cooperative samples for which a slab of the
 * wave held a block of the sample's level; those whose live footprints all lay inside that block (served from it
 * without a fetch); those of them whose block was all zero; candidates whose anchor equalled the one a fresh block
 * would have taken. */
int vct_last_trace_stats(vct_ctx* ctx, uint64_t out[32]);
/* Work-item counts behind the per-stage byte figures of bench.py (`stage_roofline`): [0] triangles uploaded,
 * [1] conservative fragments of the mesh at this grid size (the voxelizer's brick-sorted list), [2] division form of
 * the last march launch (screen trace, slab, frame step, bounce or point query): 0 none yet, 1 the IEEE divide, 2 the verified
 * two-term product (every divisor of the step tables is in the shipped table or passed the device check, 1 - max_alpha
 * >= 2^-5, every two-level blend fraction in [2^-10, 1 - 2^-10]), 3 trace_variant 3's x * r -- in bits 0-7; bits 8-9,
 * set by screen traces: how the launch's typed loads reached a mip level, 2 through one buffer resource per wave with
 * the level's byte offset in the load's scalar operand (the default kernel's plain GL_REPEAT forms of a context whose
 * levels all start below 4 GiB, unless VCT_LEVEL_DESCRIPTORS=1 or the device failed the offset part of the texel
 * self-test), 1 through a resource per level -- [3] brick slots =
 * 8^3 bricks a fragment of the mesh can land in, [4] bricks level 0 shows after the last resolve, [5] compute
 * units reserved for the communication stream (VCT_COMM_RESERVED_CUS; 0 = none), [6] form of the last main-draw
 * visibility pass (0 none yet, 1 direct, 2 tile-binned: chosen per context by timing), [7] work items
 * of the voxelize pass (brick slots, the heavy ones cut into chunks of 4096 fragments).  Synchronises the stream. */
int vct_get_stage_counts(vct_ctx* ctx, uint64_t out[8]);
/* Device time of the last trace kernel launch in milliseconds (HIP events on the ctx stream). */
int vct_last_trace_ms(vct_ctx* ctx, float* ms);
/* on = 0: march launches (trace, slab step, bounce) are no longer bracketed by the two timing events that
 * vct_last_trace_ms reads (it then reports VCT_ERR_INVALID for such a launch).  Default on.  The events cost a launch
 * ~7 us of dispatch gaps on this GPU -- configs[1], steps on one stream: 0.549 -> 0.542 ms; a 1/8 slab's 0.12 ms step
 * pays the same 7 us -- so a frame loop switches them off (the facade does; bench.py does for its timed region and
 * measures the kernel time in a separate loop with them on).  The exchange step of a multi-GPU frame keeps its own
 * pair (vct_comm_last_gather_ms) on the communication stream: leaving those out as well measured no different.
 * No reference counterpart (round 6). */
int vct_set_trace_timing(vct_ctx* ctx, int32_t on);
/* Raw handles for interop (torch tensors wrap these): HIP stream of the context and the
 * device pointers of the resident tiled G-buffer / RGBA16F frame. */
/* Self-test of the kernel's constant division (x / d as fma(x, r_hi, x * r_lo), r_hi + r_lo = 1/d to 48 bits):
 * runs it on the GPU over every fp32 x of its domain (x == +0 or 2^-100 <= |x| < inf, normal quotient)
 * next to the IEEE divide and returns the number of x whose quotient differs.  0 is the guarantee the
 * trace kernel relies on (vct_trace.hip shows why the march never leaves that domain in a way that
 * could change a result). */
int vct_selftest_const_divide(vct_ctx* ctx, float d, uint64_t* mismatches);
/* Round 6: the trace kernels fetch texels through typed-buffer loads (the level as an RGBA8 UNORM texel buffer) and take
 * the four floats the texture path returns instead of decoding the bytes themselves -- valid because that conversion
 * is bit for bit (float)c / 255.0f on gfx950.  This runs every byte value in every channel position through the same
 * load against the library's exact decode, and reads the same texels as two levels of a chain through one resource with
 * their byte offsets in the load's scalar offset operand, against the load without an offset: *mismatches = channel
 * values that differ in either part (0 expected).  vct_create runs it once per process and device; it fails
 * (VCT_ERR_DEVICE) on a device where the conversion is not exact, and on one where only the offset reads differ it
 * traces with a resource per level (vct_get_stage_counts [2], bits 8-9). */
int vct_selftest_texel_buffer(vct_ctx* ctx, uint64_t* mismatches);
/* Self-test of the rasteriser's shared-reciprocal division (csrc/vct_raster.hip div_area: the barycentrics' x / area
 * as two FMA corrections of x * RN(1/area), correctly rounded by Markstein's theorem): `count` pseudo-random pairs of
 * the operands' form (integers of 1..53 bits scaled by 2^-16) next to the IEEE division; returns the number of pairs
 * whose quotients differ in any bit (0 expected; the raster stages' equality with the oracle rests on it). */
int vct_selftest_area_divide(vct_ctx* ctx, uint64_t seed, uint64_t count, uint64_t* mismatches);
int vct_get_stream(vct_ctx* ctx, void** hip_stream);
int vct_get_frame_device(vct_ctx* ctx, void** rgba16f_dev, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif
