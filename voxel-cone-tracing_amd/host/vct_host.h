/*
 * vct_host.h -- host-side scene + camera helpers around the GI hot path (libvct_host.so, plain C++, no HIP).
 *
 * These stand where the reference's asset loader and camera stand:
 *   - scene:   R/Model.h + R/Mesh.h (assimp import, `Vertex` = position / normal / uv / tangent / bitangent,
 *              R/Mesh.h:12-19; diffuse / specular / height textures, R/Model.h:126-136).  There are no assets
 *              in the reference repo and no network here, so the built-in scenes are procedural (Cornell box,
 *              Sponza-class atrium -- flat-coloured or with procedural texture maps); a Wavefront OBJ + MTL
 *              (+ PPM / TGA maps) can be loaded by path.
 *   - camera:  R/Camera.h defaults and the matrices of VCT.h:84-86 (light) and :161-163 (view-projection).
 * The shadow-map and G-buffer stages themselves run on the GPU (vct_render_shadow_map / vct_render_gbuffer,
 * csrc/vct_raster.hip); their CPU checkers live in oracle/ and are not part of this library.
 */
#ifndef VCT_HOST_H_
#define VCT_HOST_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vcth_scene vcth_scene;

typedef struct vcth_camera {
    float position[3];   /* Camera.h: position, default (0,4,0)  VCT.h:8 */
    float yaw, pitch;    /* degrees; defaults -90, 0             Camera.h:21-22 */
    float zoom;          /* fov in degrees, default 45           Camera.h:47 */
    float z_near, z_far; /* 0.1, 1000                            VCT.h:162 */
} vcth_camera;

void vcth_default_camera(vcth_camera* cam);

/* kind: 0 = Cornell box (~40 tris), 1 = atrium (Sponza-class; `detail` scales tessellation,
 * detail = 1.0 gives ~262k triangles; flat colour per material), 2 = the same atrium with procedural
 * texture maps (checker floor + red-only specular map, brick + height map, stone + noisy height map,
 * bronze specular map, cloth with alpha cut-outs), 3 = Bistro-exterior-class street (BASELINE.json configs[4]; detail
 * 1.0 gives ~2.8 M triangles: two rows of facades with windows / balconies / awnings, terraces with tables and chairs,
 * lamps and strings of lights, 14 trees whose crowns are alpha-tested leaf cards with random orientations -- about
 * 40 % of the triangles -- every surface textured, noisy height maps).  Model-space coordinates = world / 0.05
 * (VCT.h:183). */
vcth_scene* vcth_scene_create(int kind, float detail, uint32_t seed);
/* Wavefront OBJ (+ MTL) reader -- stands where the reference's assimp import stands (R/Model.h:39-61:
 * triangulate, smooth normals, tangent space).  Reads v / vn / vt / f (polygons are fan-triangulated,
 * negative indices allowed), usemtl + mtllib (Kd -> albedo, Ks -> specular, d -> albedo alpha); missing
 * normals are generated area-weighted per position, tangents from the UVs when present else from the
 * normal.  map_Kd / map_Ks / map_bump name the diffuse / specular / height textures (R/Model.h:126-136);
 * binary PPM and uncompressed TGA files are decoded, a map that cannot be read leaves the flat colour.  Coordinates
 * are taken as MODEL space (the orchestrator scales by 0.05, VCT.h:183).  Returns NULL on failure;
 * `error` (optional, >= 256 bytes) receives the reason. */
vcth_scene* vcth_scene_load_obj(const char* path, char* error);
/* On-disk cache of a scene (triangles, frames, texture coordinates, materials, decoded texture maps): what
 * R/Model.h:39-61 + :141-226 rebuild from the .obj and its images on every start.  vcth_scene_save returns 0 on
 * success; vcth_scene_load_cache returns NULL (reason in `error`, optional, >= 256 bytes) for a missing,
 * truncated, inconsistent or differently versioned file. */
int vcth_scene_save(const vcth_scene* s, const char* path);
vcth_scene* vcth_scene_load_cache(const char* path, char* error);
void vcth_scene_destroy(vcth_scene* s);
int32_t vcth_scene_num_triangles(const vcth_scene* s);
int32_t vcth_scene_num_materials(const vcth_scene* s);
/* pos [ntri*9], material [ntri], albedo [nmat*4], specular [nmat*3]; any may be NULL. */
void vcth_scene_get(const vcth_scene* s, float* pos, int32_t* material, float* albedo,
                    float* specular);
/* Material emission [nmat*3]: Ke of the MTL file (what vct_upload_emission takes); zero for the procedural scenes and
 * for materials without Ke. */
void vcth_scene_get_emission(const vcth_scene* s, float* emission);

/* Per-vertex frame (R/Mesh.h:12-19): normal, tangent, bitangent [ntri*9] each; any may be NULL. */
void vcth_scene_get_frames(const vcth_scene* s, float* normal, float* tangent, float* bitangent);
/* VCT.h:161-163: perspective(radians(Zoom), w/h, near, far) * camera.GetViewMatrix(), column-major. */
void vcth_camera_view_proj(const vcth_camera* cam, int32_t width, int32_t height, float out_vp[16]);
/* The inverse of a column-major 4x4 matrix, computed in double (Gauss-Jordan, partial pivoting) and rounded to fp32 once:
 * what vct_render_voxels takes for the matrix above.  Returns 0, or -1 for a singular or non-finite matrix (out untouched). */
int32_t vcth_invert_matrix(const float m[16], float out_inv[16]);
/* A tangent frame for callers of vct_gather_points that have only a normal (light probes, particles): t and b are
 * orthogonal to n and to each other, of length `scale`, with dot(cross(t, b), n) > 0 -- the orientation of the frames the
 * scenes of this library carry.  Computed in double from n scaled by its largest component, so any finite non-zero n
 * works (never NaN, no overflow, no underflow); the helper axis is chosen by a branch on n's dominant axis.  n = 0 or a
 * non-finite n gives t = b = 0. */
void vcth_frame_from_normal(const float n[3], float scale, float t[3], float b[3]);
/* A sky for vct_set_sky (include/vct.h "sky light") from three colours: the nine-coefficient projection, per channel, of
 *   L(d) = horizon + (zenith - horizon) * max(t, 0) + (ground - horizon) * max(-t, 0),   t = dot(d, up) / |up|
 * computed in double from the closed form -- zonal coefficients a_0 = sqrt(4 pi) (h + (z - h) / 4 + (g - h) / 4),
 * a_1 = K_1 2 pi ((z - h) - (g - h)) / 3, a_2 = K_6 2 pi (z + g - 2 h) / 4, rotated to `up` by
 * L_lm = sqrt(4 pi / (2l + 1)) a_l Y_lm(up) -- and rounded to float once.  The sky the library then lights with is that
 * second-order series, NOT the gradient itself: it is smooth across the horizon and overshoots the three colours a
 * little (equal colours are reproduced exactly).  up = NULL, zero or non-finite counts as +y. */
void vcth_sky_gradient(const float zenith[3], const float horizon[3], const float ground[3], const float up[3], float sh[9][3]);

/* VCT.h:84-86: DepthViewProjectionMatrix = ortho(-120,120,-120,120,-100,100) * lookAt(L,0,+Y),
 * column-major. */
void vcth_light_view_proj(const float light_dir[3], float out_vp[16]);
/* Texture coordinates [ntri*6] (attribute 2, R/Mesh.h:72-73) and the material textures: RGBA8, row 0 at
 * v = 0; mat_tex [nmat*3] = diffuse / specular / height texture index or -1 (flat colour / flat height). */
void vcth_scene_get_uvs(const vcth_scene* s, float* uv);
int32_t vcth_scene_num_textures(const vcth_scene* s);
void vcth_scene_texture_info(const vcth_scene* s, int32_t i, int32_t* width, int32_t* height);
void vcth_scene_get_texture(const vcth_scene* s, int32_t i, uint8_t* rgba);
void vcth_scene_get_material_textures(const vcth_scene* s, int32_t* mat_tex);

/* The decoder behind map_Kd / map_Ks / map_bump (host/vct_image.h: PNG, baseline JPEG, BMP, TGA raw / RLE, PPM / PGM --
 * the containers stb_image serves the reference with, R/Model.h:141-226).  Two calls: rgba == NULL returns the size;
 * then rgba [h][w][4] with `capacity` bytes of room, row 0 = BOTTOM row (width / height are reported again: check them).
 * Returns 0, -1 when the file is unreadable / unsupported / corrupt, -2 when the image does not fit `capacity` (the
 * file changed between the two calls). */
int32_t vcth_image_load(const char* path, int32_t* width, int32_t* height, uint8_t* rgba, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif
