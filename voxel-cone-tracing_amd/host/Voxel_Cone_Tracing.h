// Voxel_Cone_Tracing.h -- call-compatible facade over the MI355X C ABI (include/vct.h).
//
// Stands where the reference's header-only orchestrator stands (R/Voxel_Cone_Tracing.h:11-252): a
// caller written against the reference -- `camera` global, `Voxel_Cone_Tracing(w, h, window)`,
// `init_voxel_cone_tracing()`, `Render()` per frame (R/main.cpp:64-68,90) -- compiles against this
// header unchanged in those lines.  The type, member and method names are the reference's public
// surface; nothing else is shared: there is no GL, no GLSL and no glm here.  Where the reference
// binds GL objects and issues draws, each method forwards to the C ABI:
//
//   init_voxel_cone_tracing()  VCT.h:67-140   -> vct_create, mesh upload, DrawDepthTexture, DrawVoxelTexture
//   DrawDepthTexture()         VCT.h:192-211  -> vct_render_shadow_map (GPU depth raster from the light)
//   DrawVoxelTexture()         VCT.h:213-250  -> vct_voxelize + vct_inject_light + vct_build_mips
//   Render()                   VCT.h:146-190  -> vct_render_gbuffer (GPU raster of the main draw's vertex and
//                                                non-cone fragment work) + vct_trace_current -> RGBA16F frame
//                                                (ShowVoxels: vct_render_voxels instead, the voxel view)
// Every stage runs on the GPU and a frame never leaves HBM until Frame() is read.
//
// Differences a caller can observe, all forced by running headless on a compute GPU:
//   * `GLFWwindow` is an opaque forward declaration; Render() does not query the window size.
//   * The frame lands in an RGBA16F host buffer (`Frame()`), not in GL framebuffer 0.
//   * `VoxelDimensions` / `VoxelGridWorldSize` are plain members (the reference declares them const,
//     which pins it to 128^3): set them before init_voxel_cone_tracing().
//   * `model_path` replaces the reference's hard-coded absolute Windows path (VCT.h:77; the reference
//     ships no assets): "procedural:atrium", "procedural:atrium-textured", "procedural:bistro", "procedural:cornell", or the path of
//     a Wavefront .obj (+ .mtl with map_Kd / map_Ks / map_bump as PPM or TGA).
//   * Errors keep the reference's print-and-continue behaviour (VCT.h:101-105) and are also
//     readable through `last_status` / vct_last_error(ctx).
#ifndef VOXEL_CONE_TRACING_FACADE_H_
#define VOXEL_CONE_TRACING_FACADE_H_

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/vct.h"
#include "vct_host.h"

struct GLFWwindow;   // opaque: the headless build never dereferences it (the reference does once, VCT.h:149)

// ---- the few glm spellings the reference's public fields use -----------------------------------
struct vec3 {
    float x, y, z;
    vec3() : x(0), y(0), z(0) {}
    vec3(float a, float b, float c) : x(a), y(b), z(c) {}
    vec3 operator+(const vec3& o) const { return vec3(x + o.x, y + o.y, z + o.z); }
    vec3 operator-(const vec3& o) const { return vec3(x - o.x, y - o.y, z - o.z); }
    vec3 operator*(float s) const { return vec3(x * s, y * s, z * s); }
    vec3& operator+=(const vec3& o) { x += o.x; y += o.y; z += o.z; return *this; }
    vec3& operator-=(const vec3& o) { x -= o.x; y -= o.y; z -= o.z; return *this; }
};
struct mat4 {          // column-major like glm: m[col*4 + row]
    float m[16];
    mat4() { memset(m, 0, sizeof(m)); m[0] = m[5] = m[10] = m[15] = 1.0f; }
};
namespace vct_facade {
inline float dot(const vec3& a, const vec3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline vec3 cross(const vec3& a, const vec3& b) {
    return vec3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
inline vec3 normalize(const vec3& a) { const float l = sqrtf(dot(a, a)); return a * (1.0f / l); }
inline float radians(float deg) { return deg * 0.017453292519943295f; }
inline mat4 mul(const mat4& a, const mat4& b) {
    mat4 r;
    for (int c = 0; c < 4; ++c)
        for (int row = 0; row < 4; ++row) {
            float s = 0.0f;
            for (int k = 0; k < 4; ++k) s += a.m[k * 4 + row] * b.m[c * 4 + k];
            r.m[c * 4 + row] = s;
        }
    return r;
}
inline mat4 ortho(float l, float r, float b, float t, float n, float f) {
    mat4 o;
    o.m[0] = 2.0f / (r - l); o.m[5] = 2.0f / (t - b); o.m[10] = -2.0f / (f - n);
    o.m[12] = -(r + l) / (r - l); o.m[13] = -(t + b) / (t - b); o.m[14] = -(f + n) / (f - n);
    return o;
}
inline mat4 lookAt(const vec3& eye, const vec3& center, const vec3& up) {
    const vec3 f = normalize(center - eye), s = normalize(cross(f, up)), u = cross(s, f);
    mat4 o;
    o.m[0] = s.x; o.m[4] = s.y; o.m[8] = s.z;
    o.m[1] = u.x; o.m[5] = u.y; o.m[9] = u.z;
    o.m[2] = -f.x; o.m[6] = -f.y; o.m[10] = -f.z;
    o.m[12] = -dot(s, eye); o.m[13] = -dot(u, eye); o.m[14] = dot(f, eye);
    return o;
}
}  // namespace vct_facade

// ---- Camera: the fly camera main.cpp drives (R/Camera.h:28-145), same members and defaults -----
enum Camera_Direction { FORWARD, BACKWARD, LEFT, RIGHT, UP, DOWN };

class Camera {
public:
    vec3 position, Front, Up, Right, WorldUp;
    float Yaw, Pitch;
    float MovementSpeed, MouseSensitivity, Zoom;

    explicit Camera(vec3 position_ = vec3(0.0f, 0.0f, 0.0f), vec3 Up_ = vec3(0.0f, 1.0f, 0.0f),
                    float Yaw_ = -90.0f, float Pitch_ = 0.0f)
        : position(position_), Front(0.0f, 0.0f, -1.0f), Up(0.0f, 1.0f, 0.0f), WorldUp(Up_),
          Yaw(Yaw_), Pitch(Pitch_), MovementSpeed(2.6f), MouseSensitivity(0.1f), Zoom(45.0f) {
        UpdateCamera();
    }
    mat4 GetViewMatrix() const { return vct_facade::lookAt(position, position + Front, Up); }
    void ProcessKeyBoard(Camera_Direction direction, float& deltaTime) {
        const float v = MovementSpeed * deltaTime;
        switch (direction) {
            case FORWARD: position += Front * v; break;
            case BACKWARD: position -= Front * v; break;
            case LEFT: position -= Right * v; break;
            case RIGHT: position += Right * v; break;
            case UP: position += WorldUp * v; break;
            case DOWN: position -= WorldUp * v; break;
        }
    }
    void ProcessMouseMovement(float& xOffset, float& yOffset, bool constrainPitch = true) {
        xOffset *= MouseSensitivity;
        yOffset *= MouseSensitivity;
        Yaw += xOffset;
        Pitch += yOffset;
        if (constrainPitch) Pitch = fminf(fmaxf(Pitch, -89.0f), 89.0f);
        UpdateCamera();
    }
    void ProcessMouseScroll(float yOffset) { Zoom = fminf(fmaxf(Zoom - yOffset, 1.0f), 45.0f); }
    void UpdateCamera() {
        using namespace vct_facade;
        const float cy = cosf(radians(Yaw)), sy = sinf(radians(Yaw));
        const float cp = cosf(radians(Pitch)), sp = sinf(radians(Pitch));
        Front = normalize(vec3(cy * cp, sp, sy * cp));
        Right = normalize(cross(Front, WorldUp));
        Up = normalize(cross(Right, Front));
    }
};

// the header-defined global main.cpp mutates (VCT.h:8)
inline Camera camera(vec3(0.0f, 4.0f, 0.0f));

// ---- Model: scene container (R/Model.h).  Procedural stand-ins, see the header comment. --------
struct Model {
    vcth_scene* scene = nullptr;
    std::string path;
    Model() {}
    explicit Model(const std::string& p) { Load(p); }
    Model(const Model&) = delete;
    Model& operator=(const Model&) = delete;
    ~Model() { if (scene) vcth_scene_destroy(scene); }
    bool Load(const std::string& p) {
        if (scene) { vcth_scene_destroy(scene); scene = nullptr; }
        path = p;
        char err[256] = "";
        if (p == "procedural:cornell") scene = vcth_scene_create(0, 1.0f, 1234u);
        else if (p == "procedural:atrium") scene = vcth_scene_create(1, 1.0f, 1234u);
        else if (p == "procedural:atrium-textured") scene = vcth_scene_create(2, 1.0f, 1234u);
        else if (p == "procedural:bistro") scene = vcth_scene_create(3, 1.0f, 1234u);        // Bistro-exterior-class street, 2.8 M triangles
        else if (p.size() > 9 && p.compare(p.size() - 9, 9, ".vctscene") == 0) scene = vcth_scene_load_cache(p.c_str(), err);
        else scene = vcth_scene_load_obj(p.c_str(), err);             // R/Model.h:39-61
        if (!scene) printf("ERROR::MODEL: cannot load '%s' (%s; or use procedural:atrium | procedural:cornell)\n",
                           p.c_str(), err);
        return scene != nullptr;
    }
};

struct Voxel_Cone_Tracing {
    // Global properties                                                        VCT.h:14-17
    vec3 lightDirection = vec3(0.0f, 1.0f, 0.25f);
    int VoxelDimensions = 128;
    float VoxelGridWorldSize = 150.0f;

    GLFWwindow* window = nullptr;
    int screen_width = 1280;                                                 // VCT.h:24-25
    int screen_height = 720;

    unsigned ShadowMapSize = 4096;                                           // VCT.h:35

    mat4 DepthViewProjectionMatrix, ProjX, ProjY, ProjZ;                     // VCT.h:42-45
    Model model;                                                             // VCT.h:48
    std::string model_path = "procedural:atrium";

    // VCT.h:51 / S/VoxelConeTracing.fs:36-39: Render() hands them to the composite as the VCT_SHOW_* mask (include/vct.h;
    // all true = VCT_SHOW_ALL, the unmasked frame), and cone groups nothing reads are not marched
    bool ShowDiffuse = true, ShowIndirectDiffuse = true, ShowSpecular = true,
         ShowIndirectSpecular = true, ShowAmbientOcclusion = true;
    float AmbientFactor = 0.1f;                                              // VCT.h:53
    // Multi-GPU (no reference counterpart, R/main.cpp drives one GL context): one process per GPU, each with
    // its own Voxel_Cone_Tracing; set Rank / World / Device and the 128-byte RCCL id (vct_comm_get_unique_id
    // on rank 0, shared out of band) before init.  Render() then rasterises and traces only this rank's
    // slab of tile rows and rank 0's Frame() receives the whole frame through ONE ncclGather.
    int Rank = 0, World = 1, Device = -1;
    unsigned char CommId[VCT_COMM_ID_BYTES] = {0};
    // Extension: the reference never rebuilds the shadow map or the volume after init (a changed lightDirection only
    // moves the direct term, VCT.h:168).  With DynamicLight every Render() is one whole GI pass for the current
    // lightDirection (vct_gi_pass: shadow map, voxelize + inject + mips beside the G-buffer raster, trace).
    bool DynamicLight = false;
    // The reference's own voxelization semantics (S/Voxelization.vs/.gs/.fs as written: dominant-axis raster at pixel
    // centres, last writer wins, VCT.h:213-250) instead of the north-star default (conservative + averaged); set
    // before init or before calling DrawVoxelTexture() again.
    bool ReferenceVoxelization = false;
    // 2: consecutive Render() calls alternate between two frame slots of the context (vct_set_frames_in_flight: own
    // stream, G-buffer and frame each), so frame k + 1's raster and trace start while frame k's trace drains -- what the
    // GL driver does with the reference's frames (R/main.cpp:77-94 never waits for one).  Frame() returns the frame of
    // the last Render().  Same pixels.  What it buys is small since the facade issues its frames without timing events
    // (vct_set_trace_timing: those were most of the gap a second slot hides): configs[1] 0.70 -> 0.69 ms per Render(),
    // erratic at configs[4].  Frames that are whole GI passes (DynamicLight) stay on one slot.  Set before init.
    int FramesInFlight = 1;
    // 2: the six diffuse cones are marched for one pixel per 2x2 quad and the others take a depth- and normal-aware mean
    // of the nearest four (vct_set_diffuse_rate, include/vct.h: no reference counterpart -- the shader marches them per
    // fragment); pixels on edges and thin geometry march their own.  1 (default): every pixel, the reference's frame.
    // Handed over by every Render(), like the Show* switches.  Not on a rank of a multi-GPU run.
    int DiffuseRate = 1;
    // Voxel view (vct_render_voxels, include/vct.h: no reference counterpart): with ShowVoxels on, Render() skips the
    // G-buffer raster and the trace and ray-marches level VoxelViewLevel of VoxelViewSource (a VCT_VOXVIEW_* value) into
    // the frame with the camera's matrix -- Frame() shows the voxels.  Handed over by every Render().  Not on a rank of a
    // multi-GPU run.
    bool ShowVoxels = false;
    int VoxelViewSource = VCT_VOXVIEW_CURRENT;
    int VoxelViewLevel = 0;
    // Emissive materials (vct_upload_emission, include/vct.h: no reference counterpart -- the reference's only light is the
    // directional one): fp32 RGB per material of the model, filled from the MTL file's Ke by init; SetEmission changes
    // it.  The next Render() uploads a changed table and rebuilds the volume from it (DrawVoxelTexture, or the whole GI
    // pass under DynamicLight), as a changed lightDirection is picked up under DynamicLight.  Not with
    // ReferenceVoxelization (that mode is the reference's shaders as written).
    std::vector<float> Emission;                     // [materials][3]
    bool emission_dirty = false;
    // Per-material gloss (vct_set_gloss_classes / vct_upload_material_gloss, include/vct.h: the reference hard-codes one
    // aperture and one shininess for every surface): up to VCT_GLOSS_CLASSES_MAX classes and a class per material of the
    // model (all 0 after init).  SetGlossClasses / SetGloss change them; the next Render() hands them over and its
    // G-buffer pass writes the classes of the visible materials -- no volume rebuild, the voxels know nothing of gloss.
    // An empty class list (the default) is the reference's frame.
    std::vector<vct_gloss_class> GlossClasses;
    std::vector<uint8_t> Gloss;                      // [materials]
    bool gloss_dirty = false;
    // Sky light (vct_set_sky, include/vct.h: the reference's cones return black from open air): nine spherical-harmonic
    // coefficients per channel, all zero (the default) is no sky and the reference's frame.  SetSky / SetSkyGradient change
    // them; the next Render() hands them over -- no volume rebuild, the voxels know nothing of the sky.
    float Sky[9][3] = {};
    bool sky_dirty = false;
    // Local lights (vct_set_lights, include/vct.h "local lights": the reference has the directional light only): up to
    // VCT_LIGHTS_MAX point and spot lights, lighting the voxels and the frame, without shadows.  SetLights changes them;
    // the next Render() hands them over and rebuilds the volume, as it does for a changed emission table.  They need the
    // voxels' albedo and normal: set VoxelAttributes (or Bounces = 2) before init.
    std::vector<vct_light> Lights;
    bool lights_dirty = false;
    bool VoxelAttributes = false;                    // config.voxel_attributes without a second bounce; set before init
    int Bounces = 1;    // 2 = re-inject the lit voxels once (the "2 bounces" of the reference's README.md:16,
                        // which its code does not implement: VCT.h:138-139 injects once); set before init

    // what replaces the GL object names (Depth_FBO, Depth_Texture, VoxelTexture)
    vct_ctx* ctx = nullptr;
    int last_status = VCT_OK;
    // Like the reference's Render() (VCT.h:146-190: draw into framebuffer 0, never read back) a frame stays in HBM;
    // Frame() copies it to the host when -- and only when -- somebody asks for it.
    mutable std::vector<uint16_t> FrameRGBA16F;      // screen_width * screen_height * 4 halves
    mutable bool frame_on_host = false;
    unsigned frame_no = 0;                           // Render() calls so far (FramesInFlight: selects the slot)

    Voxel_Cone_Tracing() {}
    Voxel_Cone_Tracing(int screen_width_, int screen_height_, GLFWwindow*& window_)
        : window(window_), screen_width(screen_width_), screen_height(screen_height_) {}
    Voxel_Cone_Tracing(const Voxel_Cone_Tracing&) = delete;
    Voxel_Cone_Tracing& operator=(const Voxel_Cone_Tracing&) = delete;
    ~Voxel_Cone_Tracing() { if (ctx) vct_destroy(ctx); }

    void init_voxel_cone_tracing() {
        using namespace vct_facade;
        vct_config cfg;
        vct_default_config(&cfg);
        cfg.voxel_dim = VoxelDimensions;
        cfg.grid_world_size = VoxelGridWorldSize;
        cfg.width = screen_width;
        cfg.height = screen_height;
        cfg.shadow_map_size = (int32_t)ShadowMapSize;
        cfg.ambient_factor = AmbientFactor;
        cfg.voxel_attributes = (Bounces >= 2 || VoxelAttributes) ? 1 : 0;
        cfg.device = Device;
        if (!check(vct_create(&cfg, &ctx), "vct_create")) return;
        if (World > 1 || Rank != 0 || CommId[0] || CommId[1])
            if (!check(vct_comm_init(ctx, CommId, Rank, World), "vct_comm_init")) return;
        if (FramesInFlight == 2)
            if (!check(vct_set_frames_in_flight(ctx, 2), "vct_set_frames_in_flight")) return;
        // a frame loop: no timing events around the trace launches (they cost a launch ~7 us; vct_last_trace_ms wants
        // vct_set_trace_timing(ctx, 1) before the frame it is to time)
        if (!check(vct_set_trace_timing(ctx, 0), "vct_set_trace_timing")) return;
        if (!model.Load(model_path)) { last_status = VCT_ERR_INVALID; return; }

        // VCT.h:84-86 and :128-134 (the projections are kept as public data; the HIP voxelizer maps
        // world -> voxel directly, which is what the three of them amount to: SURVEY.md a8)
        const float L[3] = {lightDirection.x, lightDirection.y, lightDirection.z};
        vcth_light_view_proj(L, DepthViewProjectionMatrix.m);
        const float G = VoxelGridWorldSize, h = G * 0.5f;
        const mat4 o = ortho(-h, h, -h, h, h, G * 1.5f);
        ProjX = mul(o, lookAt(vec3(G, 0, 0), vec3(0, 0, 0), vec3(0, 1, 0)));
        ProjY = mul(o, lookAt(vec3(0, G, 0), vec3(0, 0, 0), vec3(0, 0, -1)));
        ProjZ = mul(o, lookAt(vec3(0, 0, G), vec3(0, 0, 0), vec3(0, 1, 0)));

        const int32_t ntri = vcth_scene_num_triangles(model.scene), nmat = vcth_scene_num_materials(model.scene);
        std::vector<float> pos((size_t)ntri * 9), albedo((size_t)nmat * 4), specular((size_t)nmat * 3);
        std::vector<int32_t> material((size_t)ntri);
        vcth_scene_get(model.scene, pos.data(), material.data(), albedo.data(), specular.data());
        if (!check(vct_upload_triangles(ctx, pos.data(), material.data(), ntri, albedo.data(), nmat),
                   "vct_upload_triangles")) return;
        std::vector<float> nrm((size_t)ntri * 9), tan((size_t)ntri * 9), bit((size_t)ntri * 9);
        vcth_scene_get_frames(model.scene, nrm.data(), tan.data(), bit.data());
        if (!check(vct_upload_mesh_attributes(ctx, nrm.data(), tan.data(), bit.data(), specular.data()),
                   "vct_upload_mesh_attributes")) return;
        const int32_t ntex = vcth_scene_num_textures(model.scene);        // R/Model.h:126-136: material textures
        if (ntex > 0) {
            std::vector<float> uv((size_t)ntri * 6);
            vcth_scene_get_uvs(model.scene, uv.data());
            std::vector<std::vector<uint8_t>> texels((size_t)ntex);
            std::vector<const uint8_t*> ptr((size_t)ntex);
            std::vector<int32_t> tw((size_t)ntex), th((size_t)ntex), mat_tex((size_t)nmat * 3);
            for (int32_t i = 0; i < ntex; ++i) {
                vcth_scene_texture_info(model.scene, i, &tw[(size_t)i], &th[(size_t)i]);
                texels[(size_t)i].resize((size_t)tw[(size_t)i] * th[(size_t)i] * 4);
                vcth_scene_get_texture(model.scene, i, texels[(size_t)i].data());
                ptr[(size_t)i] = texels[(size_t)i].data();
            }
            vcth_scene_get_material_textures(model.scene, mat_tex.data());
            if (!check(vct_upload_mesh_uvs(ctx, uv.data()), "vct_upload_mesh_uvs")) return;
            if (!check(vct_upload_textures(ctx, ptr.data(), tw.data(), th.data(), ntex, mat_tex.data()),
                       "vct_upload_textures")) return;
        }
        // Ke of the MTL file, unless SetEmission was called before init for this many materials
        if (Emission.size() != (size_t)nmat * 3) {
            Emission.assign((size_t)nmat * 3, 0.0f);
            vcth_scene_get_emission(model.scene, Emission.data());
        }
        if (!UploadEmission()) return;
        if (Gloss.size() != (size_t)nmat) Gloss.assign((size_t)nmat, 0);
        if (!GlossClasses.empty() && !UploadGloss()) return;
        DrawDepthTexture();     // VCT.h:138
        DrawVoxelTexture();     // VCT.h:139
    }

    // Emission of one material, or the whole table ([materials][3]); picked up by the next Render().
    bool SetEmission(int material, float r, float g, float b) {
        if (material < 0 || (size_t)material * 3 + 2 >= Emission.size()) return false;
        float* e = &Emission[(size_t)material * 3];
        e[0] = r; e[1] = g; e[2] = b;
        emission_dirty = true;
        return true;
    }
    bool SetEmission(const float* table, size_t materials) {
        if (!table || (ctx && materials * 3 != Emission.size())) return false;
        Emission.assign(table, table + materials * 3);
        emission_dirty = true;
        return true;
    }

    // The gloss classes (1 .. VCT_GLOSS_CLASSES_MAX; none: detached), and the class of one material; picked up by the next
    // Render().  Before init SetGloss knows no materials and refuses.
    bool SetGlossClasses(const vct_gloss_class* classes, size_t n) {
        if (n > (size_t)VCT_GLOSS_CLASSES_MAX || (n && !classes)) return false;
        GlossClasses.assign(classes, classes + n);
        gloss_dirty = true;
        return true;
    }
    bool SetGloss(int material, int gloss_class) {
        if (material < 0 || (size_t)material >= Gloss.size() || gloss_class < 0 || gloss_class > 255) return false;
        Gloss[(size_t)material] = (uint8_t)gloss_class;
        gloss_dirty = true;
        return true;
    }

    // The local lights ([n], n <= VCT_LIGHTS_MAX; NULL or 0: none); picked up by the next Render().
    bool SetLights(const vct_light* lights, size_t n) {
        if (n > (size_t)VCT_LIGHTS_MAX || (n && !lights)) return false;
        Lights.assign(lights, lights + n);
        lights_dirty = true;
        return true;
    }

    // The dynamic mesh (vct_set_dynamic_mesh, include/vct.h "dynamic mesh": the reference's scene never moves): a second,
    // small mesh -- flat colours, no textures -- that every volume pass voxelizes anew and merges into the chain, so that
    // moving it costs no upload of the scene.  After init.  pos == NULL detaches.  UpdateDynamicMesh hands over new
    // positions of the same triangles (host memory, or device memory with VCT_MEM_DEVICE); the next volume pass uses
    // them: every Render() under DynamicLight, DrawVoxelTexture() otherwise.  The library's own raster stages draw the
    // object once DrawDynamicMesh says so (below); otherwise its pixels come in through ImportGBuffer.  Not with
    // ReferenceVoxelization; with Bounces = 2 only under DynamicBounce (vct_set_dynamic_bounce: the second bounce shades
    // the object's voxels with the object's albedo and normal), which is handed over here and before every bounce of
    // DrawVoxelTexture() -- with Bounces = 2 that call, not Render(), is the volume pass that follows the object.
    bool DynamicBounce = false;
    bool SetDynamicMesh(const float* pos, const int32_t* material, int32_t ntri, const float* albedo, int32_t nmat,
                        int32_t max_bricks = 0) {
        if (!ctx) return false;
        if (!check(vct_set_dynamic_bounce(ctx, DynamicBounce ? 1 : 0), "vct_set_dynamic_bounce")) return false;
        if (!check(vct_set_dynamic_mesh(ctx, pos, material, ntri, albedo, nmat, max_bricks), "vct_set_dynamic_mesh")) return false;
        // the mesh dropped its emission table: the facade's goes back on if it still fits the materials, else it is forgotten
        if (!pos || ntri == 0 || DynamicEmission.size() != (size_t)nmat * 3) DynamicEmission.clear();
        dynamic_nmat = pos && ntri ? (size_t)nmat : 0;
        if (DynamicEmission.empty()) return true;
        return check(vct_set_dynamic_emission(ctx, DynamicEmission.data()), "vct_set_dynamic_emission");
    }
    // Emission of the dynamic mesh's materials (vct_set_dynamic_emission): fp32 RGB [materials][3], finite and >= 0; NULL
    // detaches.  The object becomes a moving area light in the volume and, drawn (DrawDynamicMesh), is added to the pixels
    // that see it.  Before SetDynamicMesh the table is kept for a mesh with as many materials; after it, it is handed over
    // at once and shows from the next volume pass on.  Not with trace_variant 1 .. 4.
    std::vector<float> DynamicEmission;              // [materials][3]
    size_t dynamic_nmat = 0;
    bool SetDynamicEmission(const float* table, size_t materials) {
        if (!ctx) return false;
        if (!table) DynamicEmission.clear();
        else DynamicEmission.assign(table, table + materials * 3);
        if (!dynamic_nmat) return true;              // no mesh yet: SetDynamicMesh hands it over
        if (table && materials != dynamic_nmat) { DynamicEmission.clear(); return false; }
        return check(vct_set_dynamic_emission(ctx, table ? DynamicEmission.data() : nullptr), "vct_set_dynamic_emission");
    }
    bool UpdateDynamicMesh(const float* pos, int32_t location = VCT_MEM_HOST) {
        if (!ctx) return false;
        return check(vct_update_dynamic_positions(ctx, pos, location), "vct_update_dynamic_positions");
    }
    // Rigid parts of the dynamic mesh (vct_set_dynamic_parts, include/vct.h "dynamic mesh", Parts): an index per triangle in
    // 0 .. nparts-1; the mesh's current positions become the rest positions, and UpdateDynamicTransforms then moves every
    // part by its own 3 x 4 model matrix ([nparts][12] floats, rows first) on the device -- 48 bytes per part and frame
    // instead of 36 per triangle.  After SetDynamicMesh, which drops the parts as the library does; part == NULL detaches.
    // DownloadDynamicPositions returns the current positions [ntri][9] (picking, debugging); it waits for the stream.
    bool SetDynamicParts(const int32_t* part, int32_t nparts) {
        if (!ctx) return false;
        return check(vct_set_dynamic_parts(ctx, part, nparts), "vct_set_dynamic_parts");
    }
    // A skin of the dynamic mesh (vct_set_dynamic_skin, include/vct.h "dynamic mesh", Skin): per triangle corner four bone
    // indices in 0 .. nbones-1 and four weights ([ntri][3][4] each, used as given); UpdateDynamicTransforms then takes one
    // 3 x 4 skinning matrix per bone.  After SetDynamicMesh, which drops the skin; not together with SetDynamicParts;
    // bone == NULL with weight == NULL detaches.
    bool SetDynamicSkin(const int32_t* bone, const float* weight, int32_t nbones) {
        if (!ctx) return false;
        return check(vct_set_dynamic_skin(ctx, bone, weight, nbones), "vct_set_dynamic_skin");
    }
    bool UpdateDynamicTransforms(const float* m3x4, int32_t location = VCT_MEM_HOST) {
        if (!ctx) return false;
        return check(vct_update_dynamic_transforms(ctx, m3x4, location), "vct_update_dynamic_transforms");
    }
    bool DownloadDynamicPositions(float* pos) {
        if (!ctx) return false;
        return check(vct_download_dynamic_positions(ctx, pos), "vct_download_dynamic_positions");
    }
    // Corner normals of the dynamic mesh (vct_set_dynamic_normals, include/vct.h "dynamic mesh", Normals): one fp32 normal
    // per triangle corner, [ntri][3][3]; the drawn mesh (DrawDynamicMesh with `gbuffer`) then shades smooth instead of
    // faceted.  In the space of the rest positions while parts or a skin are attached -- the library moves them with the
    // positions -- and used as given while none is.  After SetDynamicMesh, which drops them; NULL detaches.
    // UpdateDynamicNormals hands over new ones for a deforming mesh (asynchronous, like UpdateDynamicMesh);
    // DownloadDynamicFrames returns the drawn frames [ntri][9] each (any may be NULL) and waits for the stream.
    bool SetDynamicNormals(const float* nrm) {
        if (!ctx) return false;
        return check(vct_set_dynamic_normals(ctx, nrm), "vct_set_dynamic_normals");
    }
    bool UpdateDynamicNormals(const float* nrm, int32_t location = VCT_MEM_HOST) {
        if (!ctx) return false;
        return check(vct_update_dynamic_normals(ctx, nrm, location), "vct_update_dynamic_normals");
    }
    bool DownloadDynamicFrames(float* nrm, float* tan, float* bit) {
        if (!ctx) return false;
        return check(vct_download_dynamic_frames(ctx, nrm, tan, bit), "vct_download_dynamic_frames");
    }
    // Draws the dynamic mesh in the library's own raster stages (vct_set_dynamic_draw): `shadow` -- it casts into the
    // shadow map of DrawDepthTexture() and of every whole GI pass, and every PCF reader sees it; `gbuffer` -- the main
    // draw shows it, with flat per-face normals (or SetDynamicNormals' corner normals), its table's colours and the
    // specular colour `specular` (NULL: black).
    // Render() under DynamicLight then shows and shadows the object.  After init, before or after SetDynamicMesh: the
    // setting outlives the mesh.
    bool DrawDynamicMesh(bool shadow, bool gbuffer, const float* specular = nullptr) {
        if (!ctx) return false;
        const int32_t flags = (shadow ? VCT_DYNAMIC_DRAW_SHADOW : 0) | (gbuffer ? VCT_DYNAMIC_DRAW_GBUFFER : 0);
        return check(vct_set_dynamic_draw(ctx, flags, specular), "vct_set_dynamic_draw");
    }

    // The sky: coefficients as vct_set_sky takes them (NULL: none), or the three colours of a gradient about `up` (NULL: +y)
    // through vcth_sky_gradient; picked up by the next Render().
    void SetSky(const float sh[9][3]) {
        if (sh) memcpy(Sky, sh, sizeof(Sky));
        else memset(Sky, 0, sizeof(Sky));
        sky_dirty = true;
    }
    void SetSkyGradient(const float zenith[3], const float horizon[3], const float ground[3], const float up[3] = nullptr) {
        vcth_sky_gradient(zenith, horizon, ground, up, Sky);
        sky_dirty = true;
    }

    // the five Show* switches as VCT_SHOW_* bits
    uint32_t ShowMask() const {
        return (ShowDiffuse ? (uint32_t)VCT_SHOW_DIFFUSE : 0u) | (ShowIndirectDiffuse ? (uint32_t)VCT_SHOW_INDIRECT_DIFFUSE : 0u) |
               (ShowSpecular ? (uint32_t)VCT_SHOW_SPECULAR : 0u) | (ShowIndirectSpecular ? (uint32_t)VCT_SHOW_INDIRECT_SPECULAR : 0u) |
               (ShowAmbientOcclusion ? (uint32_t)VCT_SHOW_AMBIENT_OCCLUSION : 0u);
    }

    // What every frame hands over before it is drawn: the switches, changed tables, the camera and the light.
    bool HandOverFrameState() {
        vct_set_ambient_factor(ctx, AmbientFactor);
        if (!check(vct_set_lighting_components(ctx, ShowMask()), "vct_set_lighting_components")) return false;
        if (!check(vct_set_diffuse_rate(ctx, DiffuseRate), "vct_set_diffuse_rate")) return false;
        if (emission_dirty) {                                    // a changed table: upload, and rebuild the volume from it
            if (!UploadEmission()) return false;
            if (!DynamicLight || Bounces >= 2) DrawVoxelTexture();      // (a whole GI pass below rebuilds it anyway)
            if (last_status != VCT_OK) return false;
        }
        if (lights_dirty) {                                      // refused lights stay pending, like a refused emission table
            lights_dirty = !check(vct_set_lights(ctx, Lights.empty() ? nullptr : Lights.data(), (int32_t)Lights.size()), "vct_set_lights");
            if (lights_dirty) return false;
            if (!DynamicLight || Bounces >= 2) DrawVoxelTexture();      // the voxels take them with the next voxelize + inject
            if (last_status != VCT_OK) return false;
        }
        if (gloss_dirty && !UploadGloss()) return false;        // changed classes: the G-buffer pass below writes them
        if (sky_dirty) {                                        // a refused sky stays pending, like a refused emission table
            sky_dirty = !check(vct_set_sky(ctx, Sky), "vct_set_sky");
            if (sky_dirty) return false;
        }
        const float cam[3] = {camera.position.x, camera.position.y, camera.position.z};   // VCT.h:167
        const float L[3] = {lightDirection.x, lightDirection.y, lightDirection.z};         // VCT.h:168
        vct_set_camera_position(ctx, cam);
        vct_set_light_direction(ctx, L);
        return true;
    }

    // A frame from the caller's own buffers instead of the model's raster (vct_import_gbuffer, include/vct.h "G-buffer
    // import"; no reference counterpart): what Render() hands over, the import into the selected frame slot -- this
    // rank's slab of tile rows on a multi-GPU run -- and the trace.  Frame() returns it.  The volume is the model's.
    void ImportGBuffer(const vct_gbuffer_import& in) {
        if (!ctx) return;
        if (!HandOverFrameState()) return;
        int32_t row0 = 0, row1 = 0;
        if (vct_comm_slab(ctx, &row0, &row1) == VCT_OK) {
            if (!check(vct_import_gbuffer_rows(ctx, &in, row0, row1), "vct_import_gbuffer_rows")) return;
            if (!check(vct_frame_step(ctx), "vct_frame_step")) return;
        } else {
            if (!check(vct_import_gbuffer(ctx, &in), "vct_import_gbuffer")) return;
            if (!check(vct_trace_resident(ctx), "vct_trace_resident")) return;
        }
        frame_on_host = false;
    }

    void Render() {
        if (!ctx || !model.scene) return;
        if (!HandOverFrameState()) return;
        const float cam[3] = {camera.position.x, camera.position.y, camera.position.z};   // VCT.h:167
        const float L[3] = {lightDirection.x, lightDirection.y, lightDirection.z};         // VCT.h:168
        vcth_camera hc;
        memcpy(hc.position, cam, sizeof(cam));
        hc.yaw = camera.Yaw; hc.pitch = camera.Pitch; hc.zoom = camera.Zoom;
        hc.z_near = 0.1f; hc.z_far = 1000.0f;                                              // VCT.h:162
        float vp[16];
        vcth_camera_view_proj(&hc, screen_width, screen_height, vp);                       // VCT.h:161-163
        // frame k in slot k & 1 -- unless every Render() is a whole GI pass (DynamicLight): passes that rewrite the chain run
        // one after the other whatever the slot and would only pay the hand-over between hardware queues (include/vct.h:
        // 0.842 ms per pass on alternating slots against 0.818 on one), so they stay on the slot that is selected
        int32_t row0 = 0, row1 = 0;
        const bool rank_ctx = vct_comm_slab(ctx, &row0, &row1) == VCT_OK;
        const bool whole_pass = !rank_ctx && DynamicLight && Bounces < 2;
        int32_t slots = 1;
        if (!whole_pass && vct_get_frames_in_flight(ctx, &slots, nullptr, nullptr) == VCT_OK && slots == 2)
            if (!check(vct_select_frame_slot(ctx, (int32_t)(frame_no++ & 1u)), "vct_select_frame_slot")) return;
        if (ShowVoxels) {                                        // the voxel view instead of raster + trace
            float inv[16];
            if (vcth_invert_matrix(vp, inv) != 0) { last_status = VCT_ERR_INVALID; printf("ERROR::VCT::Render: singular view-projection\n"); return; }
            if (!check(vct_render_voxels(ctx, inv, VoxelViewSource, VoxelViewLevel), "vct_render_voxels")) return;
            frame_on_host = false;
            return;
        }
        if (rank_ctx) {                                          // multi-GPU: this rank's slab, one gather
            if (!check(vct_render_gbuffer_rows(ctx, vp, row0, row1), "vct_render_gbuffer_rows")) return;
            if (!check(vct_frame_step(ctx), "vct_frame_step")) return;
            frame_on_host = false;
            return;
        }
        if (whole_pass) {
            vcth_light_view_proj(L, DepthViewProjectionMatrix.m);                          // VCT.h:84-86, per frame
            const int32_t mode = ReferenceVoxelization ? VCT_VOX_REFERENCE : VCT_VOX_CONSERVATIVE_AVG;
            if (!check(vct_gi_pass(ctx, DepthViewProjectionMatrix.m, vp, mode), "vct_gi_pass")) return;
            frame_on_host = false;
            return;
        }
        if (!check(vct_render_gbuffer(ctx, vp), "vct_render_gbuffer")) return;
        if (DiffuseRate == 2) {                                  // whole frames only: no tile-row call at rate 2
            if (!check(vct_trace_resident(ctx), "vct_trace_resident")) return;
        } else if (!check(vct_trace_resident_rows(ctx, 0, (screen_height + 7) / 8), "vct_trace_resident_rows")) return;
        frame_on_host = false;
    }

    // Block until the GPU has finished the frames issued so far (glFinish in GL terms); no copy.
    void Finish() {
        if (!ctx) return;
        int32_t row0 = 0, row1 = 0;
        if (vct_comm_slab(ctx, &row0, &row1) == VCT_OK) check(vct_comm_sync(ctx), "vct_comm_sync");
        else check(vct_synchronize(ctx), "vct_synchronize");
    }

    void DrawDepthTexture() {
        if (!ctx || !model.scene) return;
        check(vct_render_shadow_map(ctx, DepthViewProjectionMatrix.m), "vct_render_shadow_map");
    }

    void DrawVoxelTexture() {
        if (!ctx) return;
        if (!check(vct_voxelize(ctx, ReferenceVoxelization ? VCT_VOX_REFERENCE : VCT_VOX_CONSERVATIVE_AVG), "vct_voxelize")) return;
        if (!check(vct_inject_light(ctx), "vct_inject_light")) return;
        if (!check(vct_build_mips(ctx), "vct_build_mips")) return;          // VCT.h:248
        if (Bounces >= 2 && !check(vct_set_dynamic_bounce(ctx, DynamicBounce ? 1 : 0), "vct_set_dynamic_bounce")) return;
        if (Bounces >= 2) check(vct_bounce(ctx), "vct_bounce");
    }

    // The last frame as RGBA16F on the host (row 0 = bottom row of the GL window): waits for the GPU and downloads on
    // the first call after a Render().  On a multi-GPU run rank 0 holds the gathered frame; other ranks get nullptr.
    const uint16_t* Frame() const {
        if (!ctx) return nullptr;
        if (!frame_on_host) {
            FrameRGBA16F.resize((size_t)screen_width * screen_height * 4);
            int32_t row0 = 0, row1 = 0;
            int rc;
            if (vct_comm_slab(ctx, &row0, &row1) == VCT_OK) {
                if (Rank != 0) { vct_comm_sync(ctx); return nullptr; }
                rc = vct_comm_download_frame(ctx, FrameRGBA16F.data());
            } else {
                rc = vct_download_frame(ctx, FrameRGBA16F.data());
            }
            if (rc != VCT_OK) { printf("ERROR::VCT::Frame: %s\n", vct_last_error(ctx)); return nullptr; }
            frame_on_host = true;
        }
        return FrameRGBA16F.data();
    }

    // Point queries (vct_gather_points / vct_cone_points, include/vct.h: no reference counterpart -- the reference lights
    // only what its camera sees): the six-cone diffuse gather, or one cone, at points the caller names (light probes,
    // lightmap texels, particles), from the volume the last DrawVoxelTexture() built.  Host pointers; the call returns when
    // the outputs are written.  sort_cells: VCT_QUERY_SORT_CELLS, for lists that are not in spatial order (same results).
    // vcth_frame_from_normal makes a tangent frame for a point that has only a normal.
    bool GatherPoints(const vct_gather_point* points, int32_t n, float* out_gather, float* out_cones = nullptr,
                      uint8_t* out_steps = nullptr, bool sort_cells = false) {
        if (!ctx) return false;
        return check(vct_gather_points(ctx, points, n, VCT_MEM_HOST, out_gather, out_cones, out_steps,
                                       sort_cells ? VCT_QUERY_SORT_CELLS : 0u), "vct_gather_points");
    }
    bool ConePoints(const vct_cone_point* points, int32_t n, int32_t aperture, float* out_cone, uint8_t* out_steps = nullptr,
                    bool sort_cells = false) {
        if (!ctx) return false;
        return check(vct_cone_points(ctx, points, n, VCT_MEM_HOST, aperture, out_cone, out_steps,
                                     sort_cells ? VCT_QUERY_SORT_CELLS : 0u), "vct_cone_points");
    }

private:
    bool UploadEmission() {
        // a refused table stays pending: every Render() reports the refusal until SetEmission hands over a valid one
        emission_dirty = !check(vct_upload_emission(ctx, Emission.empty() ? nullptr : Emission.data()), "vct_upload_emission");
        return !emission_dirty;
    }
    bool UploadGloss() {
        // refused classes stay pending, like a refused emission table
        const bool on = !GlossClasses.empty();
        gloss_dirty = !check(vct_set_gloss_classes(ctx, on ? GlossClasses.data() : nullptr, (int32_t)GlossClasses.size()), "vct_set_gloss_classes") ||
                      !check(vct_upload_material_gloss(ctx, on && !Gloss.empty() ? Gloss.data() : nullptr), "vct_upload_material_gloss");
        return !gloss_dirty;
    }
    bool check(int rc, const char* what) {
        last_status = rc;
        if (rc != VCT_OK) printf("ERROR::VCT::%s: %s\n", what, vct_last_error(ctx));
        return rc == VCT_OK;
    }
};

#endif
