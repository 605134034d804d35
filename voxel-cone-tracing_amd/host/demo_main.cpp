// demo_main.cpp -- headless caller with the reference application's call sequence
// (R/main.cpp:64-68 set-up, :77-94 frame loop) against the facade header: proves that a caller
// written for the reference's orchestrator drives the MI355X path unchanged.  Instead of a GLFW
// window and swap-buffers it renders N frames, prints a checksum of the last RGBA16F frame and
// optionally writes it as a tonemapped PPM.
//
//   vct_demo [--scene procedural:atrium|procedural:atrium-textured|procedural:bistro|procedural:cornell] [--voxels 128] [--size 1280x720]
//            [--shadow 4096] [--frames 3] [--bounces 1|2] [--ppm out.ppm] [--gpus N] [--dynamic-light] [--frames-in-flight 1|2]
//            [--show diffuse,indirect-diffuse,specular,indirect-specular,ao] [--diffuse-rate 1|2]
//            [--voxels [current|radiance|albedo|normal[:level]]] [--ambient-cubes NX,NY,NZ FILE] [--dump-chain FILE]
//            [--emission MATERIAL=R,G,B[;MATERIAL=R,G,B...]]
//            [--gloss-classes TAN,SHIN[;TAN,SHIN...] --gloss MATERIAL=CLASS[;MATERIAL=CLASS...]]
//            [--sky-gradient ZR,ZG,ZB;HR,HG,HB;GR,GG,GB[;UX,UY,UZ] | --sky-sh FILE] [--reimport]
//            [--light X,Y,Z;R,G,B;RADIUS;SRC[;DX,DY,DZ;INNER_DEG;OUTER_DEG]]...
//            [--dynamic-obj FILE --dynamic-path X0,Y0,Z0;X1,Y1,Z1 --dynamic-draw shadow|gbuffer|both --dynamic-bounce
//             --dynamic-emission MATERIAL=R,G,B[;MATERIAL=R,G,B...] --dynamic-spin AX,AY,AZ;DEG_PER_FRAME | --dynamic-bend AX,AY,AZ;DEG_PER_FRAME
//             --dynamic-smooth]
// --dynamic-obj FILE: a second Wavefront OBJ as the context's dynamic mesh (Voxel_Cone_Tracing::SetDynamicMesh,
//   vct_set_dynamic_mesh; flat material colours, its textures are not used), translated along the segment of
//   --dynamic-path (model units, the OBJ's own; default: it stays where it is) over the run's frames.  Every Render()
//   is then a whole GI pass, as with --dynamic-light, and hands over the frame's positions first.  The voxels show the
//   object; the library's own raster stages draw it with --dynamic-draw (Voxel_Cone_Tracing::DrawDynamicMesh,
//   vct_set_dynamic_draw): `shadow` lets it cast into the shadow map, `gbuffer` shows it in the frame, `both` both.
//   Without the option a renderer brings its pixels through the G-buffer import.  Prints the two kernel times of
//   vct_last_dynamic_ms.  Not with --gpus; with --bounces 2 only together with --dynamic-bounce
//   (Voxel_Cone_Tracing::DynamicBounce, vct_set_dynamic_bounce: the second bounce runs over the object's voxels too) --
//   every frame then rebuilds the shadow map and the volume, second bounce included, before its Render().
//   --dynamic-emission LIST: emission (fp32 RGB, finite, >= 0) of the listed materials of the dynamic OBJ, over whatever
//   its MTL file's Ke gave them (Voxel_Cone_Tracing::SetDynamicEmission, vct_set_dynamic_emission): the object becomes a
//   moving area light in the volume and, drawn with --dynamic-draw gbuffer|both, is added to the pixels that see it.
//   Checked before a GPU is touched; without the option the Ke values alone are used.
//   --dynamic-spin AX,AY,AZ;DEG_PER_FRAME: the whole OBJ becomes one rigid part (Voxel_Cone_Tracing::SetDynamicParts,
//   vct_set_dynamic_parts) and frame f hands over one 3 x 4 matrix instead of a position array
//   (UpdateDynamicTransforms, vct_update_dynamic_transforms): the --dynamic-path translation at f composed with a rotation
//   by f x DEG about the axis through the object's bounding-box centre, built in double and rounded once.  The per-frame
//   position arrays are then not built.  Finite numbers and a non-zero axis, checked before a GPU is touched.
//   --dynamic-bend AX,AY,AZ;DEG_PER_FRAME: the OBJ is skinned to two bones (Voxel_Cone_Tracing::SetDynamicSkin,
//   vct_set_dynamic_skin) and frame f hands over two matrices: bone 0 the --dynamic-path translation alone, bone 1 that
//   composed with a rotation by f x DEG about the axis through the object's bounding-box centre.  A corner's weight of
//   bone 1 is clamp((c - lo) / (hi - lo), 0, 1) along the longest axis of the bounding box, bone 0 has the rest: the
//   object bends.  Not with --dynamic-spin; checked like it.
//   --dynamic-smooth: the drawn object shades with the OBJ's vertex normals (its vn records, or the reader's area-weighted
//   ones) instead of face normals (Voxel_Cone_Tracing::SetDynamicNormals, vct_set_dynamic_normals); alone, or with
//   --dynamic-path, --dynamic-spin or --dynamic-bend: the library moves the normals with the parts or the skin.  Needs
//   --dynamic-draw gbuffer|both; checked before a GPU is touched.
//
// --light SPEC (repeatable, up to 64): a local light (Voxel_Cone_Tracing::SetLights, vct_set_lights) in world units: a point
//   light at X,Y,Z of colour R,G,B (the factor at distance 1) that reaches RADIUS and whose inverse-square falloff is
//   clamped below SRC; with an axis and the inner and outer half angle in degrees, a spot light.  The lights enter the
//   voxels (the context is then created with voxel attributes) and the frame; they cast no shadows.
//   --light "0,8,0;40,30,20;25;0.5" hangs a warm lamp 8 units above the origin.  Checked before a GPU is touched.
// --reimport: after the frames, the G-buffer the library rasterised is read back and packed on the host into what a deferred
//   renderer keeps -- position F32X3, geometric and shading normals as F16X4, albedo and specular as UNORM8, the shadow
//   plane -- then imported (Voxel_Cone_Tracing::ImportGBuffer, vct_import_gbuffer) and traced, and the relative L2
//   between the two frames is printed: the cost of fp16 normals, 8-bit colours and a synthesised tangent frame.
//   Single GPU only.
// --sky-gradient COLOURS / --sky-sh FILE: sky light (Voxel_Cone_Tracing::SetSkyGradient / SetSky, vct_set_sky): what a
//   cone gathers from the part of its footprint that reaches open air.  The gradient form takes a zenith, a horizon and a
//   ground colour and an optional up vector (+y) and lights with their second-order spherical-harmonic projection
//   (vcth_sky_gradient); the file form takes the 27 coefficients sh[i][c] themselves.  --sky-gradient
//   "0.3,0.5,1.0;0.8,0.8,0.8;0.1,0.1,0.1" is a blue sky over a dark floor.  Both are checked before a GPU is touched.
// --gloss-classes LIST --gloss LIST: per-material gloss (Voxel_Cone_Tracing::SetGlossClasses / SetGloss,
//   vct_set_gloss_classes): up to 8 classes of (specular cone aperture as tan of the half angle, Phong exponent) and the
//   class of the listed material indices (the others are class 0).  --gloss-classes "0.07,20;0.2,4" --gloss "2=1" gives
//   material 2 the wide, dull reflection and leaves the rest as the reference has them.  Both lists are checked before a
//   GPU is touched; a material index the scene does not have is refused after the scene is loaded.
// --emission LIST: emission (fp32 RGB) of the listed material indices, over whatever the scene's MTL file gave them
//   (Voxel_Cone_Tracing::SetEmission, vct_upload_emission): the surfaces become area lights in the volume and are added
//   to the pixels that see them.  The procedural street (procedural:bistro) keeps its lamps in material 10: --emission "10=1,0.9,0.7" lights them.
// --ambient-cubes NX,NY,NZ FILE: after the frames, an irradiance volume -- an NX x NY x NZ grid of probes over the scene's
//   bounds, six axis-aligned gathers each (+x, -x, +y, -y, +z, -z: an ambient cube), through
//   Voxel_Cone_Tracing::GatherPoints (vct_gather_points).  FILE receives raw fp32 [nz][ny][nx][6][4] (rgb + occlusion),
//   FILE.points the [nz][ny][nx][6] vct_gather_point records that were sent.  Single GPU only.
// --dump-chain FILE: the mip chain the trace reads, as vct_download_chain_rgba8 returns it.
// --voxels SOURCE[:LEVEL]: the voxel view instead of the traced frame (Voxel_Cone_Tracing::ShowVoxels,
//   vct_render_voxels): every Render() ray-marches LEVEL (default 0) of the chain the trace reads (current, the default
//   when --voxels stands alone), the bounce-0 radiance chain, or the per-voxel albedo / normal (level 0; they need
//   --bounces 2, which keeps the attributes).  cone_steps and trace_ms then print 0 and view_ms the walk's device time.
//   (--voxels followed by a NUMBER keeps its older meaning, the grid size.)
// --diffuse-rate 2: the six diffuse cones at half screen rate with a depth- and normal-aware upsampling
//   (Voxel_Cone_Tracing::DiffuseRate, vct_set_diffuse_rate); single GPU only.  Default 1.
// --show LIST: the lighting components shown (the reference's Show* switches, VCT.h:51); the ones not listed are off.
//   Default: all five.
// --frames-in-flight 2: consecutive Render() calls alternate between two frame slots (Voxel_Cone_Tracing::FramesInFlight):
//   frame k + 1 starts while frame k drains; same pixels, same checksum.
// --dynamic-light: every Render() re-runs the whole GI pass (shadow map, voxelize, inject, mips, G-buffer, trace)
// for the current lightDirection through vct_gi_pass instead of the reference's build-once volume.
//
// --gpus N: the frame is cut into N screen-tile slabs, one process per GPU (this program re-launches
// itself N times BEFORE anything touches a GPU; rank r uses device r), each rank rasterises and traces its
// slab, rank 0 receives the frame through one ncclGather per frame and prints / writes it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <chrono>
#include <string>
#include <vector>

#include "Voxel_Cone_Tracing.h"
#include "vct_demo_options.h"

static const int SCREEN_WIDTH = 1280;
static const int SCREEN_HEIGHT = 720;

static float half_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    float f;
    if (e == 0) f = ldexpf((float)m, -24);
    else if (e == 31) f = m ? NAN : INFINITY;
    else f = ldexpf((float)(m | 0x400u), (int)e - 25);
    return s ? -f : f;
}

// round to nearest even; overflow to infinity, NaN stays NaN
static uint16_t float_to_half(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u) return (uint16_t)(sign | (u > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                 // rounds to 65536 or more
    if (u < 0x33000001u) return sign;                                       // at most half the smallest subnormal
    if (u < 0x38800000u) {                                                  // subnormal half: m * 2^-24
        const uint32_t shift = 126u - (u >> 23), mant = (u & 0x7fffffu) | 0x800000u;
        const uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
        return (uint16_t)(sign | (q + (rem > halfway || (rem == halfway && (q & 1u)) ? 1u : 0u)));
    }
    const uint32_t q = (u - 0x38000000u) >> 13, rem = u & 0x1fffu;
    return (uint16_t)(sign | (q + (rem > 0x1000u || (rem == 0x1000u && (q & 1u)) ? 1u : 0u)));
}

static uint8_t float_to_unorm8(float v) {
    return (uint8_t)(!(v > 0.0f) ? 0 : (v >= 1.0f ? 255 : (int)(v * 255.0f + 0.5f)));
}

// parent of a multi-GPU run: start one child per rank (fork + exec of this binary; the parent never
// initialises a GPU) and wait for them
static int launch_ranks(int gpus, int argc, char** argv) {
    char idfile[64];
    snprintf(idfile, sizeof(idfile), "/tmp/vct_demo_id_%d", (int)getpid());
    unlink(idfile);
    std::vector<pid_t> kids;
    for (int r = 0; r < gpus; ++r) {
        pid_t pid = fork();
        if (pid == 0) {
            std::vector<std::string> a(argv, argv + argc);
            a.push_back("--rank"); a.push_back(std::to_string(r));
            a.push_back("--idfile"); a.push_back(idfile);
            std::vector<char*> av;
            for (auto& x : a) av.push_back(const_cast<char*>(x.c_str()));
            av.push_back(nullptr);
            execv("/proc/self/exe", av.data());
            perror("execv");
            _exit(127);
        }
        kids.push_back(pid);
    }
    int rc = 0;
    for (pid_t k : kids) {
        int st = 0;
        waitpid(k, &st, 0);
        if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) rc = 5;
    }
    unlink(idfile);
    return rc;
}

int main(int argc, char** argv) {
    int w = SCREEN_WIDTH, h = SCREEN_HEIGHT, frames = 3, voxels = 128, shadow = 4096, bounces = 1;
    int gpus = 0, rank = -1, in_flight = 1, diffuse_rate = 1;
    const char* scene = "procedural:atrium";
    const char* ppm = nullptr;
    bool dynamic_light = false, reimport = false;
    const char* idfile = nullptr;
    const char* show = nullptr;
    const char* cubes_file = nullptr;
    const char* chain_file = nullptr;
    const char* emission = nullptr;
    const char* gloss_classes_arg = nullptr;
    const char* gloss_arg = nullptr;
    const char* sky_gradient_arg = nullptr;
    const char* sky_sh_arg = nullptr;
    std::vector<const char*> light_args;
    const char* dynamic_obj = nullptr;
    const char* dynamic_path = nullptr;
    const char* dynamic_draw = nullptr;
    bool dynamic_bounce = false;
    const char* dynamic_emission = nullptr;
    const char* dynamic_spin = nullptr;
    const char* dynamic_bend = nullptr;
    bool dynamic_smooth = false;
    int cubes[3] = {0, 0, 0};
    bool show_voxels = false;
    int view_source = VCT_VOXVIEW_CURRENT, view_level = 0;
    for (int i = 1; i + 1 < argc; ++i) {
        if (!strcmp(argv[i], "--gpus")) gpus = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--rank")) rank = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--idfile")) idfile = argv[++i];
    }
    if (gpus > 0 && rank < 0) return launch_ranks(gpus, argc, argv);
    // (options with a value consume it; --dynamic-light, --reimport and --dynamic-bounce have none and may stand anywhere)
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--dynamic-light")) { dynamic_light = true; continue; }
        if (!strcmp(argv[i], "--reimport")) { reimport = true; continue; }
        if (!strcmp(argv[i], "--dynamic-bounce")) { dynamic_bounce = true; continue; }
        if (!strcmp(argv[i], "--dynamic-smooth")) { dynamic_smooth = true; continue; }
        if (!strcmp(argv[i], "--voxels") && !(i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9')) {
            show_voxels = true;                             // the voxel view: SOURCE[:LEVEL] may follow
            if (i + 1 < argc && strncmp(argv[i + 1], "--", 2)) {
                const std::string v(argv[++i]);
                const size_t colon = v.find(':');
                const std::string src = v.substr(0, colon);
                const char* names[4] = {"current", "radiance", "albedo", "normal"};
                int k = 0;
                while (k < 4 && src != names[k]) ++k;
                if (k == 4) { fprintf(stderr, "--voxels: unknown source '%s'\n", src.c_str()); return 1; }
                view_source = k;
                if (colon != std::string::npos) view_level = atoi(v.c_str() + colon + 1);
            }
            continue;
        }
        if (i + 1 >= argc) {
            if (!strcmp(argv[i], "--dynamic-draw")) { fprintf(stderr, "%s\n", VCT_DEMO_DYNAMIC_DRAW_USAGE); return 1; }
            break;
        }
        if (!strcmp(argv[i], "--scene")) scene = argv[++i];
        else if (!strcmp(argv[i], "--voxels")) voxels = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--size")) sscanf(argv[++i], "%dx%d", &w, &h);
        else if (!strcmp(argv[i], "--shadow")) shadow = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--frames")) frames = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--bounces")) bounces = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--ppm")) ppm = argv[++i];
        else if (!strcmp(argv[i], "--frames-in-flight")) in_flight = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--show")) show = argv[++i];
        else if (!strcmp(argv[i], "--diffuse-rate")) diffuse_rate = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--dump-chain")) chain_file = argv[++i];
        else if (!strcmp(argv[i], "--emission")) emission = argv[++i];
        else if (!strcmp(argv[i], "--gloss-classes")) gloss_classes_arg = argv[++i];
        else if (!strcmp(argv[i], "--gloss")) gloss_arg = argv[++i];
        else if (!strcmp(argv[i], "--sky-gradient")) sky_gradient_arg = argv[++i];
        else if (!strcmp(argv[i], "--sky-sh")) sky_sh_arg = argv[++i];
        else if (!strcmp(argv[i], "--light") && i + 1 < argc) light_args.push_back(argv[++i]);
        else if (!strcmp(argv[i], "--dynamic-obj")) dynamic_obj = argv[++i];
        else if (!strcmp(argv[i], "--dynamic-path")) dynamic_path = argv[++i];
        else if (!strcmp(argv[i], "--dynamic-draw")) dynamic_draw = argv[++i];
        else if (!strcmp(argv[i], "--dynamic-emission")) dynamic_emission = argv[++i];
        else if (!strcmp(argv[i], "--dynamic-spin")) dynamic_spin = argv[++i];
        else if (!strcmp(argv[i], "--dynamic-bend")) dynamic_bend = argv[++i];
        else if (!strcmp(argv[i], "--ambient-cubes") && i + 2 < argc) {
            if (sscanf(argv[++i], "%d,%d,%d", &cubes[0], &cubes[1], &cubes[2]) != 3 || cubes[0] < 1 || cubes[1] < 1 || cubes[2] < 1 ||
                (long long)cubes[0] * cubes[1] * cubes[2] * 6 > VCT_POINT_QUERY_MAX) {
                fprintf(stderr, "--ambient-cubes: NX,NY,NZ FILE with positive counts\n");
                return 1;
            }
            cubes_file = argv[++i];
        }
    }
    std::vector<vct_gloss_class> gloss_classes;             // --gloss-classes / --gloss: both lists before a GPU is touched
    std::vector<std::pair<int, int>> gloss_of;
    if (gloss_classes_arg) {
        if (const char* at = vct_demo_parse_gloss_classes(gloss_classes_arg, gloss_classes)) {
            fprintf(stderr, "--gloss-classes: TAN,SHIN[;...], 1 to %d classes, TAN > 0 and SHIN >= 0 (at '%s')\n", VCT_GLOSS_CLASSES_MAX, at);
            return 1;
        }
    }
    if (gloss_arg) {
        if (!gloss_classes_arg) { fprintf(stderr, "--gloss: needs --gloss-classes\n"); return 1; }
        if (const char* at = vct_demo_parse_gloss(gloss_arg, (int)gloss_classes.size(), gloss_of)) {
            fprintf(stderr, "--gloss: MATERIAL=CLASS[;...] with classes below %zu (at '%s')\n", gloss_classes.size(), at);
            return 1;
        }
    }
    std::vector<vct_light> lights;                          // --light: every one before a GPU is touched
    if (light_args.size() > (size_t)VCT_LIGHTS_MAX) { fprintf(stderr, "--light: at most %d lights\n", VCT_LIGHTS_MAX); return 1; }
    for (const char* spec : light_args) {
        vct_light l;
        if (const char* at = vct_demo_parse_light(spec, l)) {
            fprintf(stderr, "--light: X,Y,Z;R,G,B;RADIUS;SRC[;DX,DY,DZ;INNER_DEG;OUTER_DEG], finite numbers, colour >= 0, radii > 0, "
                            "axis not zero, 0 <= inner < outer <= 180 (at '%s')\n", at);
            return 1;
        }
        lights.push_back(l);
    }
    // --dynamic-obj / --dynamic-path: the file and the segment before a GPU is touched
    float dyn_path[2][3] = {};
    std::vector<float> dyn_pos, dyn_albedo, dyn_normals;
    std::vector<int32_t> dyn_material;
    int32_t dyn_ntri = 0, dyn_nmat = 0;
    if (dynamic_path && !dynamic_obj) { fprintf(stderr, "--dynamic-path: needs --dynamic-obj\n"); return 1; }
    int dyn_draw_flags = 0;
    if (dynamic_draw) {
        if (!dynamic_obj) { fprintf(stderr, "--dynamic-draw: needs --dynamic-obj\n"); return 1; }
        dyn_draw_flags = vct_demo_parse_dynamic_draw(dynamic_draw);
        if (dyn_draw_flags < 0) { fprintf(stderr, "%s\n", VCT_DEMO_DYNAMIC_DRAW_USAGE); return 1; }
    }
    if (dynamic_bounce && !dynamic_obj) { fprintf(stderr, "--dynamic-bounce: needs --dynamic-obj\n"); return 1; }
    if (dynamic_smooth)
        if (const char* why = vct_demo_check_dynamic_smooth(dynamic_obj != nullptr, dyn_draw_flags)) {
            fprintf(stderr, "%s\n%s\n", why, VCT_DEMO_DYNAMIC_SMOOTH_USAGE);
            return 1;
        }
    if (dynamic_emission && !dynamic_obj) { fprintf(stderr, "--dynamic-emission: needs --dynamic-obj\n"); return 1; }
    double spin_axis[3] = {0.0, 0.0, 1.0}, spin_deg = 0.0, spin_centre[3] = {0.0, 0.0, 0.0};
    if (dynamic_spin) {
        if (!dynamic_obj) { fprintf(stderr, "--dynamic-spin: needs --dynamic-obj\n"); return 1; }
        if (!vct_demo_parse_dynamic_spin(dynamic_spin, spin_axis, &spin_deg)) { fprintf(stderr, "%s\n", VCT_DEMO_DYNAMIC_SPIN_USAGE); return 1; }
    }
    if (dynamic_bend) {                                     // the spin's axis, angle and centre serve the bend's second bone
        if (!dynamic_obj) { fprintf(stderr, "--dynamic-bend: needs --dynamic-obj\n"); return 1; }
        if (dynamic_spin) { fprintf(stderr, "--dynamic-bend: not with --dynamic-spin (parts and a skin exclude each other)\n"); return 1; }
        if (!vct_demo_parse_dynamic_bend(dynamic_bend, spin_axis, &spin_deg)) { fprintf(stderr, "%s\n", VCT_DEMO_DYNAMIC_BEND_USAGE); return 1; }
    }
    const bool dyn_by_matrix = dynamic_spin || dynamic_bend;      // a frame hands over matrices, not positions
    const size_t dyn_nmatrices = dynamic_bend ? 2 : 1;
    float dyn_lo[3] = {0.0f, 0.0f, 0.0f}, dyn_hi[3] = {0.0f, 0.0f, 0.0f};
    std::vector<float> dyn_emission;                        // [dyn_nmat][3]: the OBJ's Ke, then --dynamic-emission over it
    if (dynamic_obj) {
        if (gpus > 0 || (bounces >= 2 && !dynamic_bounce)) { fprintf(stderr, "--dynamic-obj: not with --gpus or --bounces 2\n"); return 1; }
        if (dynamic_path) {
            int used = 0;
            float* q = &dyn_path[0][0];
            if (sscanf(dynamic_path, "%f,%f,%f;%f,%f,%f%n", q, q + 1, q + 2, q + 3, q + 4, q + 5, &used) != 6 || dynamic_path[used]) {
                fprintf(stderr, "--dynamic-path: X0,Y0,Z0;X1,Y1,Z1 in model units\n");
                return 1;
            }
            for (int k = 0; k < 6; ++k)
                if (!std::isfinite(q[k])) { fprintf(stderr, "--dynamic-path: finite numbers\n"); return 1; }
        }
        char err[256] = "";
        vcth_scene* obj = vcth_scene_load_obj(dynamic_obj, err);
        if (!obj) { fprintf(stderr, "--dynamic-obj: cannot load '%s' (%s)\n", dynamic_obj, err); return 1; }
        dyn_ntri = vcth_scene_num_triangles(obj);
        dyn_nmat = vcth_scene_num_materials(obj);
        if (dyn_ntri < 1 || dyn_ntri > VCT_DYNAMIC_TRIS_MAX || dyn_nmat < 1) {
            fprintf(stderr, "--dynamic-obj: %d triangles, a dynamic mesh takes 1 .. %d\n", (int)dyn_ntri, VCT_DYNAMIC_TRIS_MAX);
            vcth_scene_destroy(obj);
            return 1;
        }
        dyn_pos.resize((size_t)dyn_ntri * 9); dyn_albedo.resize((size_t)dyn_nmat * 4); dyn_material.resize((size_t)dyn_ntri);
        std::vector<float> unused_specular((size_t)dyn_nmat * 3);
        vcth_scene_get(obj, dyn_pos.data(), dyn_material.data(), dyn_albedo.data(), unused_specular.data());
        dyn_emission.assign((size_t)dyn_nmat * 3, 0.0f);
        vcth_scene_get_emission(obj, dyn_emission.data());
        if (dynamic_smooth) {                               // the file's vn, or the reader's area-weighted normals
            dyn_normals.resize((size_t)dyn_ntri * 9);
            vcth_scene_get_frames(obj, dyn_normals.data(), nullptr, nullptr);
        }
        vcth_scene_destroy(obj);
        if (dynamic_emission)
            if (const char* at = vct_demo_parse_dynamic_emission(dynamic_emission, dyn_nmat, dyn_emission)) {
                fprintf(stderr, "%s; the OBJ has %d materials (at '%s')\n", VCT_DEMO_DYNAMIC_EMISSION_USAGE, (int)dyn_nmat, at);
                return 1;
            }
        if (dyn_by_matrix) {                                // the axis goes through the centre of the object's bounding box
            for (int k = 0; k < 3; ++k) {
                float lo = dyn_pos[(size_t)k], hi = lo;
                for (size_t i = (size_t)k; i < dyn_pos.size(); i += 3) { lo = std::min(lo, dyn_pos[i]); hi = std::max(hi, dyn_pos[i]); }
                spin_centre[k] = 0.5 * ((double)lo + (double)hi);
                dyn_lo[k] = lo; dyn_hi[k] = hi;
            }
        }
        dynamic_light = true;                               // a whole GI pass per frame: the volume follows the object
    }
    float sky_sh[9][3] = {};                                // --sky-gradient / --sky-sh: before a GPU is touched
    if (sky_gradient_arg && sky_sh_arg) { fprintf(stderr, "--sky-gradient and --sky-sh: one sky per context\n"); return 1; }
    if (sky_gradient_arg) {
        float zenith[3], horizon[3], ground[3], up[3];
        if (const char* at = vct_demo_parse_sky_gradient(sky_gradient_arg, zenith, horizon, ground, up)) {
            fprintf(stderr, "--sky-gradient: ZR,ZG,ZB;HR,HG,HB;GR,GG,GB[;UX,UY,UZ], finite numbers, up not zero (at '%s')\n", at);
            return 1;
        }
        vcth_sky_gradient(zenith, horizon, ground, up, sky_sh);
    }
    if (sky_sh_arg && !vct_demo_read_sky_sh(sky_sh_arg, sky_sh)) {
        fprintf(stderr, "--sky-sh: %s does not hold 27 finite numbers\n", sky_sh_arg);
        return 1;
    }
    GLFWwindow* window = nullptr;          // no window system on a compute node

    camera.MovementSpeed = 5.0f;           // R/main.cpp:64-65
    camera.MouseSensitivity = 0.5f;
    if (!strcmp(scene, "procedural:cornell")) {
        camera.position = vec3(0.0f, 0.0f, 58.0f);
    } else {
        camera.position = vec3(-56.0f, -9.0f, 2.0f);
        camera.Yaw = 0.0f; camera.Pitch = 8.0f;
        camera.UpdateCamera();
    }
    Voxel_Cone_Tracing voxel_cone_tracing(w, h, window);    // R/main.cpp:66
    voxel_cone_tracing.VoxelDimensions = voxels;
    voxel_cone_tracing.ShadowMapSize = (unsigned)shadow;
    voxel_cone_tracing.model_path = scene;
    voxel_cone_tracing.Bounces = bounces;
    voxel_cone_tracing.DynamicBounce = dynamic_bounce;
    voxel_cone_tracing.VoxelAttributes = !lights.empty();   // --light: the lights read the voxels' albedo and normal
    voxel_cone_tracing.DynamicLight = dynamic_light;       // every Render() = one whole GI pass (vct_gi_pass)
    voxel_cone_tracing.FramesInFlight = in_flight;
    voxel_cone_tracing.DiffuseRate = diffuse_rate;
    voxel_cone_tracing.ShowVoxels = show_voxels;
    voxel_cone_tracing.VoxelViewSource = view_source;
    voxel_cone_tracing.VoxelViewLevel = view_level;
    if (show) {                                             // --show: the listed Show* switches on, the others off
        bool* flags[5] = {&voxel_cone_tracing.ShowDiffuse, &voxel_cone_tracing.ShowIndirectDiffuse, &voxel_cone_tracing.ShowSpecular,
                          &voxel_cone_tracing.ShowIndirectSpecular, &voxel_cone_tracing.ShowAmbientOcclusion};
        const char* names[5] = {"diffuse", "indirect-diffuse", "specular", "indirect-specular", "ao"};
        for (bool* f : flags) *f = false;
        const std::string list(show);
        for (size_t p = 0; p <= list.size();) {
            size_t q = list.find(',', p);
            if (q == std::string::npos) q = list.size();
            const std::string item = list.substr(p, q - p);
            int k = 0;
            while (k < 5 && item != names[k]) ++k;
            if (k == 5 && !item.empty()) { fprintf(stderr, "--show: unknown component '%s'\n", item.c_str()); return 1; }
            if (k < 5) *flags[k] = true;
            p = q + 1;
        }
    }
    if (gpus > 0) {                                         // a rank of a multi-GPU run
        voxel_cone_tracing.Rank = rank;
        voxel_cone_tracing.World = gpus;
        // (VCT_DEMO_SINGLE_DEVICE=1: every rank on device 0 -- only the direct-slab mode, VCT_COMM_MODE=direct, accepts that;
        // it is how that mode is tested on a one-GPU box)
        voxel_cone_tracing.Device = getenv("VCT_DEMO_SINGLE_DEVICE") ? 0 : rank;
        const std::string tmp = std::string(idfile) + ".tmp";
        if (rank == 0) {                                    // create the RCCL id, publish it atomically
            if (vct_comm_get_unique_id(voxel_cone_tracing.CommId) != VCT_OK) { printf("%s\n", vct_last_error(nullptr)); return 6; }
            FILE* fp = fopen(tmp.c_str(), "wb");
            if (!fp || fwrite(voxel_cone_tracing.CommId, 1, VCT_COMM_ID_BYTES, fp) != VCT_COMM_ID_BYTES) return 6;
            fclose(fp);
            rename(tmp.c_str(), idfile);
        } else {
            FILE* fp = nullptr;
            for (int tries = 0; tries < 6000 && !(fp = fopen(idfile, "rb")); ++tries) usleep(10000);
            if (!fp || fread(voxel_cone_tracing.CommId, 1, VCT_COMM_ID_BYTES, fp) != VCT_COMM_ID_BYTES) return 6;
            fclose(fp);
        }
    }
    voxel_cone_tracing.init_voxel_cone_tracing();           // R/main.cpp:68
    if (voxel_cone_tracing.last_status != VCT_OK) return 2;

    if (emission) {                                         // --emission: per-material overrides, picked up by the first Render()
        for (const char* q = emission; *q;) {
            int m = -1, used = 0;
            float r = 0.0f, g = 0.0f, b = 0.0f;
            if (sscanf(q, "%d=%f,%f,%f%n", &m, &r, &g, &b, &used) != 4 || !voxel_cone_tracing.SetEmission(m, r, g, b)) {
                fprintf(stderr, "--emission: MATERIAL=R,G,B[;...] with material indices below %zu (at '%s')\n",
                        voxel_cone_tracing.Emission.size() / 3, q);
                return 1;
            }
            q += used;
            if (*q == ';') ++q;
            else if (*q) { fprintf(stderr, "--emission: ';' expected at '%s'\n", q); return 1; }
        }
    }

    if (!gloss_classes.empty()) {                           // picked up by the first Render()
        voxel_cone_tracing.SetGlossClasses(gloss_classes.data(), gloss_classes.size());
        for (const std::pair<int, int>& g : gloss_of)
            if (!voxel_cone_tracing.SetGloss(g.first, g.second)) {
                fprintf(stderr, "--gloss: material %d: the scene has %zu materials\n", g.first, voxel_cone_tracing.Gloss.size());
                return 1;
            }
    }

    if (sky_gradient_arg || sky_sh_arg) voxel_cone_tracing.SetSky(sky_sh);      // picked up by the first Render()
    if (!lights.empty()) voxel_cone_tracing.SetLights(lights.data(), lights.size());

    // --dynamic-obj: the object's positions for every frame of the run (an update is asynchronous: each frame's array
    // stays where it is until the run has finished), attached at the first
    // --dynamic-spin: no arrays -- the OBJ's own positions are the rest positions of one part, and a frame is 12 floats
    // (one matrix per frame of the run, for the same reason); --dynamic-bend: the same with two matrices per frame
    std::vector<std::vector<float>> dyn_frames;
    const size_t dyn_nframes = (size_t)(frames > 1 ? frames : 1);
    const size_t dyn_stride = dyn_nmatrices * 12;
    std::vector<float> dyn_matrices(dyn_by_matrix ? dyn_nframes * dyn_stride : 0);
    if (dynamic_obj) {
        for (size_t f = 0; f * dyn_stride < dyn_matrices.size(); ++f) {
            const double t = dyn_nframes > 1 ? (double)f / (double)(dyn_nframes - 1) : 0.0;
            double move[3];
            for (int k = 0; k < 3; ++k) move[k] = (double)dyn_path[0][k] + t * ((double)dyn_path[1][k] - (double)dyn_path[0][k]);
            float* m = &dyn_matrices[f * dyn_stride];
            if (dynamic_bend) { vct_demo_spin_matrix(spin_axis, 0.0, spin_centre, move, m); m += 12; }      // bone 0 does not turn
            vct_demo_spin_matrix(spin_axis, (double)f * spin_deg, spin_centre, move, m);
        }
        dyn_frames.resize(dyn_by_matrix ? 0 : dyn_nframes);
        for (size_t f = 0; f < dyn_frames.size(); ++f) {
            const float t = dyn_frames.size() > 1 ? (float)f / (float)(dyn_frames.size() - 1) : 0.0f;
            dyn_frames[f] = dyn_pos;
            for (size_t i = 0; i < dyn_frames[f].size(); ++i)
                dyn_frames[f][i] += dyn_path[0][i % 3] + t * (dyn_path[1][i % 3] - dyn_path[0][i % 3]);
        }
        const float* first = dyn_by_matrix ? dyn_pos.data() : dyn_frames[0].data();
        if (!voxel_cone_tracing.SetDynamicMesh(first, dyn_material.data(), dyn_ntri, dyn_albedo.data(), dyn_nmat)) return 3;
        if (dynamic_spin) {
            const std::vector<int32_t> one_part((size_t)dyn_ntri, 0);
            if (!voxel_cone_tracing.SetDynamicParts(one_part.data(), 1)) return 3;
        }
        if (dynamic_bend) {
            std::vector<int32_t> bone;
            std::vector<float> weight;
            vct_demo_bend_influences(dyn_pos.data(), (size_t)dyn_ntri, dyn_lo, dyn_hi, bone, weight);
            if (!voxel_cone_tracing.SetDynamicSkin(bone.data(), weight.data(), 2)) return 3;
        }
        // in the space of the positions just attached -- the rest positions of the part or the skin
        if (dynamic_smooth && !voxel_cone_tracing.SetDynamicNormals(dyn_normals.data())) return 3;
        // the OBJ's Ke with --dynamic-emission over it (an all-zero table attaches nothing)
        if (!voxel_cone_tracing.SetDynamicEmission(dyn_emission.data(), (size_t)dyn_nmat)) return 3;
        if (dyn_draw_flags && !voxel_cone_tracing.DrawDynamicMesh((dyn_draw_flags & VCT_DYNAMIC_DRAW_SHADOW) != 0,
                                                                  (dyn_draw_flags & VCT_DYNAMIC_DRAW_GBUFFER) != 0)) return 3;
    }
    auto move_dynamic = [&](int f) {                        // frame f's positions, before its Render()
        if (!dynamic_obj) return true;
        if (dyn_by_matrix) {
            if (!voxel_cone_tracing.UpdateDynamicTransforms(&dyn_matrices[((size_t)f % dyn_nframes) * dyn_stride])) return false;
        } else if (!voxel_cone_tracing.UpdateDynamicMesh(dyn_frames[(size_t)f % dyn_frames.size()].data())) return false;
        if (bounces >= 2) {                                 // Render() is no whole pass then: the maps follow the object here
            voxel_cone_tracing.DrawDepthTexture();
            voxel_cone_tracing.DrawVoxelTexture();
        }
        return voxel_cone_tracing.last_status == VCT_OK;
    };

    float delta_time = 0.05f;
    if (!move_dynamic(0)) return 3;
    voxel_cone_tracing.Render();                            // frame 0 pays first-launch costs
    voxel_cone_tracing.Finish();
    if (voxel_cone_tracing.last_status != VCT_OK) return 3;
    // R/main.cpp:77-94 as written: Render() per frame, nothing read back (the reference swaps buffers instead)
    auto t0 = std::chrono::steady_clock::now();
    for (int f = 1; f < frames; ++f) {
        camera.ProcessKeyBoard(FORWARD, delta_time);
        if (!move_dynamic(f)) return 3;
        voxel_cone_tracing.Render();
        if (voxel_cone_tracing.last_status != VCT_OK) return 3;
    }
    voxel_cone_tracing.Finish();
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // the same number of frames with the RGBA16F frame copied to the host after every Render() (a presenter without
    // GPU interop): what the per-frame download costs
    double readback_ms = 0.0;
    if (frames > 1 && gpus <= 0) {
        const vec3 keep = camera.position;
        auto t1 = std::chrono::steady_clock::now();
        for (int f = 1; f < frames; ++f) {
            if (!move_dynamic(f)) return 3;
            voxel_cone_tracing.Render();
            if (!voxel_cone_tracing.Frame()) return 3;
        }
        readback_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        camera.position = keep;
    }
    if (gpus > 0 && rank != 0) { voxel_cone_tracing.Frame(); return 0; }       // the frame lives on rank 0
    if (gpus > 0) printf("gpus=%d (screen-tile slabs + one ncclGather per frame)\n", gpus);
    if (frames > 1) {
        printf("Render(): %.3f ms per frame (wall, %d frames, frame 0 excluded, no read-back, %d frame%s in flight)\n", wall_ms / (frames - 1), frames - 1,
               voxel_cone_tracing.FramesInFlight, voxel_cone_tracing.FramesInFlight == 1 ? "" : "s");
        if (gpus <= 0) printf("Render() + Frame(): %.3f ms per frame (frame copied to the host every frame)\n", readback_ms / (frames - 1));
    }
    // the facade issues its frames without timing events; the last frame once more with them, for the trace_ms below
    // (the camera has not moved since: the same frame)
    // (single GPU only: a rank's Render() is a collective step, and the other ranks are done)
    if (gpus <= 0) {
        vct_set_trace_timing(voxel_cone_tracing.ctx, 1);
        if (!move_dynamic(frames > 1 ? frames - 1 : 0)) return 3;
        voxel_cone_tracing.Render();
        if (voxel_cone_tracing.last_status != VCT_OK) return 3;
    }
    const uint16_t* fr = voxel_cone_tracing.Frame();
    const size_t n = (size_t)w * h * 4;
    uint64_t sum = 1469598103934665603ull;                  // FNV-1a over the RGBA16F halves
    for (size_t i = 0; i < n; ++i) { sum ^= fr[i]; sum *= 1099511628211ull; }
    uint64_t steps = 0;
    float ms = 0.0f, view_ms = 0.0f;
    if (show_voxels) {                                      // a view marches no cones
        vct_last_voxel_view_ms(voxel_cone_tracing.ctx, &view_ms);
        printf("voxel view: source=%d level=%d view_ms=%.3f\n", view_source, view_level, view_ms);
    } else {
        vct_last_step_count(voxel_cone_tracing.ctx, &steps);
        if (gpus <= 0) vct_last_trace_ms(voxel_cone_tracing.ctx, &ms);      // (a rank's slab steps were not timed: 0)
    }
    printf("frames=%d size=%dx%d voxels=%d cone_steps=%llu trace_ms=%.3f fnv1a=%016llx\n", frames, w, h,
           voxels, (unsigned long long)steps, ms, (unsigned long long)sum);
    if (dynamic_obj) {                                      // what the last frame's pass made of the object
        int32_t info[8] = {};
        float dyn_ms[2] = {0.0f, 0.0f};
        if (vct_get_dynamic(voxel_cone_tracing.ctx, info) != VCT_OK || vct_last_dynamic_ms(voxel_cone_tracing.ctx, dyn_ms) != VCT_OK) {
            printf("%s\n", vct_last_error(voxel_cone_tracing.ctx));
            return 3;
        }
        printf("dynamic mesh: triangles=%d bricks=%d of %d fragments=%d skipped=%d left_out=%d voxelize_ms=%.4f merge_ms=%.4f\n",
               (int)info[0], (int)info[4], (int)info[2], (int)info[5], (int)info[6], (int)info[7], dyn_ms[0], dyn_ms[1]);
    }
    if (reimport && gpus <= 0 && !show_voxels) {
        // the renderer "that brings its own G-buffer": the rasterised planes, packed as a deferred renderer keeps them
        const size_t npix = (size_t)w * h;
        const std::vector<uint16_t> native(fr, fr + n);
        std::vector<float> planes(npix * VCT_GB_PLANES);
        if (vct_download_gbuffer(voxel_cone_tracing.ctx, planes.data()) != VCT_OK) return 7;
        vct_config cfg;
        vct_get_config(voxel_cone_tracing.ctx, &cfg);
        std::vector<float> position(npix * 3);
        std::vector<uint16_t> normal(npix * 4), shading(npix * 4);
        std::vector<uint8_t> albedo(npix * 4), specular(npix * 4);
        for (size_t i = 0; i < npix; ++i) {
            for (int c = 0; c < 3; ++c) {
                position[i * 3 + c] = planes[(VCT_GB_POSITION + c) * npix + i];
                normal[i * 4 + c] = float_to_half(planes[(VCT_GB_NORMAL + c) * npix + i]);
                shading[i * 4 + c] = float_to_half(planes[(VCT_GB_BUMP_N + c) * npix + i]);
                specular[i * 4 + c] = float_to_unorm8(planes[(VCT_GB_SPECULAR + c) * npix + i]);
            }
            for (int c = 0; c < 4; ++c) albedo[i * 4 + c] = float_to_unorm8(planes[(VCT_GB_ALBEDO + c) * npix + i]);
            normal[i * 4 + 3] = shading[i * 4 + 3] = 0;
            specular[i * 4 + 3] = 255;
        }
        vct_gbuffer_import in;
        memset(&in, 0, sizeof in);
        in.position = position.data(); in.position_format = VCT_IMPORT_POSITION_F32X3;
        in.normal = normal.data(); in.shading_normal = shading.data(); in.normal_format = VCT_IMPORT_NORMAL_F16X4;
        in.albedo = albedo.data(); in.albedo_format = VCT_IMPORT_COLOR_UNORM8X4;
        in.specular = specular.data(); in.specular_format = VCT_IMPORT_COLOR_UNORM8X4;
        in.shadow = planes.data() + (size_t)VCT_GB_SHADOW * npix;
        in.location = VCT_MEM_HOST;
        in.normal_scale = cfg.model_scale;                  // the length the raster gives planes 3-11 (ModelMatrix = scale)
        voxel_cone_tracing.ImportGBuffer(in);
        if (voxel_cone_tracing.last_status != VCT_OK) return 3;
        const uint16_t* again = voxel_cone_tracing.Frame();
        if (!again) return 3;
        double num = 0.0, den = 0.0;
        for (size_t i = 0; i < n; ++i) {
            const double a = half_to_float(again[i]), b = half_to_float(native[i]);
            if (!(fabs(a) < INFINITY) || !(fabs(b) < INFINITY)) continue;
            num += (a - b) * (a - b); den += b * b;
        }
        float import_ms = 0.0f;
        vct_last_gbuffer_import_ms(voxel_cone_tracing.ctx, &import_ms);
        printf("reimport: position f32x3, normals f16x4, colours unorm8: frame relative L2 %.3e against the rasterised G-buffer, import_ms=%.3f\n",
               den > 0.0 ? sqrt(num / den) : 0.0, import_ms);
        fr = again;
    }
    if (cubes_file && gpus <= 0) {
        // the irradiance-volume use of the point queries: probes at the cell centres of a grid over the scene's bounds
        Model& model = voxel_cone_tracing.model;
        const int32_t ntri = vcth_scene_num_triangles(model.scene), nmat = vcth_scene_num_materials(model.scene);
        std::vector<float> pos((size_t)ntri * 9), albedo((size_t)nmat * 4), specular((size_t)nmat * 3);
        std::vector<int32_t> material((size_t)ntri);
        vcth_scene_get(model.scene, pos.data(), material.data(), albedo.data(), specular.data());
        vct_config cfg;
        vct_get_config(voxel_cone_tracing.ctx, &cfg);
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t i = 0; i < pos.size(); ++i) {
            const float v = pos[i] * cfg.model_scale;
            lo[i % 3] = fminf(lo[i % 3], v); hi[i % 3] = fmaxf(hi[i % 3], v);
        }
        std::vector<vct_gather_point> pts;
        for (int z = 0; z < cubes[2]; ++z)
            for (int y = 0; y < cubes[1]; ++y)
                for (int x = 0; x < cubes[0]; ++x)
                    for (int face = 0; face < 6; ++face) {
                        vct_gather_point p;
                        const int cell[3] = {x, y, z};
                        for (int a = 0; a < 3; ++a) {
                            p.position[a] = lo[a] + (hi[a] - lo[a]) * ((float)cell[a] + 0.5f) / (float)cubes[a];
                            p.normal[a] = a == face / 2 ? (face & 1 ? -1.0f : 1.0f) : 0.0f;      // unit: the cones start one voxel off the probe
                        }
                        vcth_frame_from_normal(p.normal, 1.0f, p.tangent, p.bitangent);
                        pts.push_back(p);
                    }
        std::vector<float> out(pts.size() * 4);
        if (!voxel_cone_tracing.GatherPoints(pts.data(), (int32_t)pts.size(), out.data())) return 7;
        uint64_t q[4] = {0, 0, 0, 0};
        float qms = 0.0f;
        vct_last_point_query(voxel_cone_tracing.ctx, q);
        vct_last_point_query_ms(voxel_cone_tracing.ctx, &qms);
        printf("ambient cubes: %dx%dx%d probes, %llu gathers, cone_steps=%llu march_ms=%.3f\n", cubes[0], cubes[1], cubes[2],
               (unsigned long long)q[0], (unsigned long long)q[1], qms);
        FILE* fp = fopen(cubes_file, "wb");
        if (!fp || fwrite(out.data(), sizeof(float), out.size(), fp) != out.size()) return 4;
        fclose(fp);
        fp = fopen((std::string(cubes_file) + ".points").c_str(), "wb");
        if (!fp || fwrite(pts.data(), sizeof(vct_gather_point), pts.size(), fp) != pts.size()) return 4;
        fclose(fp);
    }
    if (chain_file && gpus <= 0) {
        vct_config cfg;
        vct_get_config(voxel_cone_tracing.ctx, &cfg);
        std::vector<uint8_t> chain(vct_chain_texels(cfg.voxel_dim) * 4);
        if (vct_download_chain_rgba8(voxel_cone_tracing.ctx, chain.data()) != VCT_OK) return 7;
        FILE* fp = fopen(chain_file, "wb");
        if (!fp || fwrite(chain.data(), 1, chain.size(), fp) != chain.size()) return 4;
        fclose(fp);
    }
    if (ppm) {
        FILE* fp = fopen(ppm, "wb");
        if (!fp) return 4;
        fprintf(fp, "P6\n%d %d\n255\n", w, h);
        for (int y = h - 1; y >= 0; --y)            // row 0 is the bottom row of the GL window
            for (int x = 0; x < w; ++x) {
                unsigned char px[3];
                for (int c = 0; c < 3; ++c) {
                    float v = half_to_float(fr[((size_t)y * w + x) * 4 + c]);
                    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
                    px[c] = (unsigned char)(powf(v, 1.0f / 2.2f) * 255.0f + 0.5f);
                }
                fwrite(px, 1, 3, fp);
            }
        fclose(fp);
    }
    return 0;
}
