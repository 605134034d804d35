#!/usr/bin/env python3
"""Generates tests/golden/ref_shader_text.npz: what the reference's shader TEXT computes, run as C++.

Where the reference tree is present only.  The cone-trace fragment shader (S/VoxelConeTracing.fs) and the voxelization
geometry / fragment shaders (S/Voxelization.gs / .fs) are read at run time -- never stored in this repository --,
rewritten mechanically into C++ (qualifiers dropped, GLSL array constructors -> braces, multi-component swizzles -> calls,
`discard` -> a flag) and compiled against tests/glsl_shim.h, a minimal GLSL stand-in; `textureLod` under the shader is
the oracle's own sampler (oracle/libvct_oracle.so), the material / height / shadow samplers are per-pixel constants.
Their `main()` then runs on seeded inputs (trace_inputs / vox_inputs below, which tests/test_shader_crosscheck.py
regenerates) and the fixture keeps what the shaders produced:

  trace_V{32,64}   colour [n][4], executed steps per cone [n][7] (-1 in cone 0: more than 7 cones), discard flag [n],
                   and the G-buffer columns the shader derives itself (bump normal 12-14, resolved specular 19-21, PCF
                   shadow term 22) that the oracle is fed as inputs
  vox_gs           dominant axis [n], clip positions [n][3][4] of 20,000 triangles
  vox_fs_V{64,256} voxel index [m][3] and stored value [m][4] of 6,000 fragments

The arrays are stored losslessly but compactly (encode / load_fixture): where a simple prediction from the seeded
inputs exists (clip position = the stored projection matrix times the vertex, bump normal of a flat height map, stored
value = albedo x k / 25, ...), the file keeps the difference of the float32 BIT PATTERNS from it -- zero wherever the
prediction is exact, whatever it is elsewhere -- and load_fixture adds it back: bit-identical arrays, independent of
the oracle under test.

    python tests/golden/make_shader_golden.py            # rewrites tests/golden/ref_shader_text.npz
    python tests/golden/make_shader_golden.py --check    # regenerates in memory and compares with the committed file
"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

GOLDEN = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
OUT = os.path.join(GOLDEN, "ref_shader_text.npz")
from oracle.pyrefgl import SHADER_DIR as SHADERS       # noqa: E402 -- the reference's Shader/ (VCT_REFERENCE_SHADERS)
REF_FS = os.path.join(SHADERS, "VoxelConeTracing.fs")
REF_VOX_FS = os.path.join(SHADERS, "Voxelization.fs")
REF_VOX_GS = os.path.join(SHADERS, "Voxelization.gs")
ORACLE = os.path.join(ROOT, "oracle", "libvct_oracle.so")
TRACE_CASES = ((32, 11), (64, 12))          # (V, seed)
VOX_FS_CASES = ((64, 64), (256, 128))       # (V, shadow map size)
GB_SHADER_COLS = [12, 13, 14, 19, 20, 21, 22]


# ---- seeded inputs (tests/test_shader_crosscheck.py regenerates them) -----------------------------------------------
def trace_inputs(V, seed, n=5000):
    """Volume, its mip chain, a random G-buffer [n][23], raw specular texels [n][4], PCF pass counts [n]."""
    import synth
    from oracle import pyoracle
    l0 = synth.noise_volume(V, seed=seed)
    chain = np.ascontiguousarray(pyoracle.build_mips(l0))
    planes = synth.random_gbuffer(n, seed=seed, discard_frac=0.05)           # [23][n]
    gb = np.ascontiguousarray(planes.T.astype(np.float32))                   # [n][23]
    rng = np.random.default_rng(seed)
    spec_raw = rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32)
    spec_raw[rng.random(n) < 0.3, 1:3] = 0.0                                 # red-only maps: the .rrra rule (trace.fs:210)
    shadow_k = rng.integers(0, 26, n).astype(np.int32)
    return chain, gb, spec_raw, shadow_k


def vox_inputs():
    """Triangles [n][9] for the geometry stage, then per VOX_FS_CASES (V, S, shadow depth [S][S], fragments [m][8],
    albedo [m][4]) -- all drawn from one generator, in this order."""
    rng = np.random.default_rng(5)
    n = 20000
    tri = rng.uniform(-70.0, 70.0, (n, 9)).astype(np.float32)
    tri[: n // 4, 3:] = tri[: n // 4, :3].repeat(2).reshape(-1, 3, 2).transpose(0, 2, 1).reshape(-1, 6) \
        + rng.uniform(-2.0, 2.0, (n // 4, 6)).astype(np.float32)                    # a quarter small triangles
    # axis-aligned ones: ties between the components of the normal (vox.gs:34-39 resolves them X, then Y, then Z)
    tri[n // 4: n // 4 + 300] = np.round(tri[n // 4: n // 4 + 300] / 8.0) * 8.0
    frags = []
    for V, S in VOX_FS_CASES:
        m = 6000
        # a shadow map with structure at every scale: blocks of depth + noise, so that windows straddle edges
        depth = (rng.integers(0, 4, (S // 8, S // 8)).repeat(8, 0).repeat(8, 1) * 0.2 + 0.1
                 + rng.uniform(0.0, 0.02, (S, S))).astype(np.float32)
        frag = np.zeros((m, 8), np.float32)
        frag[:, 0] = rng.integers(0, V, m) + 0.5                               # pixel centres of the V x V voxelization raster
        frag[:, 1] = rng.integers(0, V, m) + 0.5
        frag[:, 2] = rng.uniform(0.0, 1.0, m)
        frag[: m // 20, 2] = rng.integers(0, V, m // 20) / np.float32(V)       # depths on voxel boundaries
        frag[:, 3] = rng.integers(1, 4, m)
        frag[:, 4:6] = rng.uniform(-0.05, 1.05, (m, 2))                        # shadow coordinates, some past the rim (clamp to edge)
        frag[:, 6] = rng.uniform(0.0, 1.0, m)
        albedo = rng.uniform(0.0, 1.0, (m, 4)).astype(np.float32)
        frags.append((V, S, depth, frag, albedo))
    return tri, frags


def voxel_proj(lib, G=150.0):
    proj = np.zeros((3, 16), np.float32)
    lib.vcto_voxel_proj.argtypes = [C.c_float, C.c_int, C.c_void_p]
    for a in range(3):
        lib.vcto_voxel_proj(C.c_float(G), a + 1, proj[a].ctypes.data_as(C.c_void_p))
    return proj


# ---- the shader text as C++ -----------------------------------------------------------------------------------------
HARNESS = r'''
ShimState g_shim;
}  // namespace glsl
extern "C" int vcto_shade_pixel(const void* p, const unsigned char* chain, const float gb[23], float out[4],
                                unsigned char steps[7], float cones[28]);
using namespace glsl;
// gbin [n][23] (bump normal slots ignored: CalcBumpNormal of the shader fills them), spec_raw [n][4], shadow_k [n];
// outputs: shader colour [n][4], oracle colour [n][4], steps of both [n][7], the G-buffer as fed to the oracle [n][23]
extern "C" int run_pixels(const void* params, const unsigned char* chain, int V, float G, const float cam[3],
                          const float light[3], float ambient, float shininess, int n, const float* gbin,
                          const float* spec_raw, const int* shadow_k, float* out_shader, float* out_oracle,
                          int* steps_shader, int* steps_oracle, float* gb_used, int* discarded) {
    VoxelGridWorldSize = G; VoxelDimensions = V; ambientFactor = ambient; Shininess = shininess; Opacity = 1.0f;
    LightDirection = vec3(light[0], light[1], light[2]);
    ShadowMapSize = 4096; HeightTextureSize = vec2(64.0, 64.0);
    DiffuseTexture.which = 0; SpecularTexture.which = 1; MaskTexture.which = 2; HeightTexture.which = 3; ShadowMap.which = 4;
    for (int i = 0; i < n; ++i) {
        const float* g = gbin + 23 * i;
        Position_world = vec3(g[0], g[1], g[2]);
        Normal_world = vec3(g[3], g[4], g[5]);
        Tangent_world = vec3(g[6], g[7], g[8]);
        BiTangent_world = vec3(g[9], g[10], g[11]);
        CameraDirection_world = vec3(cam[0], cam[1], cam[2]) - Position_world;      // trace.vs:34
        Position_depth = vec4(0.5, 0.5, 0.5, 1.0);
        tex = vec2(0.25, 0.75);
        g_shim = ShimState();
        g_shim.params = params; g_shim.chain = chain;
        g_shim.diffuse = vec4(g[15], g[16], g[17], g[18]);
        g_shim.specular = vec4(spec_raw[4 * i], spec_raw[4 * i + 1], spec_raw[4 * i + 2], spec_raw[4 * i + 3]);
        g_shim.height = 0.5f;
        g_shim.shadow_pass = shadow_k[i];
        color = vec4(-1.0);
        shader_main();
        discarded[i] = g_shim.discarded ? 1 : 0;
        out_shader[4 * i] = color.x; out_shader[4 * i + 1] = color.y; out_shader[4 * i + 2] = color.z; out_shader[4 * i + 3] = color.w;
        for (int k = 0; k < 7; ++k) steps_shader[7 * i + k] = g_shim.cone_steps[k];
        if (g_shim.ncones > 7) steps_shader[7 * i] = -1;
        // the oracle's G-buffer: the same pixel with the shader's own bump normal, the resolved specular colour
        // (trace.fs:210) and the shader's shadow term as INPUTS (SURVEY.md 8 a5)
        float gb[23];
        for (int k = 0; k < 23; ++k) gb[k] = g[k];
        const mat3 TBN = inverse(transpose(mat3(Tangent_world, BiTangent_world, Normal_world)));
        const vec3 N = CalcBumpNormal(TBN);
        gb[12] = N.x; gb[13] = N.y; gb[14] = N.z;
        const vec4 sp = g_shim.specular;
        const bool has_gb = length(sp.gb()) > 0.0f;
        gb[19] = sp.x; gb[20] = has_gb ? sp.y : sp.x; gb[21] = has_gb ? sp.z : sp.x;
        g_shim.shadow_calls = 0;
        gb[22] = PCF_Shadow_Mapping(0.002f);
        for (int k = 0; k < 23; ++k) gb_used[23 * i + k] = gb[k];
        unsigned char st[7];
        vcto_shade_pixel(params, chain, gb, out_oracle + 4 * i, st, nullptr);
        for (int k = 0; k < 7; ++k) steps_oracle[7 * i + k] = st[k];
    }
    return 0;
}
'''


def glsl_to_cpp(src):
    """The mechanical rewrites; anything else in the text is compiled as it stands."""
    out = []
    for line in src.splitlines():
        if line.lstrip().startswith("#version"):
            continue
        line = re.sub(r"^\s*(in|out|uniform)\s+", "", line)                  # storage qualifiers -> plain globals
        out.append(line)
    s = "\n".join(out)
    s = re.sub(r"=\s*float\[\]\s*\(([^;]*)\)\s*;", r"= {\1};", s)           # float[](...)  -> {...}
    s = re.sub(r"=\s*vec3\[\]\s*\(([^;]*)\)\s*;", r"= {\1};", s, flags=re.S)  # vec3[](...)   -> {...}
    s = re.sub(r"\.(rgb|gb|rrra|xy)\b", r".\1()", s)                        # multi-component swizzles (reads only)
    s = re.sub(r"\bdiscard\s*;", "{ g_shim.discarded = true; return; }", s)
    s = re.sub(r"\bvoid\s+main\s*\(\s*\)", "void shader_main()", s)
    # instrumentation: count the textureLod calls of each Voxel_Cone_Tracing invocation (= its executed steps)
    s, k = re.subn(r"(vec4\s+Voxel_Cone_Tracing\s*\([^)]*\)\s*\{)", r"\1 shim_cone_begin();", s)
    assert k == 1
    return s


VOX_FS_HARNESS = r'''
ShimState g_shim;
}  // namespace glsl
using namespace glsl;
// frag [n][8]: gl_FragCoord x y z, axis, DepthCoord x y z, (pad); albedo [n][4]; out: voxel [n][3], value [n][4]
extern "C" int run_fragments(int V, int S, const float* depth, int n, const float* frag, const float* albedo, int* voxel,
                             float* value) {
    VoxelDimensions = V; ShadowMapSize = S;
    DiffuseTexture.which = 0; ShadowMap.which = 4;
    for (int i = 0; i < n; ++i) {
        const float* f = frag + 8 * i;
        g_shim = ShimState();
        g_shim.shadow_depth = depth; g_shim.shadow_S = S;
        g_shim.diffuse = vec4(albedo[4 * i], albedo[4 * i + 1], albedo[4 * i + 2], albedo[4 * i + 3]);
        gl_FragCoord = vec4(f[0], f[1], f[2], 1.0);
        gs.axis = (int)f[3];
        gs.DepthCoord = vec4(f[4], f[5], f[6], 1.0);          // an orthographic light: w = 1 (vox.vs:18-19)
        gs.TexCoord = vec2(0.25, 0.75);
        shader_main();
        if (g_shim.stores != 1) return 1 + i;
        voxel[3 * i] = g_shim.stored_pos.x; voxel[3 * i + 1] = g_shim.stored_pos.y; voxel[3 * i + 2] = g_shim.stored_pos.z;
        value[4 * i] = g_shim.stored_value.x; value[4 * i + 1] = g_shim.stored_value.y;
        value[4 * i + 2] = g_shim.stored_value.z; value[4 * i + 3] = g_shim.stored_value.w;
    }
    return 0;
}
'''

VOX_GS_HARNESS = r'''
ShimState g_shim;
static int g_emitted;
static float g_out[3][4];
static int g_axis_out;
void EmitVertex() { if (g_emitted < 3) { g_out[g_emitted][0] = gl_Position.x; g_out[g_emitted][1] = gl_Position.y;
                                        g_out[g_emitted][2] = gl_Position.z; g_out[g_emitted][3] = gl_Position.w; }
                    g_axis_out = axis; ++g_emitted; }
void EndPrimitive() {}
void shader_main();
}  // namespace glsl
using namespace glsl;
// tri [n][9] world-space positions; proj [3][16] column-major ProjX / ProjY / ProjZ; out: axis [n], clip [n][3][4]
extern "C" int run_triangles(const float* proj, int n, const float* tri, int* axis_out, float* clip) {
    mat4* P[3] = {&ProjX, &ProjY, &ProjZ};
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 4; ++c) P[a]->c[c] = vec4(proj[16 * a + 4 * c], proj[16 * a + 4 * c + 1], proj[16 * a + 4 * c + 2], proj[16 * a + 4 * c + 3]);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) gl_in[k].gl_Position = vec4(tri[9 * i + 3 * k], tri[9 * i + 3 * k + 1], tri[9 * i + 3 * k + 2], 1.0);
        g_emitted = 0;
        shader_main();
        if (g_emitted != 3) return 1 + i;
        axis_out[i] = g_axis_out;
        for (int k = 0; k < 3; ++k) for (int c = 0; c < 4; ++c) clip[12 * i + 4 * k + c] = g_out[k][c];
    }
    return 0;
}
'''


def vox_glsl_to_cpp(src, geometry):
    """Mechanical rewrites for the two voxelization stages: layout qualifiers and `flat` dropped, interface blocks ->
    a struct instance (named block) or plain globals (unnamed block), swizzles -> calls, `.r` of a fetch -> `.x`."""
    s = "\n".join(ln for ln in src.splitlines() if not ln.lstrip().startswith("#version"))
    s = re.sub(r"^\s*layout\s*\([^)]*\)\s*(in|out)\s*;", "", s, flags=re.M)           # layout (triangles) in;
    s = re.sub(r"layout\s*\([^)]*\)\s*", "", s)                                        # uniform layout(RGBA8) image3D ...
    s = re.sub(r"\bflat\s+", "", s)
    if geometry:
        s = re.sub(r"^\s*in\s+Vertex\s*\{([^}]*)\}\s*vertices\s*\[\s*\]\s*;", r"struct Vertex {\1} vertices[3];", s, flags=re.M)
        s = re.sub(r"^\s*out\s+Vertex_GS\s*\{([^}]*)\}\s*;", r"\1", s, flags=re.M)  # unnamed block: its members are globals
        s = "GlInArray gl_in; vec4 gl_Position; void EmitVertex(); void EndPrimitive();\n" + s
    else:
        s = re.sub(r"^\s*in\s+Vertex_GS\s*\{([^}]*)\}\s*gs\s*;", r"struct Vertex_GS {\1} gs;", s, flags=re.M)
        s = "vec4 gl_FragCoord;\n" + s
    s = re.sub(r"^\s*(in|out|uniform)\s+", "", s, flags=re.M)
    s = re.sub(r"\.(xyz|xy|rgb)\b", r".\1()", s)
    s = re.sub(r"\)\.r\b", ").x", s)
    s = re.sub(r"\bvoid\s+main\s*\(\s*\)", "void shader_main()", s)
    return s


def _build(tmp, name, text):
    cpp = os.path.join(tmp, name + ".cpp")
    with open(cpp, "w") as fh:
        fh.write(f'#include "{ROOT}/tests/glsl_shim.h"\nnamespace glsl {{\n' + text)
    so = os.path.join(tmp, "lib" + name + ".so")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-o", so, cpp,
                        ORACLE, f"-Wl,-rpath,{os.path.dirname(ORACLE)}"], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr[-4000:])
    return C.CDLL(so)


def generate(tmp):
    from oracle import pyoracle
    out = {}
    with open(REF_FS) as fh:
        lib = _build(tmp, "shader_gen", glsl_to_cpp(fh.read()) + HARNESS)
    for V, seed in TRACE_CASES:
        chain, gb, spec_raw, shadow_k = trace_inputs(V, seed)
        n = gb.shape[0]
        p = pyoracle.default_params(V)
        outs = np.zeros((n, 4), np.float32); outo = np.zeros((n, 4), np.float32)
        ss = np.zeros((n, 7), np.int32); so_ = np.zeros((n, 7), np.int32)
        gbu = np.zeros((n, 23), np.float32); disc = np.zeros(n, np.int32)
        cam = np.array(p.camera_pos, np.float32); light = np.array(p.light_dir, np.float32)
        rc = lib.run_pixels(C.byref(p), chain.ctypes.data_as(C.c_void_p), C.c_int(V), C.c_float(p.G),
                            cam.ctypes.data_as(C.c_void_p), light.ctypes.data_as(C.c_void_p), C.c_float(p.ambient_factor),
                            C.c_float(p.shininess), C.c_int(n), gb.ctypes.data_as(C.c_void_p),
                            spec_raw.ctypes.data_as(C.c_void_p), shadow_k.ctypes.data_as(C.c_void_p),
                            outs.ctypes.data_as(C.c_void_p), outo.ctypes.data_as(C.c_void_p),
                            ss.ctypes.data_as(C.c_void_p), so_.ctypes.data_as(C.c_void_p),
                            gbu.ctypes.data_as(C.c_void_p), disc.ctypes.data_as(C.c_void_p))
        assert rc == 0
        rest = [k for k in range(23) if k not in GB_SHADER_COLS]
        assert np.array_equal(gbu[:, rest].view(np.uint32), gb[:, rest].view(np.uint32))
        out[f"trace_V{V}_color"] = outs
        out[f"trace_V{V}_steps"] = ss.astype(np.int8)       # -1 .. 255 steps per cone never happen: int8 holds them
        out[f"trace_V{V}_discarded"] = disc.astype(np.uint8)
        out[f"trace_V{V}_gb_shader_cols"] = gbu[:, GB_SHADER_COLS]
    olib = C.CDLL(ORACLE)
    tri, frags = vox_inputs()
    n = tri.shape[0]
    with open(REF_VOX_GS) as fh:
        gs = _build(tmp, "vox_gs", vox_glsl_to_cpp(fh.read(), True) + VOX_GS_HARNESS)
    proj = voxel_proj(olib)
    axis_s = np.zeros(n, np.int32); clip = np.zeros((n, 3, 4), np.float32)
    rc = gs.run_triangles(proj.ctypes.data_as(C.c_void_p), C.c_int(n), tri.ctypes.data_as(C.c_void_p),
                          axis_s.ctypes.data_as(C.c_void_p), clip.ctypes.data_as(C.c_void_p))
    assert rc == 0
    out["vox_gs_axis"] = axis_s.astype(np.int8)
    out["vox_gs_proj"] = proj
    out["vox_gs_clip"] = clip
    with open(REF_VOX_FS) as fh:
        fs = _build(tmp, "vox_fs", vox_glsl_to_cpp(fh.read(), False) + VOX_FS_HARNESS)
    for V, S, depth, frag, albedo in frags:
        m = frag.shape[0]
        voxel = np.zeros((m, 3), np.int32); value = np.zeros((m, 4), np.float32)
        rc = fs.run_fragments(C.c_int(V), C.c_int(S), depth.ctypes.data_as(C.c_void_p), C.c_int(m),
                              frag.ctypes.data_as(C.c_void_p), albedo.ctypes.data_as(C.c_void_p),
                              voxel.ctypes.data_as(C.c_void_p), value.ctypes.data_as(C.c_void_p))
        assert rc == 0
        out[f"vox_fs_V{V}_voxel"] = voxel
        out[f"vox_fs_V{V}_value"] = value
    return out


# ---- compact, lossless storage -------------------------------------------------------------------------------------
def _delta(actual, predicted):
    """float32 bit pattern of `actual` minus that of `predicted` (wrapping): 0 where the prediction is exact."""
    a = np.ascontiguousarray(actual, np.float32).view(np.uint32)
    return (a - np.ascontiguousarray(predicted, np.float32).view(np.uint32)).view(np.int32)


def _undelta(delta, predicted):
    return (np.ascontiguousarray(predicted, np.float32).view(np.uint32) + delta.view(np.uint32)).view(np.float32)


def _gb_prediction(gb, spec_raw, shadow_k):
    """Columns 12-14: the flat-height bump normal, normalize(inverse(transpose(mat3(T, B, N))) * (0, 0, 1)) = the
    normalized cross(T, B) / det, in float64 by elementwise operations only (the same bits on every machine); 19-21: the
    specular texel (.rrra when its g and b are 0); 22: passes x 0.111."""
    t, b, n = (gb[:, c:c + 3].astype(np.float64) for c in (6, 9, 3))
    cr = np.stack([t[:, 1] * b[:, 2] - t[:, 2] * b[:, 1], t[:, 2] * b[:, 0] - t[:, 0] * b[:, 2],
                   t[:, 0] * b[:, 1] - t[:, 1] * b[:, 0]], axis=1)
    v = cr / (n[:, 0] * cr[:, 0] + n[:, 1] * cr[:, 1] + n[:, 2] * cr[:, 2])[:, None]
    v = v / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])[:, None]
    has_gb = (spec_raw[:, 1] != 0) | (spec_raw[:, 2] != 0)
    spec = np.where(has_gb[:, None], spec_raw[:, :3], spec_raw[:, :1])
    return np.concatenate([v.astype(np.float32), spec, (shadow_k.astype(np.float32) * np.float32(0.111))[:, None]], axis=1)


def _clip_prediction(proj, tri, axis):
    """Vertex k of triangle i through column-major ProjX / ProjY / ProjZ[axis - 1], summed left to right in float32."""
    m = proj[np.clip(axis.astype(np.int64), 1, 3) - 1]                     # [n][16]
    out = np.empty((tri.shape[0], 3, 4), np.float32)
    for k in range(3):
        x, y, z = tri[:, 3 * k], tri[:, 3 * k + 1], tri[:, 3 * k + 2]
        for r in range(4):
            out[:, k, r] = m[:, r] * x + m[:, 4 + r] * y + m[:, 8 + r] * z + m[:, 12 + r] * np.float32(1.0)
    return out


def _value_prediction(albedo, k):
    return np.concatenate([albedo[:, :3] * (k.astype(np.float32) / np.float32(25.0))[:, None],
                           np.ones((albedo.shape[0], 1), np.float32)], axis=1)


def encode(out):
    """The arrays of generate() -> what the fixture stores."""
    enc = {}
    for V, seed in TRACE_CASES:
        _, gb, spec_raw, shadow_k = trace_inputs(V, seed)
        for key in ("color", "steps", "discarded"):
            enc[f"trace_V{V}_{key}"] = out[f"trace_V{V}_{key}"]
        enc[f"trace_V{V}_gb_shader_cols_delta"] = _delta(out[f"trace_V{V}_gb_shader_cols"], _gb_prediction(gb, spec_raw, shadow_k))
    tri, frags = vox_inputs()
    enc["vox_gs_axis"], enc["vox_gs_proj"] = out["vox_gs_axis"], out["vox_gs_proj"]
    enc["vox_gs_clip_delta"] = _delta(out["vox_gs_clip"], _clip_prediction(out["vox_gs_proj"], tri, out["vox_gs_axis"]))
    for V, S, depth, frag, albedo in frags:
        voxel, value = out[f"vox_fs_V{V}_voxel"], out[f"vox_fs_V{V}_value"]
        assert voxel.min() >= 0 and voxel.max() < 256
        enc[f"vox_fs_V{V}_voxel"] = voxel.astype(np.uint8)
        # the PCF pass count whose prediction is closest (exact where the shader stores albedo * (count / 25))
        err = np.stack([np.abs(_value_prediction(albedo, np.full(len(value), k)) - value).sum(1) for k in range(26)], 1)
        k = err.argmin(1).astype(np.uint8)
        enc[f"vox_fs_V{V}_value_k"] = k
        enc[f"vox_fs_V{V}_value_delta"] = _delta(value, _value_prediction(albedo, k))
    return enc


def load_fixture(path=OUT):
    """The stored shader outputs, bit-identical to what generate() produced (keys as there)."""
    with np.load(path) as z:
        enc = {k: z[k] for k in z.files}
    out = {}
    for V, seed in TRACE_CASES:
        _, gb, spec_raw, shadow_k = trace_inputs(V, seed)
        for key in ("color", "steps", "discarded"):
            out[f"trace_V{V}_{key}"] = enc[f"trace_V{V}_{key}"]
        out[f"trace_V{V}_gb_shader_cols"] = _undelta(enc[f"trace_V{V}_gb_shader_cols_delta"],
                                                     _gb_prediction(gb, spec_raw, shadow_k))
    tri, frags = vox_inputs()
    out["vox_gs_axis"], out["vox_gs_proj"] = enc["vox_gs_axis"], enc["vox_gs_proj"]
    out["vox_gs_clip"] = _undelta(enc["vox_gs_clip_delta"], _clip_prediction(enc["vox_gs_proj"], tri, enc["vox_gs_axis"]))
    for V, S, depth, frag, albedo in frags:
        out[f"vox_fs_V{V}_voxel"] = enc[f"vox_fs_V{V}_voxel"].astype(np.int32)
        out[f"vox_fs_V{V}_value"] = _undelta(enc[f"vox_fs_V{V}_value_delta"], _value_prediction(albedo, enc[f"vox_fs_V{V}_value_k"]))
    return out


def main():
    check = "--check" in sys.argv[1:]
    for f in (REF_FS, REF_VOX_FS, REF_VOX_GS):
        if not os.path.exists(f):
            raise SystemExit(f"{f}: not found (the reference's shaders are needed to generate this fixture)")
    with tempfile.TemporaryDirectory() as tmp:
        out = generate(tmp)
    if check:
        got = load_fixture()
        bad = [k for k in out if k not in got or got[k].shape != out[k].shape
               or not np.array_equal(got[k].view(np.uint8), np.ascontiguousarray(out[k]).view(np.uint8))] + \
              [k for k in got if k not in out]
        if bad:
            raise SystemExit(f"{OUT}: differs in {bad}")
        print(f"{OUT}: identical")
        return
    enc = encode(out)
    np.savez_compressed(OUT, **enc)
    if any(not np.array_equal(v.view(np.uint8), np.ascontiguousarray(out[k]).view(np.uint8)) for k, v in load_fixture().items()):
        raise SystemExit("the stored form does not give back the generated arrays")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
