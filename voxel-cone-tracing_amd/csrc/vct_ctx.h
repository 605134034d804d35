// vct_ctx.h -- the context behind the C ABI (private to the library's translation units).
#ifndef VCT_CTX_H_
#define VCT_CTX_H_

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/vct.h"
#include "vct_feature_rules.h"
#include "vct_internal.h"
#include "vct_lights_check.h"

struct vct_comm;      // multi-GPU state (vct_multi.hip)

// A stream restricted to a range of the device's compute units (hipExtStreamCreateWithCUMask).  Used when
// VCT_COMM_RESERVED_CUS = k > 0 keeps the last k CUs away from the context's streams and hands exactly those to the
// multi-GPU step's communication stream: a running trace leaves another queue's kernels almost no wave slots
// (k_raster_mid 658 us instead of 60 beside a trace), and RCCL's gather kernel is such a queue.
hipError_t vct_create_masked_stream(hipStream_t* s, int device, int first_cu, int last_cu);

// Device memory with an owner.  Every buffer of the context is one of these, as a member of the struct whose lifetime
// it shares, so that dropping the struct (assigning a fresh one, leaving a scope on an error, delete) is what frees it:
// no list of pointers to keep in step.  size() counts elements.  Kernel parameter structs take get().
template <class T>
class VctBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    VctBuf() = default;
    VctBuf(const VctBuf&) = delete;
    VctBuf& operator=(const VctBuf&) = delete;
    VctBuf(VctBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    VctBuf& operator=(VctBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~VctBuf() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    hipError_t alloc(size_t n) {      // the old contents go first; a failure leaves the buffer empty
        reset();
        const hipError_t e = hipMalloc(&p_, n * sizeof(T));
        if (e == hipSuccess) n_ = n; else p_ = nullptr;
        return e;
    }
    // grow-only scratch: at least n elements, contents undefined after growing (*grew is set, never cleared)
    hipError_t reserve(size_t n, bool* grew = nullptr) {
        if (n <= n_) return hipSuccess;
        if (grew) *grew = true;
        return alloc(n);
    }
    // n elements allocated another way (fine-grained memory) that hipFree releases: owned from here on
    void adopt(T* p, size_t n) { reset(); p_ = p; n_ = n; }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// An event / a stream with an owner, like VctBuf.  Destroying a stream does not wait for it: whoever drops one with work in flight waits first.
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class VctHandle {
    H h_ = nullptr;

public:
    VctHandle() = default;
    VctHandle(const VctHandle&) = delete;
    VctHandle& operator=(const VctHandle&) = delete;
    VctHandle(VctHandle&& o) noexcept : h_(o.release()) {}
    VctHandle& operator=(VctHandle&& o) noexcept { if (this != &o) adopt(o.release()); return *this; }
    ~VctHandle() { reset(); }
    void reset() { adopt(nullptr); }
    hipError_t create(unsigned flags = 0) {      // the old one goes first; a failure leaves none
        reset();
        const hipError_t e = Create(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
    void adopt(H h) {      // one made another way (a stream with a priority or a CU mask): owned from here on
        if (h_) (void)Destroy(h_);
        h_ = h;
    }
    H release() { H h = h_; h_ = nullptr; return h; }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
};
using VctEvent = VctHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using VctStream = VctHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

// The two events around a launch that vct_set_trace_timing decides to time or not, and what the matching vct_last_*_ms
// may say about them.  begin / end go around the launch on its stream; with timing off they record nothing (an event
// costs a launch ~7 us of dispatch gaps).  Assigning a fresh VctTimer forgets the result and frees the events.
struct VctTimer {
    bool have = false;                  // a launch has run between begin and end
    bool timed = false;                 // ... the last one with timing on: the events bracket it

    hipError_t create() {               // the events now, so that no later begin allocates
        hipError_t e = ev0_ ? hipSuccess : ev0_.create();
        if (e == hipSuccess && !ev1_) e = ev1_.create();
        return e;
    }
    hipError_t begin(hipStream_t s, bool on) {
        on_ = on;
        if (!on) return hipSuccess;
        const hipError_t e = create();
        return e == hipSuccess ? hipEventRecord(ev0_.get(), s) : e;
    }
    hipError_t end(hipStream_t s) {
        const hipError_t e = on_ ? hipEventRecord(ev1_.get(), s) : hipSuccess;
        if (e == hipSuccess) { have = true; timed = on_; }
        return e;
    }
    enum Verdict { OK = 0, NEVER, UNTIMED, FAILED };      // FAILED: a HIP error, in *err
    Verdict elapsed(float* ms, hipError_t* err) const {   // waits for the second event
        if (!have) return NEVER;
        if (!timed) return UNTIMED;
        *err = hipEventSynchronize(ev1_.get());
        if (*err == hipSuccess) *err = hipEventElapsedTime(ms, ev0_.get(), ev1_.get());
        return *err == hipSuccess ? OK : FAILED;
    }
    hipEvent_t first() const { return ev0_.get(); }       // (vct_last_diffuse_rate_ms reads the marks between them)
    hipEvent_t last() const { return ev1_.get(); }

private:
    VctEvent ev0_, ev1_;
    bool on_ = false;                   // what the pending begin was given
};

// Scratch of one kind of raster pass (vct_api_raster.hip raster_args).  Between passes every visibility word is all-ones and
// the counter set of the next pass is zero: the kernels re-establish both themselves (vct_raster.hip run_visibility), so
// a pass launches no memset.  `dirty` (a launch failed, or nothing is initialised yet) makes the next pass clear
// everything once.  The shadow pass and the main draw have scratch of their own, so that the main draw's visibility
// raster can run on the second stream WHILE the shadow map is rasterised (vct_gi_pass); the shadow pass writes the
// shadow-map words and leaves `vis` unused.
struct VctRasterScratch {
    // direct form
    VctBuf<int32_t> lists;              // [2*ntri] wave list, [2*ntri] group list
    VctBuf<char> recs;                  // [2*ntri] 96-byte set-up records handed from k_raster_vis to k_raster_mid
    VctBuf<uint32_t> counts;            // two sets of [tile work items, wave list, group list, pad]
    int set = 0;                        // the counter set the next pass uses
    VctBuf<uint2> items;
    // tile-binned form (vct_raster.hip), see VctRasterArgs
    VctBuf<char> bin_recs;              // 160-byte records
    VctBuf<uint2> bin_entries;          // capacity + the spare entry k_bin_fill's idle lanes write
    VctBuf<uint32_t> bin_count;         // count + cursor, [2 * bins * VCT_BIN_CSTRIDE]
    VctBuf<uint4> bin_items;
    VctBuf<uint32_t> bin_huge;          // huge list [VCT_BIN_HUGE_CAP] + two counter sets [16] behind it
    int bin_set = 0;
    VctBuf<unsigned long long> vis;     // 64-bit visibility words of the main draw
    bool dirty = true;
    // frees the buffers sized by the mesh's triangle count (a new mesh: the next pass allocates them for it)
    void release_mesh() { lists.reset(); recs.reset(); bin_recs.reset(); bin_entries.reset(); bin_items.reset(); }
};

// What a frame slot keeps for point queries (include/vct.h "point queries", vct_api_query.hip): staging for host-located
// points and outputs, the sort's scratch, the step counters and the timing events of the march.  Everything is created
// by the first query that needs it, grows on demand and is never shrunk; a query that fails leaves what it had grown (the
// owner frees it with the slot).  Work of a query on these buffers is ordered by the slot's stream.
struct VctPointQuery {
    VctBuf<float> pts;                  // staged points of a host-located query
    VctBuf<float> out, out_cones;       // staged results [n][4], [n][6][4]
    VctBuf<uint8_t> out_steps;          // [n][6] / [n]
    VctBuf<uint32_t> keys, index;       // VCT_QUERY_SORT_CELLS: two (key, index) buffer pairs of the radix sort, [2][n] each
    VctBuf<char> sort_tmp;              // the device sort's temporary storage
    VctBuf<unsigned long long> ctr;     // [VCT_DR_COUNTERS] executed steps of the last query (zeroed by its launch)
    VctTimer timer;                     // around the march kernel (vct_last_point_query_ms)
    bool sorted = false;
    uint64_t n = 0;
    int kind = 0;
};

// What a frame slot keeps for the G-buffer import (include/vct.h "G-buffer import", vct_api_import.hip): device staging
// for a host-located import -- one buffer, every input at an offset of its own, grown on demand and never shrunk -- and
// the timing events around the import kernel.  Work on them is ordered by the slot's stream; a host-located import
// returns only when the stream has passed its kernel, so the staging is free again at every entry.
struct VctGBufferImport {
    VctBuf<char> stage;
    VctTimer timer;                     // around k_gbuffer_import (vct_last_gbuffer_import_ms)
};

// Two frames in flight (vct_set_frames_in_flight, round 6).  A whole-frame trace launch pays ~20 us of ramp and drain
// (the last generation of workgroups leaves compute units idle, tools/quant_probe.py) plus the dispatch gap to the next
// kernel of its stream: 4-5 % of a 0.61 ms frame.  A renderer that starts frame k + 1 on a second stream while frame k
// drains gets that back (tools/pipe_probe.py: trace 0.626 -> 0.598 ms per frame, Render() 0.773 -> 0.738 at
// configs[1]) -- what the reference's GL driver does with consecutive frames of its command queue.  What a frame owns
// exists once per SLOT, below; every entry point works on the selected slot (cur(c)).  The main draw's raster scratch is
// part of the slot, so frame k + 1's G-buffer pass needs nothing of frame k's and the two overlap.  Everything else
// (chain, shadow map, mesh) is shared, ordered by events: a stage that WRITES shared state (uploads, shadow map, inject,
// mips, bounce) waits for everything the other slot has in flight (pipeline_join), and the next slot switch makes the
// other stream wait for that stage.  Slot 0's stream is the context's stream.
struct VctFrameSlot {
    VctStream stream;
    VctTimer march;                     // around the march launches, a screen trace's or a bounce's (vct_last_trace_ms); `have`: one has run
    VctBuf<float> gb_tiled;             // [tiles][23][64]
    const float* gb_current = nullptr;  // tiled buffer the next resident trace reads: gb_tiled or the caller's (not owned)
    VctBuf<uint16_t> frame;             // RGBA16F [h][w][4]
    uint16_t* frame_target = nullptr;   // caller-owned output (vct_set_frame_target) or null (not owned)
    VctBuf<uint32_t> tile_steps;        // [tiles] executed steps per 8x8 tile of the screen trace
    VctBuf<uint16_t> aov;               // per-component outputs (vct_set_aov_outputs): popcount(aov_which) frames, bit order
    // pixel-emission planes (include/vct.h "emissive materials"), tiled [tiles][3][64]: present while material emission is
    // attached (the G-buffer pass writes them) or the caller set planes of its own on this slot (emis_user); a trace
    // launch with planes adds them in the composite
    VctBuf<float> emis;
    bool emis_user = false;             // vct_set_pixel_emission attached them: a detach of the material table leaves them alone
    // pixel-gloss plane (include/vct.h "per-material gloss"), tiled [tiles][64]: present while gloss classes are attached;
    // a trace launch with a plane marches each pixel's specular cone with its class's table
    VctBuf<uint8_t> gloss;
    // lit planes (include/vct.h "local lights"), tiled [tiles][3][64]: present while lights are attached; every composite
    // launch fills the rows it takes (k_light_pixels) and passes them in the place of the pixel-emission planes
    VctBuf<float> lit;
    VctTimer lit_timer;                 // around k_light_pixels (vct_last_lights_ms [1]); `have`: a launch has filled the planes
    // half-rate diffuse gather (vct_set_diffuse_rate(ctx, 2); vct_internal.h VctTraceParams::dr_*), present at rate 2 only
    VctBuf<float4> dr_ind;              // [h][w]
    VctBuf<float4> dr_coarse;           // [ch][cw]
    VctBuf<uint8_t> dr_anchor;          // [ch][cw]
    VctBuf<uint32_t> dr_list;           // [w * h]
    VctBuf<unsigned long long> dr_ctr;  // [VCT_DR_CTR_WORDS]
    VctEvent dr_ev[3];                  // between the pass's four launches (vct_last_diffuse_rate_ms)
    bool last_trace_half = false;       // the last screen trace was a half-rate pass: dr_ctr holds its marches' counts
    int last_row0 = 0, last_row1 = 0;
    int last_row_stride = 1;            // the last screen trace took every last_row_stride-th tile row of [last_row0, last_row1)
    bool last_trace_compacted = false;  // ... of trace_variant 4: counts per virtual tile, no per-row histogram
    bool last_was_screen_trace = false; // the step counters hold a screen trace (indexed by tile row), not a bounce
    bool have_gbuffer = false;          // a G-buffer is resident (uploaded by vct_trace or rendered)
    // voxel view (vct_render_voxels): the occupancy words of the level it last showed -- slot state, so that a view writes
    // nothing the other slot reads -- and what they were built from; rebuilt when either differs
    VctBuf<unsigned long long> vv_occ;
    const uint32_t* vv_texels = nullptr;
    uint64_t vv_gen = 0;
    VctTimer vv_timer;                  // around the view's walk (vct_last_voxel_view_ms)
    VctRasterScratch raster;            // the main draw's
    // the dynamic mesh's own direct-form pass of the main draw (include/vct.h "dynamic mesh", VCT_DYNAMIC_DRAW_GBUFFER):
    // its `vis` is the slot's SECOND visibility buffer, ids from 0; empty until the first pass with the flag on
    VctRasterScratch dyn_raster;
    VctPointQuery query;                // point queries issued on this slot
    VctGBufferImport gb_import;         // G-buffer imports issued on this slot

    // where a trace writes and a download reads: the caller's target or the slot's own frame
    uint16_t* frame_out() const { return frame_target ? frame_target : frame.get(); }
    // the buffers and events of the half-rate gather for a w x h frame, zeroed on the slot's stream; a failure leaves none
    hipError_t alloc_half_rate(int w, int h);      // (vct_capi.hip)
    void free_half_rate() {
        dr_ind.reset(); dr_coarse.reset(); dr_anchor.reset(); dr_list.reset(); dr_ctr.reset();
        for (VctEvent& ev : dr_ev) ev.reset();
        last_trace_half = false;
    }
};

// The mesh and its texture set (vct_upload_triangles, vct_upload_mesh_attributes / _uvs, vct_upload_textures).
struct VctMesh {
    VctBuf<float> tri_pos;
    VctBuf<int32_t> tri_mat;
    VctBuf<int32_t> tri_alpha;        // [ntri] alpha-test class per triangle (main draw), rebuilt when the mesh / textures change
    bool tri_alpha_dirty = true;
    VctBuf<float> mat_albedo;
    int32_t ntri = 0, nmat = 0;
    // raster input stages
    VctBuf<float> tri_nrm, tri_tan, tri_bit;
    VctBuf<float> mat_specular;
    VctBuf<float> mat_emission;       // [nmat][4] (rgb, 0) material emission (vct_upload_emission), or none: no emission attached
    VctBuf<uint8_t> mat_gloss;        // [nmat] gloss class per material (vct_upload_material_gloss), or none
    // material textures (vct_upload_textures) + texture coordinates (vct_upload_mesh_uvs)
    VctBuf<float> tri_uv;
    VctBuf<uint32_t> tex_texels;
    VctBuf<VctTexDesc> tex_desc;
    VctBuf<int32_t> mat_tex;
    int32_t ntex = 0;
    bool has_alpha_textures = false;
};

// Voxelization plan of the current mesh (geometry only; built by vct_upload_triangles): everything indexed by the mesh's
// triangles or brick slots -- the conservative fragments sorted by brick slot, the staging pool a pass resolves into,
// the pooled attributes, sparse-resolve state.  A new mesh starts from a fresh plan; a context whose upload failed has
// an empty one (vct_voxelize refuses).
struct VctVoxelPlan {
    VctBuf<unsigned long long> acc;    // reference mode only, allocated on first use: [nslots][512][2] ((triangle + 1) << 32 | rgb)
    VctBuf<uint32_t> attr_albedo;      // [nslots][512] resolved mean albedo (cfg.voxel_attributes)
    VctBuf<uint32_t> attr_normal;      // [nslots][512] resolved mean normal (biased)
    bool attrs_valid = false;          // attr_albedo / attr_normal hold a resolve of THIS mesh's pools (vct_bounce needs it)
    VctBuf<uint32_t> brick_slot;       // [V^3/512] brick -> slot or VCT_NO_SLOT
    uint32_t nslots = 0;
    VctBuf<uint32_t> frag_sorted;      // [n_frags] triangle << 9 | voxel inside the brick
    VctBuf<float2> frag_bary;          // [n_frags] the fragment's barycentrics (geometry only: once per mesh, k_frag_geom)
    VctBuf<float> frag_alb;            // [n_frags][3] the fragment's albedo (scenes with textures); built by the first
    bool frag_alb_dirty = true;        //   voxelize pass after the texture coordinates / textures changed
    VctBuf<uint32_t> tri_qnrm;         // [ntri][3] quantised face normals (config.voxel_attributes)
    uint32_t n_frags = 0;
    VctBuf<uint32_t> slot_first;       // [nslots + 1]
    VctBuf<uint32_t> slot_brick;       // [nslots]
    VctBuf<uint4> items;               // [n_items] work items of the voxelize pass (VctVoxParams::items)
    uint32_t n_items = 0;
    uint32_t chunk = VCT_VOX_CHUNK;
    VctBuf<unsigned long long> acc2;   // HBM accumulators of the multi-chunk slots (+ attributes): chunks add, k_vox_resolve_multi resolves and re-zeroes
    VctBuf<unsigned long long> acc2_attr;
    VctBuf<uint32_t> multi_slot;       // [n_multi] slot of every multi-chunk slot
    uint32_t n_multi = 0;
    VctBuf<uint32_t> stage;            // [nslots][512] RGBA8 of the pending north-star pass
    VctBuf<uint32_t> stage_albedo;     // [nslots][512] (cfg.voxel_attributes)
    VctBuf<uint32_t> stage_normal;
    VctBuf<int32_t> ref_big;           // reference mode: triangles left to the workgroup pass (+ counter)
    bool acc_pending = false;          // accumulators hold an unresolved voxelize pass
    // Emission pool (include/vct.h "emissive materials"): one staged RGBA8 brick per slot like `stage`, holding the
    // rounded mean of unorm8(emission[material]) over each voxel's fragments.  Light-independent: allocated by
    // vct_upload_emission, built by the first north-star pass after the mesh or the table changed (emis_dirty), added to
    // the staged texels by the resolve of every pass voxelized with it (pass_emis).
    VctBuf<uint32_t> emis_pool;        // [nslots][512]
    bool emis_dirty = true;
    bool pass_emis = false;            // the pending (or last resolved) north-star pass was voxelized with the pool built
};

// The voxel volume: the Morton mip chain the trace reads and which of its parts are current.  The flags change only in
// the functions named after what happened to the chain; entry points read them.  All of it survives a mesh change.
struct VctChain {
    int V = 0, nlev = 0;
    size_t chain_texels = 0;
    VctBuf<uint32_t> chain;           // Morton chain (bounce 0: direct light)
    VctBuf<uint32_t> chain_b;         // second chain (bounce 1), allocated by vct_bounce
    VctBuf<uint32_t> aniso;           // [6][chain_texels - V^3] directional chains (cfg.anisotropic_mips)
    bool want_cells = false;          // vct_set_footprint_records / VCT_FOOTPRINT_RECORDS=1
    VctBuf<uint4> cells;              // footprint records of the levels >= 1 of `chain` (32 B per texel of those levels)
    VctBuf<uint32_t> staging;         // linear staging for up/downloads (size of level 0)
    VctBuf<uint32_t> brick_flags;     // [V^3/512] touched in the pending pass
    VctBuf<uint32_t> brick_prev;      // [V^3/512] touched in the pass level 0 currently shows
    VctBuf<uint32_t> mip_seen;        // [V^3/512] bricks non-empty when the chain's mips were last built
    VctBuf<uint32_t> mip_seen_b;      // same for the bounce chain
    bool use_chain_b = false;         // the trace reads chain_b until the next vct_inject_light
    bool mips_valid = true;           // levels >= 1 describe level 0 (a fresh chain is all zero)
    bool cells_valid = false;         // `cells` describe the levels >= 1 of `chain`
    bool level0_dirty = false;        // level 0 was written by an upload: next resolve is dense
    uint64_t gen = 1;                 // counts the changes of anything a voxel view can show (chains, pooled attributes)
    bool chain_sparse_ready = true;   // bricks outside mip_seen have all-zero ancestors (true for a fresh, zero-filled
                                      // chain; an upload clears it until a dense mip build over a resolved level 0)

    const uint32_t* active() const { return use_chain_b ? chain_b.get() : chain.get(); }      // the chain the trace reads
    size_t nvox() const { return (size_t)V * V * V; }
    size_t nbricks() const { return nvox() / 512; }
    bool tracked() const { return brick_prev && mip_seen && !level0_dirty; }      // level 0 mirrors brick_prev: a resolve's output, not an upload's
    // the sparse mip build reduces only bricks that hold something now (brick_prev) or did at the last build (mip_seen)
    bool sparse_mips_ok() const { return tracked() && chain_sparse_ready; }
    void touched() { ++gen; }
    void level0_uploaded(bool with_levels) {      // the next resolve and mip build are dense
        touched(); use_chain_b = false; mips_valid = with_levels; cells_valid = false; level0_dirty = true; chain_sparse_ready = false;
    }
    void level0_resolved() { touched(); level0_dirty = false; use_chain_b = false; mips_valid = false; }      // vct_inject_light
    void mips_reduced(bool sparse) { if (!sparse) chain_sparse_ready = tracked(); }      // a dense build over a tracked level 0 makes the sparse form valid again
    void mips_built() { touched(); mips_valid = true; use_chain_b = false; }      // ... and the directional chains followed
    void bounce_done() { touched(); use_chain_b = true; }
    void records_valid(bool v) { cells_valid = v; }      // built; or freed / about to be rebuilt
};

// The shadow map: its words ARE the shadow pass's atomicMin words (vct_internal.h "shadow map words"), written under epoch
// 3, 2, 1, 0, then one memset and 3 again -- a new pass overwrites older epochs by itself, readers see them as depth 1.0.
struct VctShadowMap {
    VctBuf<uint32_t> words;           // size^2 (vct_internal.h vct_shadow_depth)
    int32_t size = 0;
    uint32_t ebase = 0;               // epoch base of the words the map currently shows
    VctBuf<uint2> tiles;              // decoded (min, max) per dilated 8 x 8 tile of the current map (vct_launch_shadow_minmax)
    uint32_t passes = 0;              // shadow passes rasterised into `words` since their last memset
    VctRasterScratch raster;          // scratch of the shadow pass (the main draw's is per frame slot)
    VctRasterScratch dyn_raster;      // ... and of the dynamic mesh's direct-form pass behind it (VCT_DYNAMIC_DRAW_SHADOW)
    float light_vp[16] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};

    void drop() { words.reset(); tiles.reset(); size = 0; }
    void restart_epochs() { passes = 0u; }      // fresh or cleared words: the next pass starts with the memset
    uint32_t next_epoch(bool* memset_due) const { *memset_due = (passes & 3u) == 0u; return 3u - (passes & 3u); }
    void pass_done(uint32_t epoch) { ebase = VCT_SHADOW_EPOCH(epoch); ++passes; }
    // a pass that fails leaves a map but NO tile bounds: a stale table would decide PCF windows wrongly, without one every window is fetched
    int pass_result(int rc) { if (rc) tiles.reset(); return rc; }
};

// Which form the MAIN draw's visibility takes (the shadow pass is opaque and sparse: the direct form won every measurement).
// mode 0 = auto: scenes without alpha-tested textures keep the direct form; otherwise six passes over the same tile rows are
// sampled (vct_api_raster.hip kAutoSeq) and the faster form is kept until the mesh or the textures change.  1 / 2 = VCT_RASTER_PATH=direct / binned.
struct VctRasterForm {
    int mode = 0;
    int state = 0;                    // position in the sampling sequence; 6: all sampled
    int choice = -1;                  // -1 undecided, 0 direct, 1 binned
    int rows[2] = {0, 0};             // tile rows of the sampled passes
    bool in_sequence = false;         // the pass pick() was last asked about is the sequence's next
    VctEvent ev[8];                   // begin / end of the four timed samples
    int last_form = 0;                // form of the last main-draw visibility pass: 1 direct, 2 tile-binned (vct_get_stage_counts [6])
    uint32_t bin_test_caps[2] = {0u, 0u};   // VCT_BIN_TEST_CAPS="records,entries": capacities REPORTED to the binned kernels (tests of the overflow paths)

    void restart() { state = 0; choice = -1; }      // a new mesh or texture set: measured again
    // the form of a pass over tile rows [row0, row1) (*binned), and the timed sample it is (0 .. 3) or -1
    int pick(int row0, int row1, bool has_alpha_textures, bool* binned);      // (vct_api_raster.hip)
    void launched() { if (in_sequence) ++state; }      // after the pass's visibility launch (and its end event) succeeded
};

// vct_gi_pass runs the G-buffer raster on a second stream beside the voxel stages: created on first use.
struct VctForkJoin {
    VctStream aux;
    VctEvent ev_fork, ev_shadow, ev_join;
};

// Ordering between the two frame slots' streams.  The other slot's stream receives work only while its slot is selected,
// so ONE join (drain) per selection orders (waits for) everything it holds: later producers of the same selection skip theirs.
// vct_gi_pass -- five producers in a row -- paid five cross-queue waits per pass for nothing (0.860 ms against 0.817 on one slot).
struct VctSlotOrder {
    VctEvent ev;                      // scratch event of the cross-slot waits
    bool streams_overlap = false;     // the second slot's stream was SEEN to run beside the first (vct_capi.hip streams_overlap)
    bool produced = false;            // a stage that writes shared state ran on the selected slot's stream since the last switch
    bool joined = false, drained = false;      // ... and the other slot's stream was joined / drained since then
    void note_producer() { produced = true; }      // the next slot switch makes the other stream wait for this stream
    void reset() { produced = joined = drained = false; }
};

// Gloss classes (include/vct.h "per-material gloss", vct_api_gloss.hip): the attached table, the march steps of each
// class's step table, and the device copy of both with the tables (vct_internal.h VctGlossTable).  n == 0: none attached.
// vct_refresh_steps rebuilds the device copy with the diffuse and the specular table, under the same division verdict.
struct VctGloss {
    int n = 0;
    vct_gloss_class cls[VCT_GLOSS_CLASSES_MAX] = {};
    int nsteps[VCT_GLOSS_CLASSES_MAX] = {};
    VctBuf<VctGlossTable> table;      // one element
};

// Sky light (include/vct.h "sky light", vct_api_sky.hip): the attached coefficients as given, their folded polynomial
// form (vct_sky_check.h vct_sky_fold), and the device copy of the latter that the SKY kernels read.  Context state: every
// frame slot and every point query sees the same sky.
#define VCT_SKY_DEV_FLOATS 32           // 27 coefficients, padded to whole 32-byte scalar loads
struct VctSky {
    bool attached = false;
    float sh[27] = {};
    float poly[27] = {};
    VctBuf<float> poly_dev;           // [VCT_SKY_DEV_FLOATS]
    const float* dev() const { return attached ? poly_dev.get() : nullptr; }
};

// Local lights (include/vct.h "local lights", vct_api_lights.hip): the attached lights as given and the device copy of
// their folded form (vct_lights_check.h VctLightDev) that both kernels read.  n == 0: none attached.  Context state:
// every frame slot and the voxel chain see the same lights.
struct VctLights {
    int n = 0;
    vct_light given[VCT_LIGHTS_MAX] = {};
    VctBuf<VctLightDev> table;        // [VCT_LIGHTS_MAX]
    VctTimer vox_timer;               // around k_light_voxels (vct_last_lights_ms [0])
};

// What outlives the dynamic mesh (vct_set_dynamic_draw, vct_set_dynamic_bounce): context state BESIDE the layer, so that
// attaching, replacing or detaching a mesh carries nothing over by hand.
struct VctDynamicSettings {
    int32_t draw_flags = 0;             // VCT_DYNAMIC_DRAW_*
    float draw_specular[3] = {0.0f, 0.0f, 0.0f};
    int32_t bounce_on = 0;              // the second bounce over the layer; read by the next vct_bounce
};

// The dynamic mesh (include/vct.h "dynamic mesh", vct_api_dynamic.hip): the context's own copy of its triangles and
// everything the per-pass path needs, allocated by vct_set_dynamic_mesh so that no pass allocates.  ntri == 0: none
// attached.  Nothing here is indexed by the static mesh's slots: it survives vct_upload_triangles.  What lives and dies
// together is one member, and a fresh layer (attach, replace, detach) has a fresh one of each.  Only vct_api_dynamic.hip
// and the inline helpers of this file name a member; every other file calls what is declared under its name below.
struct VctDynamic {
    int32_t ntri = 0, nmat = 0;
    uint32_t max_bricks = 0;            // brick slots of the layer (vct_dynamic_check.h vct_dynamic_capacity)
    VctBuf<float> pos;                  // [ntri][9] positions of the last update
    VctBuf<int32_t> mat;                // [ntri]
    VctBuf<float> albedo;               // [nmat][4]
    VctBuf<int32_t> big_list;           // [ntri]
    VctBuf<uint32_t> words;             // [VCT_DYN_WORDS] counters and the two statistics sets (vct_internal.h)
    VctBuf<uint32_t> brick_slot;        // [V^3 / 512]
    VctBuf<uint32_t> slot_brick;        // [max_bricks] of the pending pass
    VctBuf<uint32_t> res_brick;         // [max_bricks] of the last resolved pass
    VctBuf<unsigned long long> acc;     // [max_bricks][512][2]
    VctBuf<unsigned long long> acc_attr;   // [max_bricks][512][3] (cfg.voxel_attributes)
    VctBuf<uint32_t> pool_rad, pool_alb, pool_nrm;      // [max_bricks][512] of the last resolved pass
    VctTimer vox_timer, merge_timer;    // vct_last_dynamic_ms
    // The pass in flight.  in_chain: the last vct_inject_light merged THIS layer into level 0 -- false for a fresh layer
    // (attached or replaced since) and after an inject that had no pass of the layer to merge; a pass the layer was left
    // out of for capacity keeps it true and shows zero used slots on the device.  emis: the pending pass was voxelized
    // with the emission table, so its merge -- or its discard -- takes the EMIS form and leaves the sums zero.
    struct Pass {
        bool pending = false;           // the accumulators hold a pass no merge has resolved
        int set = 0;                    // the statistics set of the last resolved pass
        bool in_chain = false;
        bool emis = false;
    } pass;
    // Drawing the mesh in the raster stages (vct_set_dynamic_draw): the draw copy and the frames, all four or none, exist
    // while a flag is on and a mesh is attached; k_dyn_draw_prepare rebuilds them behind every copy into `pos`.
    struct DrawCopy {
        VctBuf<float> pos;              // [ntri][9] `pos`, a triangle outside the vertex contract as nine zeros
        VctBuf<float> nrm, tan, bit;    // [ntri][9] the face frame at all three vertices, or the corner frames of `corner_nrm`
    } draw;
    // Corner normals (vct_set_dynamic_normals), empty: none -- the frames are the faces'.  They belong to the mesh like the
    // emission table, are in the space of the mover's rest positions, and outlive a mover attached, replaced or detached.
    VctBuf<float> corner_nrm;           // [ntri][3][3] as given
    // Emission of the mesh's materials (vct_set_dynamic_emission): the table and the sums beside `acc`, both or neither.
    struct Emission {
        VctBuf<float> table;            // [nmat][4] (rgb, 0)
        VctBuf<unsigned long long> acc; // [max_bricks][512][2]
    } emis;
    // The mover (vct_feature_rules.h): rigid parts (vct_set_dynamic_parts) or a skin (vct_set_dynamic_skin), one at a time.
    // All of it or none (VCT_MOVER_NONE, n == 0): it belongs to the mesh like the emission table and is dropped on attach,
    // replace and detach of the mesh.  While attached, `pos` is `rest` moved by the matrices of the last
    // vct_update_dynamic_transforms (or the rest itself behind a vct_update_dynamic_positions).
    struct Mover {
        VctMover kind = VCT_MOVER_NONE;
        int32_t n = 0;                  // parts or bones: the matrices vct_update_dynamic_transforms takes
        VctBuf<float> rest;             // [ntri][9] the positions at the attach or of the last vct_update_dynamic_positions
        VctBuf<float4> m;               // [n][3] rows of the matrices, the context's own copy: 16-byte aligned, as the kernels load them
        VctTimer timer;                 // vct_last_dynamic_transform_ms
        bool moved = false;             // `pos` is `rest` moved by `m` (a vct_update_dynamic_transforms since the rest was set), not `rest` itself
        // the kind's own arrays, checked on the host; those of the other kind stay empty
        VctBuf<int32_t> part;           // parts: [ntri] in 0 .. n-1
        VctBuf<uint16_t> bone;          // skin: [ntri][3][4] in 0 .. n-1, packed: 24 bytes per triangle
        VctBuf<float> weight;           // skin: [ntri][3][4] finite
    } mover;

    bool attached() const { return ntri > 0; }
    int32_t matrices() const { return mover.n; }      // what vct_update_dynamic_transforms takes; 0: no mover
};

struct vct_ctx {
    vct_config cfg;
    int device = 0;
    int reserved_cus = 0;             // VCT_COMM_RESERVED_CUS at vct_create: CUs kept for the communication stream
    std::string err;

    VctChain vol;
    VctBuf<float> gb_linear;          // [23][w*h] staging
    // lighting components (vct_set_lighting_components): VCT_SHOW_* mask of the composite; per-component outputs
    // (vct_set_aov_outputs): VCT_AOV_* bits, one buffer per frame slot (VctFrameSlot::aov)
    uint32_t show_mask = VCT_SHOW_ALL;
    uint32_t aov_which = 0;
    int diffuse_rate = 1;             // vct_set_diffuse_rate: 1, or 2 = the half-rate diffuse gather
    int diffuse_rate_waves = 1;       // waves per 64 marched points of its marches (VCT_DIFFUSE_RATE_WAVES=2: A/B)
    VctBuf<uint8_t> dbg_steps;
    VctBuf<float> dbg_cones;
    VctBuf<unsigned long long> step_counter;   // [VCT_STEP_COUNTERS] atomic bank of the bounce kernels (memset before each bounce)
    VctBuf<unsigned long long> stats;  // [32] march statistics of instrumented builds (VCT_STATS); scratch of the self-tests
    VctBuf<uint32_t> vt_pix;          // trace_variant 4: compaction list [tiles][64] + the virtual-tile counter behind it
    VctBuf<VctStep> steps_dev;        // [2][VCT_MAX_STEPS]
    VctBuf<uint32_t> spread_lut;      // [1024] spread3(i) << 2 (vct_trace.hip: dilated anchor coordinates by scalar load)
    int n_diffuse = 0, n_specular = 0;
    VctGloss gloss;
    VctSky sky;
    VctLights lights;
    VctDynamic dyn;
    VctDynamicSettings dyn_settings;
    bool steps_dirty = true;
    bool fast_div = false;            // set by vct_refresh_steps: constant divisors admit the FMA division
    // set by vct_create: the default trace kernel runs in its CHAIN form, one texel buffer per wave and the level's byte
    // offset in the loads' scalar operand (vct_trace.hip ChainRef) -- every level starts below 4 GiB, the device passed the
    // offset read of the texel self-test, and VCT_LEVEL_DESCRIPTORS=1 does not ask for a resource per level and fetch
    bool chain_form = false;
    // division of the last march launch: 1 IEEE, 2 verified product, 3 x * r; a screen trace adds its texel-resource form
    // in bits 8-9 (vct_trace.hip vct_launch_trace).  vct_get_stage_counts [2].
    int last_march_form = 0;
    // vct_set_trace_timing: bracket every march launch with the two timing events vct_last_trace_ms reads.  On by default
    // (every entry point keeps working); a frame loop switches it off -- the two events cost a launch ~7 us of dispatch
    // gaps on this GPU (one-stream step 0.549 -> 0.542 ms, a 1/8 slab's 0.12 ms step the same 7 us).
    bool time_traces = true;

    float cam[3] = {0.0f, 4.0f, 0.0f};        // VCT.h:8
    float light[3] = {0.0f, 1.0f, 0.25f};     // VCT.h:14

    VctMesh mesh;
    VctShadowMap shadow;
    VctRasterForm raster_form;
    VctForkJoin fork;
    VctVoxelPlan vox;
    VctBuf<uint32_t> plan;             // [4] device counters used while planning
    VctBuf<uint32_t> bounce_list;      // counter word + occupied-voxel list of the bounce
    VctBuf<uint32_t> brick_over;
    VctBuf<uint32_t> bounce_dyn_map;   // [nbricks] brick -> resolved slot of the dynamic layer, of one bounce (vct_set_dynamic_bounce)
    int acc_mode = 0;                  // vct_voxelize_mode of the pending (or last resolved) pass
    vct_comm* comm = nullptr;          // multi-GPU slabs + gather (vct_comm_init)
    // frame slots (see VctFrameSlot): slots [0, frames_in_flight) are live, slots[cur_slot] is selected
    int frames_in_flight = 1;          // 1 or 2
    int cur_slot = 0;
    VctFrameSlot slots[2];
    VctSlotOrder xslot;
};

// the selected frame slot, and the other one (meaningful with two frames in flight)
inline VctFrameSlot& cur(vct_ctx* c) { return c->slots[c->cur_slot]; }
inline const VctFrameSlot& cur(const vct_ctx* c) { return c->slots[c->cur_slot]; }
inline VctFrameSlot& other(vct_ctx* c) { return c->slots[1 - c->cur_slot]; }

inline int vct_tiles_x(const vct_ctx* c) { return (c->cfg.width + VCT_TILE - 1) / VCT_TILE; }
inline int vct_tiles_y(const vct_ctx* c) { return (c->cfg.height + VCT_TILE - 1) / VCT_TILE; }
inline bool vct_rows_in_frame(const vct_ctx* c, int row0, int row1) { return row0 >= 0 && row1 <= vct_tiles_y(c) && row0 <= row1; }
inline size_t vct_gb_tiled_floats(const vct_ctx* c) { return (size_t)vct_tiles_x(c) * vct_tiles_y(c) * VCT_GB_NPLANES * VCT_TILE_PIX; }
inline size_t vct_emis_tiled_floats(const vct_ctx* c) { return (size_t)vct_tiles_x(c) * vct_tiles_y(c) * VCT_EMIS_NPLANES * VCT_TILE_PIX; }
inline size_t vct_gloss_tiled_bytes(const vct_ctx* c) { return (size_t)vct_tiles_x(c) * vct_tiles_y(c) * VCT_TILE_PIX; }
inline float vct_vertex_limit(const vct_ctx* c) { return VCT_VERTEX_LIMIT_GRIDS * c->cfg.grid_world_size; }      // the vertex contract's bound (include/vct.h), in fp32 as every kernel compares it
inline size_t vct_aov_frames(uint32_t which) { return (size_t)__builtin_popcount(which); }      // one frame per VCT_AOV_* bit that is on

// ---- what more than one translation unit needs, by the file that defines it: vct_capi.hip ----
int vct_fail(vct_ctx* c, int code, const std::string& msg);
int vct_create_overlapping_stream(vct_ctx* c, hipStream_t base, hipStream_t* out, bool* overlaps);
// a stage that WRITES state both slots read waits on the GPU for all the other slot has in flight; the next slot switch makes the other stream wait for it
int vct_pipeline_join(vct_ctx* c);
// Uploads free and reallocate buffers the other slot's kernels may still read: the host waits for that slot.
int vct_pipeline_drain(vct_ctx* c);
// c->gb_linear and c->vol.staging are ONE staging buffer each for both frame slots, used on the selected slot's stream: before
// this slot's work overwrites one the host waits for whatever the other slot's stream still has in flight -- that may be a
// tile kernel reading it.  Only a host-located linear hand-over or a download pays this (a volume upload drains the pipeline
// anyway); with one slot it does nothing.
int vct_staging_free(vct_ctx* c);
// *ms of a timer for a vct_last_*_ms getter, or the getter's refusal: `never` / `untimed` are its words for a timer that
// never ran / whose last launch was issued with timing off
int vct_timer_ms(vct_ctx* c, const VctTimer& t, float* ms, const char* never, const char* untimed);
// vct_feature_rules.h on a context: the features and modes in force, gathered in this one place; and the refusal of the
// first pair of the matrix among `features` x `modes` (VCT_OK: none), in the name of the entry point `who`.  A feature's
// setter asks with its feature against the modes in force, a mode's setter with the features in force against its mode,
// a launch with both as they are.
struct VctRulesInForce { unsigned features, modes; };
VctRulesInForce vct_rules_in_force(const vct_ctx* c);
int vct_refuse_conflict(vct_ctx* c, const char* who, unsigned features, unsigned modes);
// vct_planes.hip -- what the per-pixel side planes of a frame slot (VctFrameSlot::emis, gloss, lit) do the same way.
// Each kind has a function that gives a slot zeroed planes on its stream if it has none (*fresh, if given, is set when it
// had none: vct_emission_planes, vct_gloss_plane, vct_lights_planes below) and one that takes them away again.
typedef hipError_t VctPlanesEnsure(const vct_ctx* c, VctFrameSlot& s, bool* fresh);
typedef void VctPlanesDrop(VctFrameSlot& s);
// a zeroed tiled buffer of n elements on stream s for a `b` that is empty; a failure leaves it empty
template <class T>
hipError_t vct_planes_ensure(VctBuf<T>& b, size_t n, hipStream_t s, bool* fresh = nullptr);
// Planes for every live slot, all or nothing, after the caller's own allocations gave `e`: each slot's stream is waited
// for; a failure drops the planes this call created, sets the error in the name of `who` and returns its code.
int vct_planes_attach(vct_ctx* c, const char* who, VctPlanesEnsure* ensure, VctPlanesDrop* drop, hipError_t e = hipSuccess);
// The caller's planes `src` (nplanes of elem-byte elements; layout VCT_GB_LINEAR / _TILED, location VCT_MEM_HOST /
// _DEVICE, both checked by the caller) into the tiled buffer `tiled` of the selected slot, on its stream; host memory is
// free again on return.  A linear host array passes through c->gb_linear.
int vct_planes_set(vct_ctx* c, void* tiled, const void* src, int32_t layout, int32_t location, int nplanes, size_t elem);
// a tiled buffer of the selected slot as linear planes into host memory, through c->gb_linear; synchronous
int vct_planes_download(vct_ctx* c, const void* tiled, void* out, int nplanes, size_t elem);
// vct_api_scene.hip: textures are used once both the maps and the texture coordinates are there
VctTextures vct_textures_of(const vct_ctx* c);
// vct_api_raster.hip: `shadow_ready` not null: the visibility raster is issued at once, only the shading kernel (it reads the shadow map) waits for it
int vct_render_gbuffer_rows_on(vct_ctx* c, const float view_proj[16], int32_t row0, int32_t row1, hipStream_t s, hipEvent_t shadow_ready = nullptr);
// vct_api_voxel.hip: parameters of the voxelizer kernels (the context's mesh and shadow map, the buffers of plan `v`); the reference's ProjX/Y/Z
VctVoxParams vct_vox_params(const vct_ctx* c, const VctVoxelPlan& v);
void vct_glm_voxel_projections(const vct_ctx* c, float proj[48]);
// ... their half that any mesh shares, everything else zero: the grid, the model scale and the shadow map
VctVoxParams vct_vox_params_scene(const vct_ctx* c);
// k_light_voxels on the selected slot's stream: the attached lights' direct term into the bricks of `slot_brick` that the
// last resolve wrote, from the two attribute pools of those slots (vct_inject_light; the dynamic layer's merge)
int vct_light_voxels(vct_ctx* c, const uint32_t* attr_albedo, const uint32_t* attr_normal, const uint32_t* slot_brick, uint32_t nslots);
// one Morton level of N^3 texels -> linear staging -> host, synchronised (the next level reuses the staging buffer)
int vct_download_level(vct_ctx* c, const uint32_t* morton, int N, uint8_t* dst);
// vct_api_trace.hip: the step tables on the device follow the config; everything the march needs (screen trace and bounce)
int vct_refresh_steps(vct_ctx* c);
// the step sequence of one aperture (trace.fs:90-104); -1: more than VCT_MAX_STEPS steps, or a march that would not end
int vct_build_steps(const vct_config& cfg, float tan_half, std::vector<VctStep>& out);
// both verdicts of the texel self-test apart (vct_api_trace.hip): vct_create fails on the first and falls back on the second
int vct_texel_buffer_selftest(vct_ctx* c, uint64_t* bad_decode, uint64_t* bad_offset);
void vct_fill_march_params(const vct_ctx* c, VctTraceParams& p, const uint32_t* chain);
// asynchronous, on the slot's stream.  row_stride > 1: only every row_stride-th tile row from row0 on; pack_rows: those rows back to back in out_base (interleaved slabs)
int vct_launch_trace_rows(vct_ctx* c, int row0, int row1, uint16_t* out_base = nullptr, int row_stride = 1, bool pack_rows = false);
// vct_api_emission.hip: drops the material emission table, its pool and the planes it attached (a new mesh, a NULL or all-zero
// table); zeroed pixel-emission planes for a slot that has none (vct_planes_ensure).  The planes live while EITHER table
// is attached -- the static mesh's or the dynamic mesh's: vct_emission_table_attached; vct_emission_planes_release drops
// them once neither is (the caller's own planes stay), called by whoever has just dropped a table.
void vct_emission_detach(vct_ctx* c);
inline bool vct_dynamic_emission_attached(const vct_ctx* c) { return (bool)c->dyn.emis.table; }
inline bool vct_emission_table_attached(const vct_ctx* c) { return c->mesh.mat_emission || vct_dynamic_emission_attached(c); }
void vct_emission_planes_release(vct_ctx* c);
hipError_t vct_emission_planes(const vct_ctx* c, VctFrameSlot& s, bool* fresh = nullptr);
void vct_emission_planes_drop(VctFrameSlot& s);      // ... and takes them away again (the VctPlanesDrop of vct_planes_attach)
// vct_api_gloss.hip: a zeroed pixel-gloss plane for a slot that has none; drops the material map (a new mesh)
hipError_t vct_gloss_plane(const vct_ctx* c, VctFrameSlot& s, bool* fresh = nullptr);
void vct_material_gloss_detach(vct_ctx* c);
// vct_api_lights.hip: zeroed lit planes for a slot that has none, the timer around their kernel started over
hipError_t vct_lights_planes(const vct_ctx* c, VctFrameSlot& s, bool* fresh = nullptr);
// vct_api_dynamic.hip: the dynamic mesh's part of vct_voxelize (discard of an unresolved pass, slots, fragments) and of
// vct_inject_light (merge into level 0, its local lights), on the selected slot's stream; nothing attached: nothing issued.
// The merge decides by itself whether there is a pass of the layer to merge and records it for vct_bounce.
int vct_dynamic_voxelize(vct_ctx* c);
int vct_dynamic_merge(vct_ctx* c);
// k_dyn_draw_prepare over the attached mesh's positions on the selected slot's stream (nothing drawn: nothing issued)
int vct_dynamic_draw_prepare(vct_ctx* c);
// a raster stage draws the mesh: attached, `flag` (VCT_DYNAMIC_DRAW_*) on in the settings and the layer's draw copy there
inline bool vct_dynamic_drawn(const vct_ctx* c, int32_t flag) { return c->dyn.attached() && (c->dyn_settings.draw_flags & flag) && c->dyn.draw.pos; }
// the mesh half (and ntri) of the dynamic mesh's own raster pass, from the draw copy: no specular table (a constant), no
// emission, no gloss classes, no textures, no alpha test; and the shade kernel's view of that pass `da`
void vct_dynamic_raster_mesh(const vct_ctx* c, VctRasterArgs& a);
void vct_dynamic_shade_args(const vct_ctx* c, const VctRasterArgs& da, VctDynShadeArgs& ds);
// vct_bounce refuses: a mesh is attached and vct_set_dynamic_bounce is off
inline bool vct_dynamic_blocks_bounce(const vct_ctx* c) { return c->dyn.attached() && !c->dyn_settings.bounce_on; }
// The layer's part of a bounce, called in front of the launch: *dyn says whether it takes the DYN form (attached, switched
// on, the layer in the chain, attribute pools); then `da` is filled and c->bounce_dyn_map, allocated on first use, is
// cleared on the selected slot's stream -- before every bounce that uses it, so the last one's bricks need no undoing.
int vct_dynamic_bounce_args(vct_ctx* c, VctBounceDynArgs& da, bool* dyn);
// vct_multi.hip: slab of the attached communicator (false: none attached); its release
bool vct_comm_rows(const vct_ctx* c, int* row0, int* row1);
void vct_comm_release(vct_ctx* c);

#define HIP_TRY(c, expr)                                                                     \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return vct_fail((c), e_ == hipErrorOutOfMemory ? VCT_ERR_NOMEM : VCT_ERR_DEVICE, \
                            std::string(#expr) + ": " + hipGetErrorString(e_));              \
    } while (0)
#define PIPE_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

#endif
