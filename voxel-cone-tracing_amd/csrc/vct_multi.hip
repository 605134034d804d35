// vct_multi.hip -- one frame across the GPUs of a node: screen-tile slabs + ONE RCCL gather per frame
// (BASELINE.json config 4).
//
// The reference is single-GPU (R/main.cpp:77-94 is one GL context), so nothing here has a counterpart in
// it.  Pixels are independent given the read-only chain (S/VoxelConeTracing.fs:165-228 reads only its own
// varyings and the shared textures), so the frame's 8-pixel tile rows are cut into `world` equal
// contiguous slabs; every rank holds its own replica of scene + chain, rasterises and traces only its
// slab, and the root receives the other ranks' slabs with a single ncclGather of padded equal slabs
// (/opt/rocm/include/rccl/rccl.h: ncclGather, in place on the root) -- root fan-in over its direct xGMI
// links, one hop per link, no ring.  No collective touches the data path of the trace itself.
//
// One process per GPU.  Per frame the host issues, natively: wait(buffer k free) -> trace kernel writes
// the slab straight into gather buffer k (vct_set_frame_target-style full-frame addressing, no copy) ->
// event -> ncclGather on a communication stream -> event.  Two buffers, so that frame k+1 may be traced while frame
// k is still being gathered -- on one GPU that overlap was measured NOT to happen (0 of 103 gather copies ran beside a
// trace, profiles/experiments/r04_gather_timeline.txt: the gather's kernels wait for the wave slots the trace holds); a
// frame costs slab trace + dependent dispatch (~23 us) + wire time.  vct_comm_last_gather_ms reports the gather alone.
//
// RCCL is loaded lazily (dlopen) so single-GPU users of libvct_amd.so never pay for it and the library
// carries no link-time dependency on a particular librccl build (a Python process that already loaded
// torch's bundled RCCL reuses that one).
//
// Everything a communicator holds has an owner (vct_comm; RcclComm and DirectRendezvous for what vct_ctx.h has none for),
// and vct_frame_step is ONE skeleton for the RCCL path, the direct-mode root and the direct-mode peer: they differ in
// where the slab goes and in the exchange_* functions.
#include <dlfcn.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "vct_ctx.h"

namespace {

// the RCCL entry points used, with the types of rccl.h restated (opaque comm, 128-byte id)
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef int ncclResult_t;
enum { ncclSuccess = 0, ncclInProgress = 7, ncclFloat16 = 6 };
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t*) = nullptr;
    ncclResult_t (*Gather)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*CommCount)(ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommCuDevice)(ncclComm_t, int*) = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};

Rccl* rccl() {
    static Rccl r;
    if (r.lib || !r.err.empty()) return &r;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char* n : names) {
        r.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (r.lib) break;
    }
    if (!r.lib) { r.err = std::string("cannot load RCCL: ") + dlerror(); return &r; }
    auto sym = [&](const char* n) { void* p = dlsym(r.lib, n); if (!p) r.err = std::string("RCCL lacks ") + n; return p; };
    r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.CommAbort = (decltype(r.CommAbort))sym("ncclCommAbort");
    r.CommGetAsyncError = (decltype(r.CommGetAsyncError))sym("ncclCommGetAsyncError");
    r.Gather = (decltype(r.Gather))sym("ncclGather");
    r.Send = (decltype(r.Send))sym("ncclSend");
    r.Recv = (decltype(r.Recv))sym("ncclRecv");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    // optional (diagnostics only: vct_comm_info)
    r.CommCount = (decltype(r.CommCount))dlsym(r.lib, "ncclCommCount");
    r.CommUserRank = (decltype(r.CommUserRank))dlsym(r.lib, "ncclCommUserRank");
    r.CommCuDevice = (decltype(r.CommCuDevice))dlsym(r.lib, "ncclCommCuDevice");
    r.GetVersion = (decltype(r.GetVersion))dlsym(r.lib, "ncclGetVersion");
    return &r;
}

// gathered[rank][local row j][8 pixel rows][w] -> frame row (j * world + rank) * 8 + ...; one 8-byte pixel per thread step
__global__ void __launch_bounds__(256)
k_deinterleave(const uint2* __restrict__ gathered, uint2* __restrict__ frame, int w, int h, int world, size_t slab_pixels) {
    const size_t n = (size_t)w * h;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / (size_t)w), x = (int)(i - (size_t)y * w);
        const int tr = y >> 3, r = tr % world, j = tr / world;
        frame[i] = gathered[(size_t)r * slab_pixels + (size_t)(j * 8 + (y & 7)) * w + x];
    }
}

// ---- direct slabs (VCT_COMM_MODE=direct; experimental, default off) ------------------------------------------------
// Every rank's trace kernel stores its slab straight into the ROOT's frame buffers (mapped through hipIpc handles: 8 B
// per pixel over xGMI), and the frame's exchange step is two flags instead of a collective: no RCCL at all.
//   rendezvous   a POSIX shared-memory block named after the communicator id: the root publishes the IPC handles of
//                its two frame buffers there, the ranks open them; the same block -- page-locked and mapped into every
//                rank's GPU (coherent host memory) -- carries the flags
//   step f, buffer k = f & 1, generation g = f / 2 + 1
//     rank r > 0:  wait release[k] >= g - 1 (the root is past frame f - 2)  ->  trace into the mapped frame  ->  done[k][r] = g
//     root:        release[k] = g - 1 (ordered behind everything it issued on its stream: the consumer of frame f - 2)
//                  ->  trace its own slab  ->  wait done[k][r] >= g for every r  ->  (de-interleave)  ->  frame f is there
//   Every wait is one lane spinning on a system-scope load with a deadline (the communicator's timeout): a dead peer
//   costs a wrong frame and an error from vct_comm_sync, never a hang.
// NOT validated across GPUs (one GPU per box here): what is tested is two processes on ONE GPU (IPC mapping, flags,
// ordering, the failure path).  Whether peer stores are visible to the root's next kernel without more than the
// end-of-kernel release is what the first run on a multi-GPU node has to show; hence off by default.
#define VCT_DIRECT_MAX_RANKS 64
struct DirectShm {
    uint32_t magic, world;
    volatile uint32_t handles_ready;                    // root: the two handles below are valid
    volatile uint32_t attached[VCT_DIRECT_MAX_RANKS];   // rank r: opened them
    hipIpcMemHandle_t frame[2];
    // flags (GPU-written, GPU-read; host memory mapped into every rank's device)
    uint32_t done[2][VCT_DIRECT_MAX_RANKS];
    uint32_t release[2];
    uint32_t timed_out;                                 // a wait gave up
};

// lanes 0 .. n-1 each wait for flags[lane * stride] >= want; deadline in wall-clock ticks (the device's
// hipDeviceAttributeWallClockRate, vct_comm::wall_khz).  `abort_word` is this process' own page-locked word: its host sets
// it before tearing the communicator down, so a wait still queued behind long compute gives up at once instead of
// polling memory that is about to be unmapped (advisor, round 5).
__global__ void k_flag_wait(const uint32_t* flags, int n, int stride, uint32_t want, uint32_t* timed_out, long long ticks,
                            const uint32_t* abort_word) {
    const int i = threadIdx.x;
    if (i >= n) return;
    const long long t0 = (long long)wall_clock64();
    while (__hip_atomic_load(flags + (size_t)i * stride, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < want) {
        if (__hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;   // local teardown: not a peer's fault
        if ((long long)wall_clock64() - t0 > ticks) {
            __hip_atomic_store(timed_out, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        __builtin_amdgcn_s_sleep(32);
    }
}
__global__ void k_flag_set(uint32_t* flag, uint32_t v) {
    __threadfence_system();
    __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// True once pred() holds, false when timeout_ms since t0 passed first (pred is asked before the clock).  spin_first: 2000
// yields, then 200 us sleeps -- what is usually over within microseconds; otherwise 1 ms sleeps -- processes still starting.
template <class Pred>
bool wait_until(Pred pred, long long timeout_ms, bool spin_first, std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now()) {
    for (int spins = 0; !pred();) {
        if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_ms) return false;
        if (spin_first && ++spins < 2000) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(spin_first ? 200 : 1000));
    }
    return true;
}

// VCT_COMM_MODE=direct: direct slabs, no RCCL (see DirectShm)
bool direct_mode() { const char* mode = getenv("VCT_COMM_MODE"); return mode && mode[0] == 'd'; }

// The RCCL communicator with an owner: destroyed with it, unless it was aborted first -- one that may be half way through
// a collective the peers will never finish (ncclCommAbort frees its resources without waiting for them).  (`h` is set by
// ncclCommInitRank alone, so the loader found every entry point used here.)
struct RcclComm {
    ncclComm_t h = nullptr;
    RcclComm() = default;
    RcclComm(const RcclComm&) = delete;
    RcclComm& operator=(const RcclComm&) = delete;
    ~RcclComm() { if (h) (void)rccl()->CommDestroy(h); }
    bool abort() { const bool had = h != nullptr; if (had) (void)rccl()->CommAbort(h); h = nullptr; return had; }
};

// What one process holds of the direct mode's rendezvous (see DirectShm): the shared block -- mapped, page-locked and
// visible to this rank's GPU --, a rank's mappings of the root's two frame buffers, the block's name (the root unlinks
// it) and this process' abort word.  Kernels use all of it: whoever drops it has drained their streams (~vct_comm).
struct DirectRendezvous {
    char name[48] = {0};
    bool root = false;
    DirectShm* shm = nullptr;          // host mapping of the rendezvous block
    bool registered = false;           // ... page-locked (hipHostRegister)
    DirectShm* shm_dev = nullptr;      // the same block as this rank's GPU sees it
    uint16_t* peer_frame[2] = {nullptr, nullptr};      // ranks > 0: the root's frame buffers, mapped
    uint32_t* abort_host = nullptr;    // this process' abort word (page-locked, mapped): k_flag_wait gives up when it is set
    uint32_t* abort_dev = nullptr;

    DirectRendezvous() = default;
    DirectRendezvous(const DirectRendezvous&) = delete;
    DirectRendezvous& operator=(const DirectRendezvous&) = delete;
    ~DirectRendezvous() {      // in this order: the frame mappings, the block, its name, the abort word
        for (uint16_t* p : peer_frame) if (p) (void)hipIpcCloseMemHandle(p);
        if (shm) { if (registered) (void)hipHostUnregister(shm); munmap(shm, sizeof(DirectShm)); }
        if (root && name[0]) shm_unlink(name);
        if (abort_host) (void)hipHostFree(abort_host);
    }
    hipError_t create_abort_word() {
        hipError_t e = hipHostMalloc((void**)&abort_host, sizeof(uint32_t), hipHostMallocMapped);
        if (e == hipSuccess) { *abort_host = 0u; e = hipHostGetDevicePointer((void**)&abort_dev, abort_host, 0); }
        return e;
    }
    void raise_abort() { if (abort_host) __atomic_store_n(abort_host, 1u, __ATOMIC_RELEASE); }
    // The rendezvous: shared block, the root's IPC handles (of `root_frame`), every rank's mapping.  The host-side
    // waits share ONE deadline, the communicator's timeout from t0 on.  A failure leaves what it got to the destructor.
    int attach(vct_ctx* c, const void* id128, int rank, int world, int timeout_ms, const VctBuf<uint16_t> root_frame[2]) {
        if (world > VCT_DIRECT_MAX_RANKS) return vct_fail(c, VCT_ERR_INVALID, "direct slabs: at most 64 ranks");
        const unsigned char* id = (const unsigned char*)id128;
        snprintf(name, sizeof(name), "/vct_%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x%02x", id[0], id[1], id[2], id[3],
                 id[4], id[5], id[6], id[7], id[8], id[9], id[10], id[11]);
        root = rank == 0;
        const auto t0 = std::chrono::steady_clock::now();
        auto wait = [&](auto pred) { return wait_until(pred, timeout_ms, false, t0); };
        int fd = -1;
        if (root) {
            shm_unlink(name);
            fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
            if (fd < 0 || ftruncate(fd, sizeof(DirectShm)) != 0) { if (fd >= 0) close(fd); return vct_fail(c, VCT_ERR_DEVICE, "direct slabs: cannot create the rendezvous block"); }
        } else {
            if (!wait([&] { return (fd = shm_open(name, O_RDWR, 0600)) >= 0; }))
                return vct_fail(c, VCT_ERR_DEVICE, "direct slabs: the root's rendezvous block never appeared");
            struct stat st;
            if (!wait([&] { return fstat(fd, &st) != 0 || (size_t)st.st_size >= sizeof(DirectShm); })) {      // created, not sized yet
                close(fd);
                return vct_fail(c, VCT_ERR_DEVICE, "direct slabs: rendezvous block not sized");
            }
        }
        void* p = mmap(nullptr, sizeof(DirectShm), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        close(fd);
        if (p == MAP_FAILED) return vct_fail(c, VCT_ERR_DEVICE, "direct slabs: mmap failed");
        shm = (DirectShm*)p;
        hipError_t e = hipHostRegister(p, sizeof(DirectShm), hipHostRegisterMapped | hipHostRegisterPortable);
        registered = e == hipSuccess;
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&shm_dev, p, 0);
        if (e != hipSuccess) return vct_fail(c, VCT_ERR_DEVICE, std::string("direct slabs: hipHostRegister: ") + hipGetErrorString(e));
        if (root) {
            shm->world = (uint32_t)world;
            for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipIpcGetMemHandle(&shm->frame[k], root_frame[k].get());
            if (e != hipSuccess) return vct_fail(c, VCT_ERR_DEVICE, std::string("direct slabs: hipIpcGetMemHandle: ") + hipGetErrorString(e));
            shm->magic = 0x56435444u;
            __atomic_store_n(&shm->handles_ready, 1u, __ATOMIC_RELEASE);
            for (int r = 1; r < world; ++r)
                if (!wait([&] { return __atomic_load_n(&shm->attached[r], __ATOMIC_ACQUIRE) != 0u; }))
                    return vct_fail(c, VCT_ERR_DEVICE, "direct slabs: rank " + std::to_string(r) + " never attached");
        } else {
            if (!wait([&] { return __atomic_load_n(&shm->handles_ready, __ATOMIC_ACQUIRE) != 0u; }))
                return vct_fail(c, VCT_ERR_DEVICE, "direct slabs: the root never published its frame buffers");
            for (int k = 0; k < 2 && e == hipSuccess; ++k)
                e = hipIpcOpenMemHandle((void**)&peer_frame[k], shm->frame[k], hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) return vct_fail(c, VCT_ERR_DEVICE, std::string("direct slabs: hipIpcOpenMemHandle: ") + hipGetErrorString(e));
            __atomic_store_n(&shm->attached[rank], 1u, __ATOMIC_RELEASE);
        }
        return VCT_OK;
    }
};

}  // namespace

// The ORDER of the owning members is the teardown order read backwards, and a correctness requirement: ~vct_comm drains
// the streams, then the rendezvous goes (IPC mappings, hipHostUnregister + munmap, shm_unlink on the root, abort word),
// then the RCCL communicator, then buffers and events, and last of all the communication stream.
struct vct_comm {
    VctStream comm_stream;
    VctEvent traced[2], gathered[2];
    VctEvent g0[2], g1[2];             // timing: around the frame's exchange step
    VctBuf<uint16_t> buf[2];           // root: the frame (world padded slabs); others: this rank's slab (none in direct mode)
    VctBuf<uint16_t> il_frame[2];      // root only, see `interleaved`
    RcclComm comm;
    DirectRendezvous rv;               // direct slabs (VCT_COMM_MODE=direct): no RCCL communicator; see DirectShm above
    int rank = 0, world = 1;
    int row0 = 0, row1 = 0;            // tile rows of this rank's slab
    size_t slab_halves = 0;            // halves per padded slab of the EQUAL partition (the gather's sendcount)
    // load-aware partition (vct_comm_set_slab_rows): tile-row boundaries of every rank, [world + 1]; empty = the equal
    // partition above.  Uneven slabs travel by grouped ncclSend / ncclRecv straight to their rows of the root's frame.
    std::vector<int> starts;
    // Interleaved slabs (vct_comm_set_interleaved): tile row r belongs to rank r % world -- every rank samples the whole
    // frame, so the slabs cost the same BY CONSTRUCTION (no histogram, no feedback rounds).  A rank traces its rows back
    // to back into its padded slab, the slabs travel with the one equal-count ncclGather, and the root de-interleaves
    // them into `il_frame` (one 8-byte copy per pixel on the communication stream, behind the gather).
    bool interleaved = false;
    // VCT_COMM_STREAM=same: the gather is issued on the context's stream right behind the trace instead of on the
    // communication stream behind an event (profiles/experiments/README.md "gather beside the next trace")
    bool same_stream = false;
    unsigned long long frames = 0;     // steps issued
    int last = -1;                     // buffer of the last issued step
    bool direct = false;
    hipStream_t ctx_stream = nullptr;  // the context's stream (direct mode queues flag kernels and peer stores on it: drained at teardown)
    hipStream_t ctx_stream2 = nullptr; // ... and the other frame slot's, when the context runs two frames in flight
    long long wall_khz = 100000;       // wall_clock64 rate of this device (hipDeviceAttributeWallClockRate)
    int timeout_ms = 60000;            // vct_comm_sync gives up after this long and aborts the communicator
    bool broken = false;               // the communicator was aborted (a peer died or hung): only vct_comm_destroy is left

    ~vct_comm() {
        if (direct) {
            // Direct slabs: flag waits and the trace kernels that store into the root's mapped frame may still be QUEUED
            // (a host-side deadline fires before a wait that sits behind long compute has even started).  They must have
            // left the GPU before the mappings they use go away -- so: raise the abort word (every wait of this process
            // returns at its next poll; each is deadline-bounded anyway), drain BOTH streams, and only then close the IPC
            // handles and unregister the block.  Cannot hang: nothing left in the queues waits on a peer.
            rv.raise_abort();
            if (ctx_stream) (void)hipStreamSynchronize(ctx_stream);
            if (ctx_stream2) (void)hipStreamSynchronize(ctx_stream2);
            if (comm_stream) (void)hipStreamSynchronize(comm_stream.get());
        } else if (comm_stream && !broken) {
            (void)hipStreamSynchronize(comm_stream.get());
        }
        if (broken) comm.abort();      // (not destroyed: that would wait for the peers.  Direct slabs have none.)
    }
    // direct slabs, step f: its generation, and the flag waits' deadline in wall_clock64 ticks (ticks per ms = the rate in kHz)
    uint32_t gen() const { return (uint32_t)(frames >> 1) + 1u; }
    long long ticks() const { return (long long)timeout_ms * wall_khz; }
};

// An RCCL call failed: the communicator may be half way through a collective the peers will never finish, so it
// is aborted and the context keeps only the error.
static int comm_fail(vct_ctx* c, vct_comm* m, const std::string& what, ncclResult_t r) {
    std::string msg = what + ": " + (rccl()->GetErrorString ? rccl()->GetErrorString(r) : "RCCL error");
    if (m->comm.abort()) msg += " (communicator aborted)";
    m->broken = true;
    return vct_fail(c, VCT_ERR_DEVICE, msg);
}

static size_t row_halves(const vct_ctx* c) { return (size_t)VCT_TILE * c->cfg.width * 4; }      // RGBA16F halves of one tile row
static int launched(vct_ctx* c) { HIP_TRY(c, hipGetLastError()); return VCT_OK; }      // what the launch just issued came to

// the root's de-interleave of `world` gathered slabs into a frame (k_deinterleave), on stream s
static int launch_deinterleave(vct_ctx* c, hipStream_t s, const void* gathered, void* frame, int world, size_t slab_pixels) {
    hipLaunchKernelGGL(k_deinterleave, dim3(2048), dim3(256), 0, s, (const uint2*)gathered, (uint2*)frame, c->cfg.width,
                       c->cfg.height, world, slab_pixels);
    return launched(c);
}

void vct_comm_release(vct_ctx* c) {
    if (!c || !c->comm) return;
    // (frame slots may have been added or switched since vct_comm_init: the streams that carry this communicator's work NOW)
    c->comm->ctx_stream = cur(c).stream.get();
    c->comm->ctx_stream2 = c->frames_in_flight > 1 ? other(c).stream.get() : nullptr;
    delete c->comm;
    c->comm = nullptr;
}

// slab of the attached communicator (vct_api_trace.hip: vct_gi_pass on a rank context); false when there is none
bool vct_comm_rows(const vct_ctx* c, int* row0, int* row1) {
    if (!c || !c->comm) return false;
    *row0 = c->comm->row0;
    *row1 = c->comm->row1;
    if (c->comm->interleaved) { *row0 = 0; *row1 = vct_tiles_y(c); }      // its rows are spread over the whole frame
    return true;
}

extern "C" {

int vct_slab_partition(int32_t height, int32_t world, int32_t rank, int32_t* row0, int32_t* row1,
                       int32_t* rows_per_rank) {
    if (height <= 0 || world <= 0 || rank < 0 || rank >= world) return VCT_ERR_INVALID;
    const int ty = (height + VCT_TILE - 1) / VCT_TILE;
    const int per = (ty + world - 1) / world;
    const int r0 = rank * per < ty ? rank * per : ty;
    if (row0) *row0 = r0;
    if (row1) *row1 = r0 + per < ty ? r0 + per : ty;
    if (rows_per_rank) *rows_per_rank = per;
    return VCT_OK;
}

// Equal-WORK boundaries from a per-tile-row cost histogram (e.g. the executed cone steps per tile row of the previous
// frame, vct_last_row_steps): starts[r] = first tile row of rank r, starts[world] = tile_rows, chosen so that every
// slab's cost is as close to total / world as whole rows allow.  Pure host arithmetic; every rank computes the same
// boundaries from the same (all-reduced or root-broadcast) histogram.
int vct_slab_partition_weighted(const uint64_t* row_cost, int32_t tile_rows, int32_t world, int32_t* starts) {
    if (!row_cost || !starts || tile_rows <= 0 || world <= 0) return VCT_ERR_INVALID;
    long double total = 0.0L;
    for (int i = 0; i < tile_rows; ++i) total += (long double)row_cost[i] + 1.0L;     // +1: empty rows still cost a launch slot
    starts[0] = 0;
    long double acc = 0.0L;
    int row = 0;
    for (int r = 1; r < world; ++r) {
        const long double want = total * (long double)r / (long double)world;
        // advance while taking the next row leaves the prefix closer to the target than stopping here
        while (row < tile_rows) {
            const long double with = acc + (long double)row_cost[row] + 1.0L;
            if (with <= want || (with - want) < (want - acc)) { acc = with; ++row; } else break;
        }
        // every remaining rank must still be able to get a (possibly empty) slab inside the frame
        if (row < starts[r - 1]) row = starts[r - 1];
        starts[r] = row;
    }
    starts[world] = tile_rows;
    return VCT_OK;
}

int vct_comm_get_unique_id(void* id128) {
    if (!id128) return VCT_ERR_INVALID;
    if (direct_mode()) {              // direct slabs never touch RCCL: any 128 unpredictable bytes name the rendezvous
        FILE* fp = fopen("/dev/urandom", "rb");
        const bool ok = fp && fread(id128, 1, 128, fp) == 128;
        if (fp) fclose(fp);
        return ok ? VCT_OK : vct_fail(nullptr, VCT_ERR_DEVICE, "vct_comm_get_unique_id: /dev/urandom unreadable");
    }
    Rccl* r = rccl();
    if (!r->err.empty()) return vct_fail(nullptr, VCT_ERR_DEVICE, r->err);
    ncclUniqueId id;
    if (r->GetUniqueId(&id) != ncclSuccess) return vct_fail(nullptr, VCT_ERR_DEVICE, "ncclGetUniqueId failed");
    memcpy(id128, id.internal, 128);
    return VCT_OK;
}

// All or nothing: the communicator is built into a local object and attached to the context only when every
// allocation and the rendezvous / ncclCommInitRank succeeded; on any failure the local object goes with the scope and
// the context is as before (a retry is possible, vct_frame_step keeps refusing).
int vct_comm_init(vct_ctx* c, const void* id128, int32_t rank, int32_t world) {
    if (!c) return VCT_ERR_INVALID;
    if (!id128 || world <= 0 || rank < 0 || rank >= world) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_init: bad rank / world / id");
    if (c->comm) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_init: already initialised (vct_comm_destroy first)");
    PIPE_TRY(vct_refuse_conflict(c, "vct_comm_init", vct_rules_in_force(c).features, VCT_MODE_COMM));
    const bool direct = direct_mode();
    Rccl* r = direct ? nullptr : rccl();
    if (r && !r->err.empty()) return vct_fail(c, VCT_ERR_DEVICE, r->err);
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<vct_comm> m(new vct_comm());
    m->rank = rank;
    m->world = world;
    m->direct = direct;
    int rows_per_rank = 0;
    vct_slab_partition(c->cfg.height, world, rank, &m->row0, &m->row1, &rows_per_rank);
    m->slab_halves = (size_t)rows_per_rank * row_halves(c);
    const size_t buf_halves = rank == 0 ? m->slab_halves * world : m->slab_halves;      // allocation of each gather buffer
    if (const char* t = getenv("VCT_COMM_TIMEOUT_MS")) { const int v = atoi(t); if (v > 0) m->timeout_ms = v; }
    if (const char* t = getenv("VCT_COMM_STREAM")) m->same_stream = t[0] == 's';
    hipError_t e;
    hipStream_t cs = nullptr;
    if (c->reserved_cus > 0) {       // the CUs the context's streams leave alone (VCT_COMM_RESERVED_CUS)
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, c->device);
        if (e == hipSuccess) e = vct_create_masked_stream(&cs, c->device, prop.multiProcessorCount - c->reserved_cus, prop.multiProcessorCount);
    } else {
        // the exchange step is meant to run beside the next frame's trace: a stream that shares the context stream's hardware
        // queue would run behind it instead (round 6: HIP hands out four queues; RCCL and torch hold streams of their own)
        bool overlaps = false;
        e = vct_create_overlapping_stream(c, cur(c).stream.get(), &cs, &overlaps) == VCT_OK ? hipSuccess : hipErrorUnknown;
    }
    m->comm_stream.adopt(cs);
    m->ctx_stream = cur(c).stream.get();
    if (direct && e == hipSuccess) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0) m->wall_khz = khz;
        e = m->rv.create_abort_word();
    }
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        if (direct && rank == 0) {
            // Direct mode: peers store into the root's frame over IPC / xGMI and the root's next kernel reads it with only
            // a kernel-boundary acquire, which need not invalidate lines of LOCAL coarse-grained memory that the root's L2
            // kept from an earlier frame.  Fine-grained memory is not cached that way, so the frame buffers peers write
            // are allocated fine-grained (advisor, round 5); no fallback -- a coarse-grained frame could be silently stale.
            uint16_t* p = nullptr;
            e = hipExtMallocWithFlags((void**)&p, buf_halves * 2, hipDeviceMallocFinegrained);
            if (e == hipSuccess) m->buf[k].adopt(p, buf_halves);
        } else if (!direct) {        // (a rank of the direct mode owns no slab buffer: it writes the root's)
            e = m->buf[k].alloc(buf_halves);
        }
        if (e == hipSuccess && m->buf[k]) e = hipMemsetAsync(m->buf[k].get(), 0, buf_halves * 2, cur(c).stream.get());
        if (e == hipSuccess) e = m->traced[k].create(hipEventDisableTiming);
        if (e == hipSuccess) e = m->gathered[k].create(hipEventDisableTiming);
        if (e == hipSuccess) e = m->g0[k].create();
        if (e == hipSuccess) e = m->g1[k].create();
        if (e == hipSuccess) e = hipEventRecord(m->gathered[k].get(), cur(c).stream.get());      // "previous gather" of the first use
    }
    if (e == hipSuccess) e = hipStreamSynchronize(cur(c).stream.get());
    if (e != hipSuccess)
        return vct_fail(c, e == hipErrorOutOfMemory ? VCT_ERR_NOMEM : VCT_ERR_DEVICE, std::string("vct_comm_init: ") + hipGetErrorString(e));
    if (direct) {
        PIPE_TRY(m->rv.attach(c, id128, rank, world, m->timeout_ms, m->buf));
    } else {
        ncclUniqueId id;
        memcpy(id.internal, id128, 128);
        const ncclResult_t nr = r->CommInitRank(&m->comm.h, world, id, rank);
        if (nr != ncclSuccess) {
            m->comm.h = nullptr;          // nothing to destroy: ncclCommInitRank failed
            return vct_fail(c, VCT_ERR_DEVICE, std::string("ncclCommInitRank: ") + r->GetErrorString(nr));
        }
    }
    c->comm = m.release();
    return VCT_OK;
}

int vct_comm_destroy(vct_ctx* c) {
    if (!c) return VCT_ERR_INVALID;
    vct_comm_release(c);
    return VCT_OK;
}

int vct_comm_slab(vct_ctx* c, int32_t* row0, int32_t* row1) {
    if (!c) return VCT_ERR_INVALID;
    if (!c->comm) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_slab: call vct_comm_init first");
    if (row0) *row0 = c->comm->row0;
    if (row1) *row1 = c->comm->row1;
    return VCT_OK;
}

int vct_comm_set_timeout_ms(vct_ctx* c, int32_t ms) {
    if (!c) return VCT_ERR_INVALID;
    if (!c->comm) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_set_timeout_ms: call vct_comm_init first");
    if (ms <= 0) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_set_timeout_ms: timeout must be > 0");
    c->comm->timeout_ms = ms;
    return VCT_OK;
}

// Collective (every rank passes the same boundaries): slab r = tile rows [starts[r], starts[r+1]).  starts == NULL
// returns to the equal partition.  Frames in flight are drained first; a rank whose new slab outgrows its gather
// buffers gets larger ones.  Contiguous slabs and interleaved tile rows are alternatives: this call switches the
// interleaved assignment off (the last of vct_comm_set_slab_rows / vct_comm_set_interleaved wins).
int vct_comm_set_slab_rows(vct_ctx* c, const int32_t* starts) {
    if (!c) return VCT_ERR_INVALID;
    vct_comm* m = c->comm;
    if (!m || m->broken) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_set_slab_rows: no usable communicator (vct_comm_init)");
    const int ty = vct_tiles_y(c);
    if (starts) {
        if (starts[0] != 0 || starts[m->world] != ty) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_set_slab_rows: boundaries must run from 0 to the frame's tile rows");
        for (int r = 0; r < m->world; ++r)
            if (starts[r + 1] < starts[r]) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_set_slab_rows: boundaries must not decrease");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_comm_sync(c));
    m->interleaved = false;
    if (!starts) {
        m->starts.clear();
        vct_slab_partition(c->cfg.height, m->world, m->rank, &m->row0, &m->row1, nullptr);
    } else {
        m->starts.assign(starts, starts + m->world + 1);
        m->row0 = starts[m->rank];
        m->row1 = starts[m->rank + 1];
    }
    // (the root's frame never grows; direct slabs: a rank owns no buffer, it writes the root's frame)
    const size_t need = (size_t)(m->row1 - m->row0) * row_halves(c);
    if (m->rank != 0 && !m->direct && need > m->buf[0].size()) {
        VctBuf<uint16_t> nb[2];
        for (VctBuf<uint16_t>& b : nb) {
            const hipError_t e = b.alloc(need);
            if (e != hipSuccess) return vct_fail(c, VCT_ERR_NOMEM, std::string("vct_comm_set_slab_rows: ") + hipGetErrorString(e));
        }
        for (int k = 0; k < 2; ++k) m->buf[k] = std::move(nb[k]);
    }
    m->last = -1;
    return VCT_OK;
}

// Collective (every rank passes the same value): interleaved tile rows instead of contiguous slabs.  Frames in flight
// are drained first.  The load-aware boundaries are dropped (the two are alternatives).
int vct_comm_set_interleaved(vct_ctx* c, int32_t on) {
    if (!c) return VCT_ERR_INVALID;
    vct_comm* m = c->comm;
    if (!m || m->broken) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_set_interleaved: no usable communicator (vct_comm_init)");
    HIP_TRY(c, hipSetDevice(c->device));
    PIPE_TRY(vct_comm_sync(c));
    // the root's de-interleave target first: a failed allocation leaves this rank's state untouched.  (The other
    // ranks cannot see the root's failure: on VCT_ERR_NOMEM the caller must destroy the communicator on every rank.)
    if (on && m->rank == 0)
        for (VctBuf<uint16_t>& f : m->il_frame)
            if (!f) {
                const hipError_t e = f.alloc((size_t)c->cfg.width * c->cfg.height * 4);
                if (e != hipSuccess) return vct_fail(c, VCT_ERR_NOMEM, std::string("vct_comm_set_interleaved: ") + hipGetErrorString(e));
            }
    m->starts.clear();
    vct_slab_partition(c->cfg.height, m->world, m->rank, &m->row0, &m->row1, nullptr);
    m->interleaved = on != 0;
    if (m->interleaved) {
        const int ty = vct_tiles_y(c);
        m->row0 = m->rank < ty ? m->rank : ty;
        m->row1 = ty;
    }
    m->last = -1;
    return VCT_OK;
}

// ---- the exchange of one frame step: what runs on the exchange stream `cs` between the step's g0 and g1 events ---------

// the direct mode's flag kernels (see DirectShm)
static int flag_set(vct_ctx* c, hipStream_t s, uint32_t* flag, uint32_t v) {
    hipLaunchKernelGGL(k_flag_set, dim3(1), dim3(1), 0, s, flag, v);
    return launched(c);
}
static int flag_wait(vct_ctx* c, vct_comm* m, hipStream_t s, const uint32_t* flags, int n, uint32_t want) {
    hipLaunchKernelGGL(k_flag_wait, dim3(1), dim3(64), 0, s, flags, n, 1, want, &m->rv.shm_dev->timed_out, m->ticks(), m->rv.abort_dev);
    return launched(c);
}

static int exchange_rccl(vct_ctx* c, vct_comm* m, int k, hipStream_t cs) {
    Rccl* r = rccl();
    uint16_t* slab = m->buf[k].get();
    if (m->starts.empty()) {
        // ONE collective per frame, equal (padded) or interleaved slabs alike.  Root: in place (its slab already sits at
        // offset rank * sendcount = 0).
        const ncclResult_t nr = r->Gather(slab, m->rank == 0 ? slab : nullptr, m->slab_halves, ncclFloat16, 0, m->comm.h, cs);
        return nr == ncclSuccess ? VCT_OK : comm_fail(c, m, "ncclGather", nr);
    }
    // load-aware slabs differ in size: one fused group of point-to-point transfers, each slab straight to its
    // rows of the root's frame (what ncclGather is made of inside RCCL, with per-rank counts)
    ncclResult_t gr = r->GroupStart();
    if (gr != ncclSuccess) return comm_fail(c, m, "ncclGroupStart", gr);
    if (m->rank == 0) {
        for (int peer = 1; peer < m->world && gr == ncclSuccess; ++peer) {
            const size_t n = (size_t)(m->starts[peer + 1] - m->starts[peer]) * row_halves(c);
            if (n) gr = r->Recv(slab + (size_t)m->starts[peer] * row_halves(c), n, ncclFloat16, peer, m->comm.h, cs);
        }
    } else {
        const size_t n = (size_t)(m->row1 - m->row0) * row_halves(c);
        if (n) gr = r->Send(slab, n, ncclFloat16, 0, m->comm.h, cs);
    }
    const ncclResult_t ge = r->GroupEnd();
    if (gr != ncclSuccess) return comm_fail(c, m, "ncclSend/ncclRecv", gr);
    if (ge != ncclSuccess) return comm_fail(c, m, "ncclGroupEnd", ge);
    return VCT_OK;
}

static int exchange_direct_root(vct_ctx* c, vct_comm* m, int k, hipStream_t cs) {
    return m->world > 1 ? flag_wait(c, m, cs, &m->rv.shm_dev->done[k][1], m->world - 1, m->gen()) : VCT_OK;
}

static int exchange_direct_peer(vct_ctx* c, vct_comm* m, int k, hipStream_t cs) {
    return flag_set(c, cs, &m->rv.shm_dev->done[k][m->rank], m->gen());
}

// One frame: trace this rank's slab into gather buffer k and start its exchange.  Asynchronous.
int vct_frame_step(vct_ctx* c) {
    if (!c) return VCT_ERR_INVALID;
    vct_comm* m = c->comm;
    if (!m) return vct_fail(c, VCT_ERR_INVALID, "vct_frame_step: call vct_comm_init first");
    if (m->broken || (!m->comm.h && !m->direct)) return vct_fail(c, VCT_ERR_DEVICE, "vct_frame_step: the communicator was aborted (vct_comm_destroy, then vct_comm_init again)");
    if (!cur(c).have_gbuffer) return vct_fail(c, VCT_ERR_INVALID, "vct_frame_step: no G-buffer resident yet");
    HIP_TRY(c, hipSetDevice(c->device));
    const int k = (int)(m->frames & 1ull);
    const hipStream_t ts = cur(c).stream.get();
    const bool peer = m->direct && m->rank != 0;      // stores its slab straight into the root's mapped frame
    HIP_TRY(c, hipStreamWaitEvent(ts, m->gathered[k].get(), 0));    // buffer k is free once its last gather is done
    if (m->direct)      // the root releases buffer k (it is past frame f - 2), a peer waits for that
        PIPE_TRY(peer ? flag_wait(c, m, ts, &m->rv.shm_dev->release[k], 1, m->gen() - 1u)
                      : flag_set(c, ts, &m->rv.shm_dev->release[k], m->gen() - 1u));
    // This rank's slab: the start of its own buffer k (the root's slab always begins at tile row 0: the frame buffer
    // itself, in-place gather), or its place in the root's mapped buffer k -- packed slab `rank` (equal / interleaved)
    // or its own rows.  Contiguous slabs: the kernel addresses the full frame, so it gets the slab's address minus the
    // slab's first row as its output base -- passed to the launch, never stored in the context (on a non-root rank
    // that address lies before the allocation).  Interleaved: every world-th tile row from `rank` on, back to back
    // at the start of the slab.  An empty slab launches nothing.
    uint16_t* slab = !peer ? m->buf[k].get()
                           : m->rv.peer_frame[k] + (m->starts.empty() ? (size_t)m->rank * m->slab_halves : (size_t)m->row0 * row_halves(c));
    const bool il = m->interleaved;
    PIPE_TRY(vct_launch_trace_rows(c, m->row0, m->row1, il ? slab : slab - (size_t)m->row0 * row_halves(c), il ? m->world : 1, il));
    // The exchange stream, ordered behind the trace.  (A peer's exchange is one flag store behind its own stores:
    // always on the context's stream, no `traced` event.)
    const bool behind_trace = m->same_stream || peer;
    const hipStream_t cs = behind_trace ? ts : m->comm_stream.get();
    if (!behind_trace) {
        HIP_TRY(c, hipEventRecord(m->traced[k].get(), ts));
        HIP_TRY(c, hipStreamWaitEvent(cs, m->traced[k].get(), 0));
    }
    HIP_TRY(c, hipEventRecord(m->g0[k].get(), cs));
    PIPE_TRY(!m->direct ? exchange_rccl(c, m, k, cs) : peer ? exchange_direct_peer(c, m, k, cs) : exchange_direct_root(c, m, k, cs));
    if (il && m->rank == 0)      // the root has every rank's packed slab in buffer k: its rows go to their places in the frame
        PIPE_TRY(launch_deinterleave(c, cs, m->buf[k].get(), m->il_frame[k].get(), m->world, m->slab_halves / 4));
    HIP_TRY(c, hipEventRecord(m->g1[k].get(), cs));
    HIP_TRY(c, hipEventRecord(m->gathered[k].get(), cs));
    m->last = k;
    ++m->frames;
    return VCT_OK;
}

// Waits for the trace and the gather streams -- with a deadline: a rank that died or hangs leaves its peers inside
// the collective forever, so after timeout_ms (vct_comm_set_timeout_ms / VCT_COMM_TIMEOUT_MS, default 60 s) or on an
// asynchronous RCCL error the communicator is aborted and the call fails; the context itself stays usable for
// single-GPU calls after vct_comm_destroy.
int vct_comm_sync(vct_ctx* c) {
    if (!c) return VCT_ERR_INVALID;
    vct_comm* m = c->comm;
    if (!m) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_sync: call vct_comm_init first");
    if (m->broken) return vct_fail(c, VCT_ERR_DEVICE, "vct_comm_sync: the communicator was aborted");
    HIP_TRY(c, hipSetDevice(c->device));
    // BOTH streams are polled under the deadline: with frames issued back to back the context stream itself waits on
    // gathered[k] (vct_frame_step), i.e. behind a collective a dead peer never finishes -- a blocking
    // hipStreamSynchronize of the context stream here would hang before the deadline loop was ever reached.
    // After the abort below the stuck collective's kernel ends, its event completes and both streams drain.
    // Compute queued on the context's stream in front of the exchange (several 4K / 1024^3 GI passes, a first-use divisor
    // self-test) is not communication: it gets a deadline of its own -- the last step's "slab traced" event -- and the
    // communication deadline starts when that has fired (advisor, round 4).  Both are bounded: a trace that waits behind
    // the gather of a dead peer two frames back never fires the event, and the second wait then aborts as before.
    if (m->last >= 0 && !m->same_stream && !m->direct && m->traced[m->last])
        (void)wait_until([&] { return hipEventQuery(m->traced[m->last].get()) != hipErrorNotReady; }, m->timeout_ms, true);
    const int pending = 1;      // (no VCT_* code: those are <= 0)
    auto poll = [&]() -> int {
        hipError_t qc = hipStreamQuery(cur(c).stream.get());
        if (qc != hipSuccess && qc != hipErrorNotReady) HIP_TRY(c, qc);
        if (qc == hipSuccess && c->frames_in_flight > 1) {      // two frames in flight: the other slot's stream carries steps too
            qc = hipStreamQuery(other(c).stream.get());
            if (qc != hipSuccess && qc != hipErrorNotReady) HIP_TRY(c, qc);
        }
        const hipError_t q = hipStreamQuery(m->comm_stream.get());
        if (q == hipSuccess && qc == hipSuccess) {
            if (m->direct && __atomic_load_n(&m->rv.shm->timed_out, __ATOMIC_ACQUIRE)) {
                m->broken = true;
                return vct_fail(c, VCT_ERR_DEVICE, "vct_comm_sync: a rank's flag wait gave up after " + std::to_string(m->timeout_ms) +
                                                   " ms (a peer died or hangs); the frame is incomplete, communicator unusable");
            }
            return VCT_OK;
        }
        if (q != hipSuccess && q != hipErrorNotReady) HIP_TRY(c, q);
        ncclResult_t async = ncclSuccess;
        if (m->comm.h && rccl()->CommGetAsyncError && rccl()->CommGetAsyncError(m->comm.h, &async) == ncclSuccess &&
            async != ncclSuccess && async != ncclInProgress)
            return comm_fail(c, m, "vct_comm_sync: asynchronous RCCL error", async);
        return pending;
    };
    int rc = pending;
    if (wait_until([&] { return (rc = poll()) != pending; }, m->timeout_ms, true)) return rc;      // the common case: done within microseconds
    m->comm.abort();
    m->broken = true;
    return vct_fail(c, VCT_ERR_DEVICE, "vct_comm_sync: the gather did not complete within " + std::to_string(m->timeout_ms) +
                                       " ms (a peer rank died or hangs); communicator aborted");
}

// Diagnostics for multi-GPU bench lines: what RCCL itself says about the communicator.
// out[0] = ncclCommCount, out[1] = ncclCommUserRank, out[2] = ncclCommCuDevice, out[3] = ncclGetVersion (-1: not exported)
int vct_comm_info(vct_ctx* c, int32_t out[4]) {
    if (!c || !out) return VCT_ERR_INVALID;
    vct_comm* m = c->comm;
    if (m && m->direct) {        // direct slabs: no RCCL; what the rendezvous block says, version 0
        out[0] = (int32_t)m->rv.shm->world; out[1] = m->rank; out[2] = c->device; out[3] = 0;
        return VCT_OK;
    }
    if (!m || !m->comm.h) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_info: no usable communicator (vct_comm_init)");
    Rccl* r = rccl();
    int v[4] = {-1, -1, -1, -1};
    if (r->CommCount) (void)r->CommCount(m->comm.h, &v[0]);
    if (r->CommUserRank) (void)r->CommUserRank(m->comm.h, &v[1]);
    if (r->CommCuDevice) (void)r->CommCuDevice(m->comm.h, &v[2]);
    if (r->GetVersion) (void)r->GetVersion(&v[3]);
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    return VCT_OK;
}

// Device time of the LAST frame's exchange step on this rank (the ncclGather / the send-recv group, plus the root's
// de-interleave in interleaved mode), between two events on the stream it ran on.  Waits for that step (vct_comm_sync).
int vct_comm_last_gather_ms(vct_ctx* c, float* ms) {
    if (!c || !ms) return VCT_ERR_INVALID;
    vct_comm* m = c->comm;
    if (!m || m->last < 0) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_last_gather_ms: no frame stepped yet");
    PIPE_TRY(vct_comm_sync(c));
    HIP_TRY(c, hipEventElapsedTime(ms, m->g0[m->last].get(), m->g1[m->last].get()));
    return VCT_OK;
}

int vct_comm_frame(vct_ctx* c, void** dev, size_t* bytes) {
    if (!c || !dev) return VCT_ERR_INVALID;
    vct_comm* m = c->comm;
    if (!m || m->last < 0) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_frame: no frame gathered yet");
    if (m->rank != 0) return vct_fail(c, VCT_ERR_INVALID, "vct_comm_frame: only the root (rank 0) holds the frame");
    *dev = m->interleaved ? m->il_frame[m->last].get() : m->buf[m->last].get();
    if (bytes) *bytes = (size_t)c->cfg.width * c->cfg.height * 8;
    return VCT_OK;
}

int vct_comm_download_frame(vct_ctx* c, void* out) {
    if (!c || !out) return VCT_ERR_INVALID;
    void* dev = nullptr;
    size_t bytes = 0;
    int rc = vct_comm_frame(c, &dev, &bytes);
    if (rc) return rc;
    rc = vct_comm_sync(c);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(out, dev, bytes, hipMemcpyDeviceToHost));
    return VCT_OK;
}

// The interleaved step's data path on ONE GPU, for any world size (no multi-GPU box is needed to check it): the resident
// G-buffer is traced once per emulated rank -- its rows, strided and packed, into slab `rank` of a stand-in gather
// buffer, exactly as vct_frame_step does -- the root's de-interleave kernel runs over that buffer, and the result is
// compared with the frame one launch traces.  *mismatches = pixels that differ (0 expected).
int vct_selftest_interleaved(vct_ctx* c, int32_t world, uint64_t* mismatches) {
    if (!c || !mismatches || world < 1) return VCT_ERR_INVALID;
    if (!cur(c).have_gbuffer) return vct_fail(c, VCT_ERR_INVALID, "vct_selftest_interleaved: no G-buffer resident yet");
    HIP_TRY(c, hipSetDevice(c->device));
    const int w = c->cfg.width, h = c->cfg.height, ty = vct_tiles_y(c);
    const int per = (ty + world - 1) / world;
    const size_t slab_pixels = (size_t)per * VCT_TILE * w, npix = (size_t)w * h;
    VctBuf<uint2> gathered, il, plain;
    if (gathered.alloc(slab_pixels * world) != hipSuccess || il.alloc(npix) != hipSuccess || plain.alloc(npix) != hipSuccess)
        return vct_fail(c, VCT_ERR_NOMEM, "vct_selftest_interleaved: out of memory");
    hipError_t e = hipMemsetAsync(gathered.get(), 0, slab_pixels * world * 8, cur(c).stream.get());
    if (e == hipSuccess) e = hipMemsetAsync(plain.get(), 0, npix * 8, cur(c).stream.get());
    if (e != hipSuccess) return vct_fail(c, VCT_ERR_DEVICE, hipGetErrorString(e));
    for (int r = 0; r < world; ++r)
        PIPE_TRY(vct_launch_trace_rows(c, r < ty ? r : ty, ty, (uint16_t*)(gathered.get() + slab_pixels * r), world, true));
    PIPE_TRY(launch_deinterleave(c, cur(c).stream.get(), gathered.get(), il.get(), world, slab_pixels));
    PIPE_TRY(vct_launch_trace_rows(c, 0, ty, (uint16_t*)plain.get()));
    std::vector<uint2> a(npix), b(npix);
    e = hipStreamSynchronize(cur(c).stream.get());
    if (e == hipSuccess) e = hipMemcpy(a.data(), il.get(), npix * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(b.data(), plain.get(), npix * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return vct_fail(c, VCT_ERR_DEVICE, hipGetErrorString(e));
    uint64_t bad = 0;
    for (size_t i = 0; i < npix; ++i) bad += (a[i].x != b[i].x || a[i].y != b[i].y) ? 1u : 0u;
    *mismatches = bad;
    return VCT_OK;
}

}  // extern "C"
