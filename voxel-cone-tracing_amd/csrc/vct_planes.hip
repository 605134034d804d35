// vct_planes.hip -- the tiled per-pixel planes of a frame slot: the G-buffer [tile][23][64] floats, the pixel-emission and
// lit planes [tile][3][64] floats, the pixel-gloss plane [tile][64] bytes.  The two layout kernels, and what every kind of
// plane does the same way on the host: a zeroed buffer for a slot that has none, attaching to every live slot, taking a
// caller's array, downloading.
#include "vct_ctx.h"

namespace {

// planes [NPLANES][h*w] -> tiled [tile][NPLANES][64]; pixels outside the frame are zero (albedo.a = 0).
template <class T, int NPLANES>
__global__ void k_tile_gbuffer(const T* __restrict__ planes, T* __restrict__ tiled, int w,
                               int h, int tiles_x, int tiles_y) {
    const size_t total = (size_t)tiles_x * tiles_y * NPLANES * VCT_TILE_PIX;
    const size_t npix = (size_t)w * h;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const size_t r = i >> 6;
        const int plane = (int)(r % NPLANES);
        const size_t tile = r / NPLANES;
        const int ty = (int)(tile / tiles_x), tx = (int)(tile - (size_t)ty * tiles_x);
        const int x = tx * VCT_TILE + (lane & 7), y = ty * VCT_TILE + (lane >> 3);
        T v = (T)0;
        if (x < w && y < h) v = planes[(size_t)plane * npix + (size_t)y * w + x];
        tiled[i] = v;
    }
}

// tiled [tile][NPLANES][64] -> linear planes [NPLANES][h*w] (downloads / tests)
template <class T, int NPLANES>
__global__ void k_untile_gbuffer(const T* __restrict__ tiled, T* __restrict__ planes, int w, int h,
                                 int tiles_x) {
    const size_t npix = (size_t)w * h;
    const size_t total = npix * NPLANES;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int plane = (int)(i / npix);
        const size_t pix = i - (size_t)plane * npix;
        const int y = (int)(pix / w), x = (int)(pix - (size_t)y * w);
        const size_t tile = (size_t)(y / VCT_TILE) * tiles_x + x / VCT_TILE;
        const int lane = (y % VCT_TILE) * VCT_TILE + (x % VCT_TILE);
        planes[i] = tiled[(tile * NPLANES + plane) * VCT_TILE_PIX + lane];
    }
}

inline int grid_for(size_t n, int threads) {
    size_t b = (n + threads - 1) / threads;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (int)b;
}

template <class T, int NPLANES>
void tile(const void* linear, void* tiled, int w, int h, hipStream_t s) {
    const int tx = (w + VCT_TILE - 1) / VCT_TILE, ty = (h + VCT_TILE - 1) / VCT_TILE;
    const size_t n = (size_t)tx * ty * NPLANES * VCT_TILE_PIX;
    hipLaunchKernelGGL((k_tile_gbuffer<T, NPLANES>), dim3(grid_for(n, 256)), dim3(256), 0, s, (const T*)linear, (T*)tiled,
                       w, h, tx, ty);
}
template <class T, int NPLANES>
void untile(const void* tiled, void* linear, int w, int h, hipStream_t s) {
    const int tx = (w + VCT_TILE - 1) / VCT_TILE;
    hipLaunchKernelGGL((k_untile_gbuffer<T, NPLANES>), dim3(256 * 8), dim3(256), 0, s, (const T*)tiled, (T*)linear, w, h, tx);
}

size_t tiled_elems(const vct_ctx* c, int nplanes) { return (size_t)vct_tiles_x(c) * vct_tiles_y(c) * nplanes * VCT_TILE_PIX; }

}  // namespace

// The kinds of planes there are: 23 or 3 planes of floats, one plane of bytes.  Another kind is an error, not a fall-back.
hipError_t vct_launch_tile_planes(const void* linear, void* tiled, int nplanes, size_t elem, int w, int h, hipStream_t s) {
    if (elem == sizeof(float) && nplanes == VCT_GB_NPLANES) tile<float, VCT_GB_NPLANES>(linear, tiled, w, h, s);
    else if (elem == sizeof(float) && nplanes == VCT_EMIS_NPLANES) tile<float, VCT_EMIS_NPLANES>(linear, tiled, w, h, s);
    else if (elem == 1 && nplanes == 1) tile<uint8_t, 1>(linear, tiled, w, h, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t vct_launch_untile_planes(const void* tiled, void* linear, int nplanes, size_t elem, int w, int h, hipStream_t s) {
    if (elem == sizeof(float) && nplanes == VCT_GB_NPLANES) untile<float, VCT_GB_NPLANES>(tiled, linear, w, h, s);
    else if (elem == sizeof(float) && nplanes == VCT_EMIS_NPLANES) untile<float, VCT_EMIS_NPLANES>(tiled, linear, w, h, s);
    else if (elem == 1 && nplanes == 1) untile<uint8_t, 1>(tiled, linear, w, h, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <class T>
hipError_t vct_planes_ensure(VctBuf<T>& b, size_t n, hipStream_t s, bool* fresh) {
    if (b) return hipSuccess;
    hipError_t e = b.alloc(n);
    if (e == hipSuccess) e = hipMemsetAsync(b.get(), 0, n * sizeof(T), s);
    if (e != hipSuccess) b.reset();
    else if (fresh) *fresh = true;
    return e;
}
template hipError_t vct_planes_ensure<float>(VctBuf<float>&, size_t, hipStream_t, bool*);
template hipError_t vct_planes_ensure<uint8_t>(VctBuf<uint8_t>&, size_t, hipStream_t, bool*);

int vct_planes_attach(vct_ctx* c, const char* who, VctPlanesEnsure* ensure, VctPlanesDrop* drop, hipError_t e) {
    bool fresh[2] = {false, false};
    for (int k = 0; k < c->frames_in_flight && e == hipSuccess; ++k) {
        e = ensure(c, c->slots[k], &fresh[k]);
        if (e == hipSuccess) e = hipStreamSynchronize(c->slots[k].stream.get());
    }
    if (e == hipSuccess) return VCT_OK;
    for (int k = 0; k < 2; ++k)
        if (fresh[k]) drop(c->slots[k]);
    return vct_fail(c, e == hipErrorOutOfMemory ? VCT_ERR_NOMEM : VCT_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
}

int vct_planes_set(vct_ctx* c, void* tiled, const void* src, int32_t layout, int32_t location, int nplanes, size_t elem) {
    hipStream_t s = cur(c).stream.get();
    const size_t npix = (size_t)c->cfg.width * c->cfg.height;
    if (layout == VCT_GB_TILED) {
        HIP_TRY(c, hipMemcpyAsync(tiled, src, tiled_elems(c, nplanes) * elem,
                                  location == VCT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    } else {
        if (location == VCT_MEM_HOST) {
            PIPE_TRY(vct_staging_free(c));
            HIP_TRY(c, c->gb_linear.reserve(npix * VCT_GB_NPLANES));
            HIP_TRY(c, hipMemcpyAsync(c->gb_linear.get(), src, npix * nplanes * elem, hipMemcpyHostToDevice, s));
            src = c->gb_linear.get();
        }
        HIP_TRY(c, vct_launch_tile_planes(src, tiled, nplanes, elem, c->cfg.width, c->cfg.height, s));
    }
    if (location == VCT_MEM_HOST) HIP_TRY(c, hipStreamSynchronize(s));      // the caller's memory is free again
    return VCT_OK;
}

int vct_planes_download(vct_ctx* c, const void* tiled, void* out, int nplanes, size_t elem) {
    hipStream_t s = cur(c).stream.get();
    const size_t npix = (size_t)c->cfg.width * c->cfg.height;
    PIPE_TRY(vct_staging_free(c));
    HIP_TRY(c, c->gb_linear.reserve(npix * VCT_GB_NPLANES));
    HIP_TRY(c, vct_launch_untile_planes(tiled, c->gb_linear.get(), nplanes, elem, c->cfg.width, c->cfg.height, s));
    HIP_TRY(c, hipMemcpyAsync(out, c->gb_linear.get(), npix * nplanes * elem, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return VCT_OK;
}
