// vct_api_import.hip -- the C ABI of the G-buffer import (include/vct.h "G-buffer import"): a renderer's depth, normal
// and colour buffers into the selected frame slot's resident tiled G-buffer.
#include "vct_ctx.h"
#include "vct_import_check.h"

static const char* import_verdict_text(int verdict) {
    switch (verdict) {
        case VCT_IMPORT_BAD_NULL: return "null descriptor, or a null position, normal or albedo buffer";
        case VCT_IMPORT_BAD_FORMAT: return "unknown position, normal, albedo or specular format";
        case VCT_IMPORT_BAD_LOCATION: return "unknown location";
        case VCT_IMPORT_BAD_FLAGS: return "unknown flag bit";
        case VCT_IMPORT_BAD_MATRIX: return "inv_view_proj has a non-finite element";
        case VCT_IMPORT_BAD_NORMAL_SCALE: return "normal_scale must be finite and > 0";
        case VCT_IMPORT_BAD_SPECULAR_CONSTANT: return "specular_constant has a non-finite element (and there is no specular buffer)";
        default: return "tile-row range outside the frame";
    }
}

// The inputs of a host-located import on the device: rows [in_row0, in_row1) of every buffer the descriptor names are
// copied to their place in the slot's staging (the rest of it is not read), and `dev` gets the descriptor with the
// staged pointers.  On the slot's stream.
static int stage_inputs(vct_ctx* c, VctFrameSlot& s, const vct_gbuffer_import& in, int in_row0, int in_row1, vct_gbuffer_import& dev) {
    const int32_t w = c->cfg.width, h = c->cfg.height;
    const void* src[7] = {in.position, in.normal, in.shading_normal, in.albedo, in.specular, in.shadow, in.material};
    const size_t elem[7] = {vct_import_position_bytes(in.position_format), vct_import_normal_bytes(in.normal_format),
                            vct_import_normal_bytes(in.normal_format), vct_import_color_bytes(in.albedo_format),
                            vct_import_color_bytes(in.specular_format), sizeof(float), sizeof(uint16_t)};
    size_t off[7], total = 0;
    for (int k = 0; k < 7; ++k) {
        off[k] = total;
        if (src[k]) total += (vct_import_buffer_bytes(elem[k], w, h) + 255) & ~(size_t)255;
    }
    HIP_TRY(c, s.gb_import.stage.reserve(total));
    const void* staged[7];
    for (int k = 0; k < 7; ++k) {
        staged[k] = src[k] ? s.gb_import.stage.get() + off[k] : nullptr;
        if (!src[k] || in_row1 <= in_row0) continue;
        const size_t first = vct_import_buffer_bytes(elem[k], w, in_row0), bytes = vct_import_buffer_bytes(elem[k], w, in_row1 - in_row0);
        HIP_TRY(c, hipMemcpyAsync(s.gb_import.stage.get() + off[k] + first, (const char*)src[k] + first, bytes, hipMemcpyHostToDevice,
                                  s.stream.get()));
    }
    dev = in;
    dev.position = staged[0]; dev.normal = staged[1]; dev.shading_normal = staged[2]; dev.albedo = staged[3];
    dev.specular = staged[4]; dev.shadow = (const float*)staged[5]; dev.material = (const uint16_t*)staged[6];
    return VCT_OK;
}

extern "C" {

int vct_import_gbuffer_rows(vct_ctx* c, const vct_gbuffer_import* in, int32_t row0, int32_t row1) {
    if (!c) return VCT_ERR_INVALID;
    const int verdict = vct_import_check_desc(in, vct_tiles_y(c), row0, row1);
    if (verdict != VCT_IMPORT_OK) return vct_fail(c, VCT_ERR_INVALID, std::string("vct_import_gbuffer: ") + import_verdict_text(verdict));
    HIP_TRY(c, hipSetDevice(c->device));
    VctFrameSlot& s = cur(c);
    const bool host = in->location == VCT_MEM_HOST;
    vct_gbuffer_import dev = *in;
    if (host) {
        // the input rows that hold pixel rows [8 row0, min(8 row1, h))
        const int h = c->cfg.height;
        const int y0 = row0 * VCT_TILE, y1 = row1 * VCT_TILE < h ? row1 * VCT_TILE : h;
        const bool flip = (in->flags & VCT_IMPORT_FLIP_Y) != 0;
        PIPE_TRY(stage_inputs(c, s, *in, flip ? h - y1 : y0, flip ? h - y0 : y1, dev));
    }
    VctImportArgs a;
    memset(&a, 0, sizeof(a));
    a.desc = &dev;
    a.W = c->cfg.width; a.H = c->cfg.height; a.row0 = row0; a.row1 = row1;
    a.shadow = c->shadow.words.get(); a.shadow_ebase = c->shadow.ebase; a.shadow_size = c->shadow.size;
    a.shadow_tiles = c->shadow.tiles.get(); a.light_vp = c->shadow.light_vp;
    a.tiled = s.gb_tiled.get();
    a.nmat = c->mesh.nmat;
    if (in->material && c->mesh.mat_emission) {
        HIP_TRY(c, vct_emission_planes(c, s));
        a.emission = c->mesh.mat_emission.get(); a.emis_tiled = s.emis.get();
    }
    if (in->material && c->gloss.n && c->mesh.mat_gloss) {
        HIP_TRY(c, vct_gloss_plane(c, s));
        a.mat_gloss = c->mesh.mat_gloss.get(); a.gloss_tiled = s.gloss.get();
    }
    HIP_TRY(c, s.gb_import.timer.begin(s.stream.get(), c->time_traces));
    HIP_TRY(c, vct_launch_gbuffer_import(a, s.stream.get()));
    HIP_TRY(c, s.gb_import.timer.end(s.stream.get()));
    // the slot's own buffer is the resident G-buffer from here on, also after a zero-copy vct_trace of a caller's
    s.gb_current = s.gb_tiled.get();
    s.last_row0 = row0;
    s.last_row1 = row1;
    s.last_row_stride = 1;
    s.have_gbuffer = true;
    if (host) HIP_TRY(c, hipStreamSynchronize(s.stream.get()));      // the planes are written, the caller's memory is free again
    return VCT_OK;
}

int vct_import_gbuffer(vct_ctx* c, const vct_gbuffer_import* in) {
    if (!c) return VCT_ERR_INVALID;
    return vct_import_gbuffer_rows(c, in, 0, vct_tiles_y(c));
}

int vct_last_gbuffer_import_ms(vct_ctx* c, float* ms) {
    if (!c || !ms) return VCT_ERR_INVALID;
    return vct_timer_ms(c, cur(c).gb_import.timer, ms, "vct_last_gbuffer_import_ms: no G-buffer import has run on this frame slot",
                        "vct_last_gbuffer_import_ms: the last import was issued with timing off (vct_set_trace_timing)");
}

}  // extern "C"
