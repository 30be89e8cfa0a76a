// ctx.h — MiCtx, the per-stream device context behind include/mi_av1dsp.h (one per decoder
// frame context; calls on one context are serialised by the caller and use one stream).
#pragma once
#include "common.h"

#include <cstring>
#include <vector>

// The device scratch of a resized output (mi_display_tensor, mi_display_scaled): the tap tables of
// a list of axes, then the horizontal pass's result, in one allocation that is replaced only when
// a call needs more. The tables depend on the list alone, and so does where they lie: a call with
// the list of the one before it on this context (every picture of a stream, as a rule) reuses
// them, ordered behind their launch on the context's stream.
struct MiResizeScratch {
    uint8_t *p = nullptr;
    size_t bytes = 0;
    // the axis count, the filter and the bits of its b and c, then n_in, n_out, phase per axis of
    // the tables held (all 0: none): another filter on the same geometry has other tables, and
    // other capacities too
    static constexpr int kKeyHead = 4;
    int key[kKeyHead + 3 * mi::kTapAxes] = {0};
    // Before any launch of the call: at least `need` bytes, or false with nothing held. Growing
    // loses the tables.
    bool ensure(size_t need) {
        if (need <= bytes) return true;
        if (p) (void)hipFree(p);   // (waits for the work that reads it)
        p = nullptr;
        bytes = 0;
        forget();
        if (hipMalloc(&p, need) != hipSuccess) return false;
        bytes = need;
        return true;
    }
    bool holds(const mi::TapList &t) const {
        int k[kKeyHead + 3 * mi::kTapAxes];
        fill(t, k);
        return memcmp(k, key, sizeof(key)) == 0;
    }
    // before the launches that write or read the tables, and after all of them were enqueued
    // without error: a call that fails in between leaves no tables to reuse
    void forget() { memset(key, 0, sizeof(key)); }
    void keep(const mi::TapList &t) { fill(t, key); }

  private:
    static void fill(const mi::TapList &t, int *k) {
        memset(k, 0, sizeof(key));
        k[0] = t.n;
        k[1] = t.filter;
        memcpy(k + 2, &t.b, sizeof(float));
        memcpy(k + 3, &t.c, sizeof(float));
        for (int a = 0; a < t.n; a++) {
            int *q = k + kKeyHead + 3 * a;
            q[0] = t.ax[a].n_in, q[1] = t.ax[a].n_out, q[2] = t.ax[a].phase;
        }
    }
};

struct MiCtx {
    int device = 0;
    int last_error = 0;
    // film-grain scratch (grain templates, scaling LUTs, block offsets)
    int16_t *fg_lut = nullptr;
    uint8_t *fg_scaling = nullptr;
    uint8_t *fg_offsets = nullptr;
    size_t fg_offsets_bytes = 0;
    // mi_display_picture with grain: the grained picture the converter reads (one allocation in
    // the geometry of the shown picture, replaced only when a picture needs more)
    uint8_t *disp_fg = nullptr;
    size_t disp_fg_bytes = 0;
    // mi_display_scaled_tm: the tone-mapped picture Q the scaled passes read (planar, at dst_bpc;
    // one allocation of its own, replaced only when a call needs more)
    uint8_t *disp_q = nullptr;
    size_t disp_q_bytes = 0;
    // mi_display_tensor and mi_display_scaled: a scratch each, so that alternating calls of the
    // two keep their tables
    MiResizeScratch tens, scal;
    // mi_display_*_tm: the device tables (lut_out, then lut_in) of the key `tone_key` (*tm with
    // the peaks zeroed for sources that do not read them, pri, trc, source bpc), their matrix, and
    // two pinned staging buffers used in turn; `tone_ev[i]` marks when buffer i may be rewritten.
    // tone_prepare compares the key per table (lut_out: dst_trc, dst_bpc; lut_in: peaks, trc,
    // source bpc; m: the primaries) and rebuilds only the stale ones. HLG sources (accepted only
    // with `hlg` set: mi_ctx_enable_hlg): lut_gain behind lut_in with a key of its own (the bits
    // of dst_peak), and the luminance row `tone_yw`, built with m
    uint8_t *tone_dev = nullptr;
    uint8_t *tone_host[2] = {nullptr, nullptr};
    hipEvent_t tone_ev[2] = {nullptr, nullptr};
    bool tone_ev_pending[2] = {false, false};
    int tone_slot = 0;
    bool tone_valid = false;
    int32_t tone_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float tone_m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool hlg = false;
    bool tone_gain_valid = false;
    int32_t tone_gain_key = 0;
    float tone_yw[3] = {0, 0, 0};
    // persistent intra reconstruction: per-block done epochs, queue heads, error word
    uint32_t *ir_done = nullptr;
    size_t ir_done_n = 0;
    int *ir_words = nullptr;      // [0..63] queue heads, [64] error, [72..79] XCD worker ranks
    uint32_t ir_epoch = 0;        // never reset: done words and edge granules hold old epochs
    unsigned long long *ir_gran = nullptr;   // edge granules (ipred.hip GranCtx), zeroed when allocated
    size_t ir_gran_n = 0;
    unsigned long long *ir_tl = nullptr;     // MI_IR_TIMELINE stamps (diagnostics)
    size_t ir_tl_n = 0;
    // one-grid MC with in-launch hand-off (mi_mc_frame_sync): per-tile flags of SEG masks,
    // epoch (never reset: the flags hold old epochs), error word
    uint32_t *mc_flags = nullptr;
    size_t mc_flags_n = 0;
    uint32_t mc_epoch = 0;
    int *mc_err = nullptr;
    // deferred DC runs (mi_itx_frame_runs MI_ITX_DC_DEFER -> mi_deblock_frame_dc): the map
    // (zeroed when allocated and when its 16-bit tag wraps), its geometry and the pending tag
    uint32_t *dc_map = nullptr;
    size_t dc_map_n = 0;
    int dc_w = 0, dc_h = 0, dc_layout = -1;
    uint32_t dc_tag = 0, dc_pending = 0;
    // frame executor (frame_exec.cpp): device copy of one frame's descriptors, staged through
    // pinned host memory; `fx_ev` marks when the staging buffer may be rewritten
    uint8_t *fx_dev = nullptr, *fx_host = nullptr;
    size_t fx_dev_bytes = 0, fx_host_bytes = 0;
    hipEvent_t fx_ev = nullptr;
    bool fx_ev_pending = false;
    // per-stage timing of mi_frame_run (mi_ctx_set_timing): 5 events per frame (before the
    // upload, after it, after inter prediction + residuals, after intra, at the end)
    bool tm_on = false;
    std::vector<hipEvent_t> tm_ev;
    double tm_host_ms = 0, tm_stage_ms = 0, tm_strips_ms = 0;
    int64_t tm_bytes = 0;
    int tm_frames = 0;
    void tm_clear() {
        for (hipEvent_t e : tm_ev) (void)hipEventDestroy(e);
        tm_ev.clear();
        tm_host_ms = tm_stage_ms = tm_strips_ms = 0;
        tm_bytes = 0;
        tm_frames = 0;
    }
    ~MiCtx() {
        tm_clear();
        if (fx_ev) (void)hipEventDestroy(fx_ev);
        if (fx_dev) (void)hipFree(fx_dev);
        if (fx_host) (void)hipHostFree(fx_host);
        if (ir_done) (void)hipFree(ir_done);
        if (mc_flags) (void)hipFree(mc_flags);
        if (mc_err) (void)hipFree(mc_err);
        if (dc_map) (void)hipFree(dc_map);
        if (ir_words) (void)hipFree(ir_words);
        if (ir_gran) (void)hipFree(ir_gran);
        if (ir_tl) (void)hipFree(ir_tl);
        if (fg_lut) (void)hipFree(fg_lut);
        if (fg_scaling) (void)hipFree(fg_scaling);
        if (fg_offsets) (void)hipFree(fg_offsets);
        if (disp_fg) (void)hipFree(disp_fg);
        if (disp_q) (void)hipFree(disp_q);
        if (tens.p) (void)hipFree(tens.p);
        if (scal.p) (void)hipFree(scal.p);
        if (tone_dev) (void)hipFree(tone_dev);
        for (int i = 0; i < 2; i++) {
            if (tone_ev[i]) (void)hipEventDestroy(tone_ev[i]);
            if (tone_host[i]) (void)hipHostFree(tone_host[i]);
        }
    }
};

struct MiIntraFrame;
namespace mi_internal {
// mi_intra_recon over frames, or (nstrips > 1, one frame) over the frame's strips: queue q =
// blocks [strip_start[q], strip_start[q + 1]) on XCD q (capi.cpp)
// granules: edges handed over as data-tagged granules (ipred.hip); then deps need list only the
// blocks whose pixels are read beyond the edges (CfL luma, intra block copy sources)
int intra_recon(MiCtx *ctx, const MiIntraFrame *frames, int nframes, const int32_t *strip_start, int nstrips,
                unsigned flags, void *stream, bool granules = false);
// What the film-grain entries of capi.cpp and dsp_calls.cpp share (capi.cpp): the kernels'
// constant tables, uploaded once per process (0 or -EIO), and the parameter ranges they index with
int fg_tables();
bool fg_data_ok(const MiFilmGrainData *data);
}
