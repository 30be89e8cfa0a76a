// capi.cpp — the C-ABI of include/mi_av1dsp.h: contexts and the batched per-frame entry points
// (mi_itx_frame*, mi_mc_*, mi_ipred_blocks / mi_intra_*, mi_deblock_*, mi_cdef_*, mi_lr_*,
// mi_film_grain_*), and mi_internal::intra_recon. The table-compatible per-call entry points
// (mi_dsp_*) are in dsp_calls.cpp.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <errno.h>
#include <mutex>
#include <string.h>
#include <string>
#include <vector>
#include "common.h"
#include "ctx.h"


namespace {

int fail(MiCtx *c, int e) {
    if (c) c->last_error = e;
    return e;
}

// The context's device words ([0..63] queue heads, [64] dependency-wait give-up / untaken
// blocks, [65] rejected descriptors, [72..79] XCD worker ranks), allocated zeroed on first use.
// Zeroed on the context's own stream: a null-stream hipMemset is not ordered with a
// non-blocking stream and may land after (or during) the first kernel that uses the words --
// with two contexts whose streams overlap, it reset the queue heads of a running persistent
// intra launch, which then re-ran blocks whose coefficients it had already consumed.
int ctx_words(MiCtx *c, hipStream_t s) {
    if (c->ir_words) return 0;
    if (hipMalloc(&c->ir_words, 128 * sizeof(int)) != hipSuccess) return -ENOMEM;
    if (hipMemsetAsync(c->ir_words, 0, 128 * sizeof(int), s) != hipSuccess) return -EIO;
    return 0;
}

bool same_geometry(const MiPicture *a, const MiPicture *b) {
    return a->bpc == b->bpc && a->w == b->w && a->h == b->h && a->layout == b->layout &&
           a->stride[0] == b->stride[0] && a->stride[1] == b->stride[1];
}

} // namespace

extern "C" {

const char *mi_version(void) { return "rav1d_amd mi_av1dsp 0.1 (gfx950)"; }

int mi_ctx_create(int device, MiCtx **out) {
    if (!out) return -EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return -ENODEV;
    MiCtx *c = new (std::nothrow) MiCtx;
    if (!c) return -ENOMEM;
    c->device = device;
    *out = c;
    return 0;
}

void mi_ctx_destroy(MiCtx *ctx) { delete ctx; }

int mi_ctx_last_error(const MiCtx *ctx) { return ctx ? ctx->last_error : -EINVAL; }

static int itx_frame(MiCtx *ctx, const MiPicture *pic, const MiTxBlock *blocks,
                     const uint32_t *size_start, const uint32_t *band_start, void *coef, unsigned flags,
                     void *stream, const uint32_t *dc_end = nullptr);

int mi_itx_frame(MiCtx *ctx, const MiPicture *pic, const MiTxBlock *blocks,
                 const uint32_t size_start[MI_N_RECT_TX_SIZES + 1], void *coef, unsigned flags,
                 void *stream) {
    return itx_frame(ctx, pic, blocks, size_start, nullptr, coef, flags, stream);
}

int mi_itx_frame_banded(MiCtx *ctx, const MiPicture *pic, const MiTxBlock *blocks,
                        const uint32_t band_start[MI_N_RECT_TX_SIZES][MI_ITX_BANDS + 1], void *coef,
                        unsigned flags, void *stream) {
    if (!band_start) return fail(ctx, -EINVAL);
    // bands of one size are consecutive ranges and the sizes follow each other
    uint32_t ss[MI_N_RECT_TX_SIZES + 1];
    for (int t = 0; t < MI_N_RECT_TX_SIZES; t++) {
        ss[t] = band_start[t][0];
        if (t && band_start[t][0] != band_start[t - 1][MI_ITX_BANDS]) return fail(ctx, -EINVAL);
        for (int q = 0; q < MI_ITX_BANDS; q++)
            if (band_start[t][q + 1] < band_start[t][q]) return fail(ctx, -EINVAL);
    }
    ss[MI_N_RECT_TX_SIZES] = band_start[MI_N_RECT_TX_SIZES - 1][MI_ITX_BANDS];
    return itx_frame(ctx, pic, blocks, ss, &band_start[0][0], coef, flags, stream);
}

int mi_itx_frame_runs(MiCtx *ctx, const MiPicture *pic, const MiTxBlock *blocks,
                      const uint32_t band_start[MI_N_RECT_TX_SIZES][MI_ITX_BANDS + 1],
                      const uint32_t dc_end[MI_N_RECT_TX_SIZES][MI_ITX_BANDS], void *coef, unsigned flags,
                      void *stream) {
    if (!band_start || !dc_end) return fail(ctx, -EINVAL);
    uint32_t ss[MI_N_RECT_TX_SIZES + 1];
    for (int t = 0; t < MI_N_RECT_TX_SIZES; t++) {
        ss[t] = band_start[t][0];
        if (t && band_start[t][0] != band_start[t - 1][MI_ITX_BANDS]) return fail(ctx, -EINVAL);
        for (int q = 0; q < MI_ITX_BANDS; q++)
            if (band_start[t][q + 1] < band_start[t][q] || dc_end[t][q] < band_start[t][q] ||
                dc_end[t][q] > band_start[t][q + 1])
                return fail(ctx, -EINVAL);
    }
    ss[MI_N_RECT_TX_SIZES] = band_start[MI_N_RECT_TX_SIZES - 1][MI_ITX_BANDS];
    return itx_frame(ctx, pic, blocks, ss, &band_start[0][0], coef, flags, stream, &dc_end[0][0]);
}

static int itx_frame(MiCtx *ctx, const MiPicture *pic, const MiTxBlock *blocks,
                     const uint32_t *size_start, const uint32_t *band_start, void *coef, unsigned flags,
                     void *stream, const uint32_t *dc_end) {
    if (!ctx || !pic || !size_start) return fail(ctx, -EINVAL);
    // any itx frame call supersedes a deferral still pending: its DC runs belong to pixels this
    // call rewrites (only a deferring launch below sets a new one)
    ctx->dc_pending = 0;
    if (pic->bpc != 8 && pic->bpc != 10 && pic->bpc != 12) return fail(ctx, -EINVAL);
    mi::ItxArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < 3; p++) {
        a.plane[p] = (uint8_t *)pic->data[p];
        a.stride[p] = pic->stride[p ? 1 : 0];
    }
    a.blocks = blocks;
    a.coef = (uint8_t *)coef;
    a.bdmax = (1 << pic->bpc) - 1;
    a.zero_coefs = (flags & MI_ITX_KEEP_COEFS) ? 0 : 1;
    if (flags & ~(MI_ITX_KEEP_COEFS | MI_ITX_DC_DEFER)) return fail(ctx, -EINVAL);
    if ((flags & MI_ITX_DC_DEFER) && !dc_end) return fail(ctx, -EINVAL);
    {
        const int sh = pic->layout == 1 || pic->layout == 2, sv = pic->layout == 1;
        const int aw = (pic->w + 127) & ~127, ah = (pic->h + 127) & ~127;
        for (int p = 0; p < (pic->layout ? 3 : 1); p++) {
            a.pw[p] = p ? aw >> sh : aw;
            a.ph[p] = p ? ah >> sv : ah;
        }
    }
    if (int e = ctx_words(ctx, (hipStream_t)stream)) return fail(ctx, e);
    a.err = ctx->ir_words + 65;
    for (int k = 0; k < MI_N_RECT_TX_SIZES; k++)
        if (size_start[k + 1] < size_start[k]) return fail(ctx, -EINVAL);
    const int wg = mi::itx_fill_schedule(a, size_start, band_start, dc_end);
    bool deferring = false;
    if (flags & MI_ITX_DC_DEFER) {
        // the DC runs go to the context's DC map for the next mi_deblock_frame_dc; under stream
        // capture they are added to the pixels as without the flag (a tag fixed in a graph would
        // let a replay match the map entries of the previous replay)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) return fail(ctx, -EIO);
        if (cap == hipStreamCaptureStatusNone) {
            const mi::DcMapGeom g = mi::dc_map_geom(pic->w, pic->h, pic->layout);
            if (g.entries > ctx->dc_map_n) {
                if (ctx->dc_map) (void)hipFree(ctx->dc_map);
                ctx->dc_map = nullptr;
                ctx->dc_map_n = 0;
                if (hipMalloc(&ctx->dc_map, g.entries * 4) != hipSuccess) return fail(ctx, -ENOMEM);
                if (hipMemsetAsync(ctx->dc_map, 0, g.entries * 4, (hipStream_t)stream) != hipSuccess) return fail(ctx, -EIO);
                ctx->dc_map_n = g.entries;
                ctx->dc_tag = 0;
            }
            if (++ctx->dc_tag > 0xffffu) {   // the 16-bit tag wraps: no stale entry may match
                if (hipMemsetAsync(ctx->dc_map, 0, ctx->dc_map_n * 4, (hipStream_t)stream) != hipSuccess) return fail(ctx, -EIO);
                ctx->dc_tag = 1;
            }
            a.dc_map = ctx->dc_map;
            for (int p = 0; p < 3; p++) {
                a.dc_off[p] = g.off[p];
                a.dc_stride[p] = g.stride[p];
            }
            a.dc_tag = ctx->dc_tag;
            deferring = true;
        }
    }
    // (an empty or refused call defers nothing: no tag is left pending for it)
    if (wg == 0) return 0;
    if (!blocks || !coef) return fail(ctx, -EINVAL);
    // One launch (itx.hip): the large sizes' workgroups first, the small ones fill in around
    // them. A side stream for the large sizes (event fork/join) measured slower (4K10 itx
    // 56 -> 74 us) than the cross-queue dependency saves.
    hipStream_t s = (hipStream_t)stream;
    const int r = mi::launch_itx_frame(a, wg, pic->bpc, s);
    if (r) return fail(ctx, -EIO);
    if (deferring) {   // the launch is enqueued: the next mi_deblock_frame_dc owes its DC runs
        ctx->dc_pending = ctx->dc_tag;
        ctx->dc_w = pic->w;
        ctx->dc_h = pic->h;
        ctx->dc_layout = pic->layout;
    }
    return 0;
}

}  // extern "C"

namespace {
// McArgs from the current picture and the references (planes, strides, clamp bounds, bit
// depth). same_size: the references must share cur's geometry (non-scaled MC, warp).
int fill_mc_args(mi::McArgs &a, const MiPicture *cur, const MiPicture *refs, int nrefs, bool same_size) {
    memset(&a, 0, sizeof(a));
    if (cur->bpc != 8 && cur->bpc != 10 && cur->bpc != 12) return -EINVAL;
    if (nrefs < 0 || nrefs > 7 || (nrefs && !refs)) return -EINVAL;
    const int ss_hor = cur->layout == 1 || cur->layout == 2, ss_ver = cur->layout == 1;
    for (int p = 0; p < 3; p++) a.dst[p] = (uint8_t *)cur->data[p];
    a.dst_stride[0] = cur->stride[0];
    a.dst_stride[1] = cur->stride[1];
    for (int r = 0; r < nrefs; r++) {
        if (same_size ? !same_geometry(cur, &refs[r])
                      : refs[r].bpc != cur->bpc || refs[r].layout != cur->layout || refs[r].w <= 0 || refs[r].h <= 0)
            return -EINVAL;
        for (int p = 0; p < 3; p++) {
            const int sh = p ? ss_hor : 0, sv = p ? ss_ver : 0;
            a.ref[r][p] = (const uint8_t *)refs[r].data[p];
            a.ref_w[r][p] = (refs[r].w + sh) >> sh;
            a.ref_h[r][p] = (refs[r].h + sv) >> sv;
        }
        a.ref_stride[r][0] = refs[r].stride[0];
        a.ref_stride[r][1] = refs[r].stride[1];
        // mc_kernel forms reference row offsets with 24-bit multiplies
        for (int k = 0; k < 2; k++)
            if (refs[r].stride[k] <= 0 || refs[r].stride[k] >= (1 << 24)) return -EINVAL;
    }
    a.nrefs = nrefs;
    a.bpc = cur->bpc;
    a.ib = cur->bpc == 8 ? 4 : 14 - cur->bpc;
    a.bias = cur->bpc == 8 ? 0 : 8192;
    a.bdmax = (1 << cur->bpc) - 1;
    a.layout = cur->layout;
    a.seg_ss_hor = cur->layout ? ss_hor : 0;   // w_mask[chr_layout_idx] (recon_tmpl.c:1868)
    a.seg_ss_ver = cur->layout ? ss_ver : 0;
    return 0;
}
}  // namespace

namespace mi_internal {
int fg_tables() {
    static std::once_flag once;
    static int tables_rc = 0;
    std::call_once(once, [] { tables_rc = mi::init_fg_tables(); });
    return tables_rc ? -EIO : 0;
}
bool fg_data_ok(const MiFilmGrainData *data) {
    return !(data->num_y_points < 0 || data->num_y_points > 14 || data->ar_coeff_lag < 0 || data->ar_coeff_lag > 3 ||
             data->num_uv_points[0] < 0 || data->num_uv_points[0] > 10 || data->num_uv_points[1] < 0 ||
             data->num_uv_points[1] > 10 || data->ar_coeff_shift < 6 || data->ar_coeff_shift > 9);
}
}  // namespace mi_internal
using mi_internal::fg_data_ok;
using mi_internal::fg_tables;

extern "C" {

int mi_mc_frame(MiCtx *ctx, const MiPicture *cur, const MiPicture *refs, int nrefs,
                const MiMcBlock *blocks, const uint32_t class_start[2 * MI_MC_NCLASS + 1], uint8_t *masks,
                int16_t *tmp, void *stream) {
    return mi_mc_frame_ex(ctx, cur, refs, nrefs, blocks, class_start, masks, tmp, 0, stream);
}

int mi_mc_frame_ex(MiCtx *ctx, const MiPicture *cur, const MiPicture *refs, int nrefs,
                   const MiMcBlock *blocks, const uint32_t class_start[2 * MI_MC_NCLASS + 1], uint8_t *masks,
                   int16_t *tmp, unsigned flags, void *stream) {
    if (!ctx || !cur || !class_start || (flags & ~MI_MC_ONE_GRID)) return fail(ctx, -EINVAL);
    for (int k = 0; k < 2 * MI_MC_NCLASS; k++)
        if (class_start[k] > class_start[k + 1]) return fail(ctx, -EINVAL);
    mi::McArgs a;
    // scaled references take mi_mc_scaled (the reference's mc_scaled path)
    if (int e = fill_mc_args(a, cur, refs, nrefs, true)) return fail(ctx, e);
    if (class_start[2 * MI_MC_NCLASS] == class_start[0]) return 0;
    if (!blocks || !nrefs) return fail(ctx, -EINVAL);
    a.blocks = blocks;
    a.masks = masks;
    a.tmp = tmp;
    memcpy(a.class_start, class_start, sizeof(a.class_start));
    const int w0 = mi::mc_plan(a, 0), w1 = mi::mc_plan(a, 1);
    if (w0 < 0 || w1 < 0) return fail(ctx, -EINVAL);
    hipStream_t s = (hipStream_t)stream;
    // luma first: chroma units of SEG blocks read the mask their luma unit writes (one grid
    // only when the caller says no chroma unit of this call does)
    int r;
    if ((flags & MI_MC_ONE_GRID) && w0 && w1) {
        r = mi::launch_mc(a, 2, w0 + w1, s);
    } else {
        r = mi::launch_mc(a, 0, w0, s);
        if (!r) r = mi::launch_mc(a, 1, w1, s);
    }
    return r ? fail(ctx, -EIO) : 0;
}

// The device error word of the MC hand-off: bit 1 a unit's mask offset lies past the flag
// buffer (mask_bytes too small for it: -EINVAL), bit 0 a wait gave up (-ETIMEDOUT). Both
// status entry points report the same code.
static int mc_err_code(int e) { return (e & 2) ? -EINVAL : -ETIMEDOUT; }

int mi_mc_frame_sync(MiCtx *ctx, const MiPicture *cur, const MiPicture *refs, int nrefs,
                     const MiMcBlock *blocks, const uint32_t class_start[2 * MI_MC_NCLASS + 1], uint8_t *masks,
                     size_t mask_bytes, int16_t *tmp, void *stream) {
    if (!ctx || !cur || !class_start) return fail(ctx, -EINVAL);
    for (int k = 0; k < 2 * MI_MC_NCLASS; k++)
        if (class_start[k] > class_start[k + 1]) return fail(ctx, -EINVAL);
    mi::McArgs a;
    if (int e = fill_mc_args(a, cur, refs, nrefs, true)) return fail(ctx, e);
    if (class_start[2 * MI_MC_NCLASS] == class_start[0]) return 0;
    if (!blocks || !nrefs || (mask_bytes && !masks)) return fail(ctx, -EINVAL);
    a.blocks = blocks;
    a.masks = masks;
    a.tmp = tmp;
    memcpy(a.class_start, class_start, sizeof(a.class_start));
    const int w0 = mi::mc_plan(a, 0), w1 = mi::mc_plan(a, 1);
    if (w0 < 0 || w1 < 0) return fail(ctx, -EINVAL);
    hipStream_t s = (hipStream_t)stream;
    // Under stream capture the epoch below would be frozen into the graph: a replay would find
    // the flags of its previous replay already at "its" epoch and read masks that are still
    // being rewritten. Captured calls therefore take the two launches of mi_mc_frame (luma,
    // then chroma; no flags), which any number of replays orders correctly.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) return fail(ctx, -EIO);
    if (cap != hipStreamCaptureStatusNone) {
        int r = w0 ? mi::launch_mc(a, 0, w0, s) : 0;
        if (!r && w1) r = mi::launch_mc(a, 1, w1, s);
        return r ? fail(ctx, -EIO) : 0;
    }
    // the tile flags: 32 per 16 mask bytes (a SEG unit has at most 32 tiles), zeroed when
    // allocated and never reset (each call has its own epoch)
    const size_t nf = (mask_bytes / 16 + 1) * 32;
    if (nf > 0xffffffffu) return fail(ctx, -EINVAL);
    if (nf > ctx->mc_flags_n) {
        if (ctx->mc_flags) (void)hipFree(ctx->mc_flags);
        ctx->mc_flags = nullptr;
        ctx->mc_flags_n = 0;
        if (hipMalloc(&ctx->mc_flags, nf * sizeof(uint32_t)) != hipSuccess) return fail(ctx, -ENOMEM);
        if (hipMemsetAsync(ctx->mc_flags, 0, nf * sizeof(uint32_t), s) != hipSuccess) return fail(ctx, -EIO);
        ctx->mc_flags_n = nf;
    }
    if (!ctx->mc_err) {
        if (hipMalloc(&ctx->mc_err, sizeof(int)) != hipSuccess) return fail(ctx, -ENOMEM);
        if (hipMemsetAsync(ctx->mc_err, 0, sizeof(int), s) != hipSuccess) return fail(ctx, -EIO);
    }
    if (++ctx->mc_epoch == 0) ctx->mc_epoch = 1;
    a.seg_flags = ctx->mc_flags;
    a.seg_epoch = ctx->mc_epoch;
    a.seg_nflags = (uint32_t)nf;
    a.err = ctx->mc_err;
    // one grid, the luma group's waves first (see mi_av1dsp.h)
    const int r = w0 && w1 ? mi::launch_mc(a, 2, w0 + w1, s) : mi::launch_mc(a, w0 ? 0 : 1, w0 ? w0 : w1, s);
    return r ? fail(ctx, -EIO) : 0;
}

int mi_mc_sync_status(MiCtx *ctx, void *stream) {
    if (!ctx) return -EINVAL;
    if (!ctx->mc_err) return 0;
    int e = 0;
    if (hipMemcpyAsync(&e, ctx->mc_err, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return fail(ctx, -EIO);
    if (e && hipMemsetAsync(ctx->mc_err, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) return fail(ctx, -EIO);
    return e ? fail(ctx, mc_err_code(e)) : 0;
}

int mi_mc_scaled(MiCtx *ctx, const MiPicture *cur, const MiPicture *refs, int nrefs,
                 const MiMcBlock *blocks, int n, int16_t *tmp, void *stream) {
    if (!ctx || !cur || n < 0) return fail(ctx, -EINVAL);
    mi::McArgs a;
    if (int e = fill_mc_args(a, cur, refs, nrefs, false)) return fail(ctx, e);
    if (!n) return 0;
    if (!blocks || !nrefs) return fail(ctx, -EINVAL);
    a.tmp = tmp;
    return mi::launch_mc_scaled(a, blocks, n, cur->w, cur->h, (hipStream_t)stream) ? fail(ctx, -EIO) : 0;
}

int mi_mc_warp(MiCtx *ctx, const MiPicture *cur, const MiPicture *refs, int nrefs,
               const MiWarpBlock *blocks, int n, int16_t *tmp, void *stream) {
    if (!ctx || !cur || n < 0) return fail(ctx, -EINVAL);
    mi::McArgs a;
    if (int e = fill_mc_args(a, cur, refs, nrefs, true)) return fail(ctx, e);
    if (!n) return 0;
    if (!blocks || !nrefs) return fail(ctx, -EINVAL);
    a.tmp = tmp;
    return mi::launch_mc_warp(a, blocks, n, (hipStream_t)stream) ? fail(ctx, -EIO) : 0;
}

int mi_mc_combine(MiCtx *ctx, const MiPicture *cur, const MiMcCombine *units, int n,
                  const int16_t *tmp, uint8_t *masks, void *stream) {
    if (!ctx || !cur || n < 0) return fail(ctx, -EINVAL);
    mi::McArgs a;
    if (int e = fill_mc_args(a, cur, nullptr, 0, true)) return fail(ctx, e);
    if (!n) return 0;
    if (!units || !tmp) return fail(ctx, -EINVAL);
    a.tmp = const_cast<int16_t *>(tmp);
    a.masks = masks;
    return mi::launch_mc_combine(a, units, n, (hipStream_t)stream) ? fail(ctx, -EIO) : 0;
}

int mi_superres_frame(MiCtx *ctx, const MiPicture *src, const MiPicture *dst, void *stream) {
    if (!ctx || !src || !dst) return fail(ctx, -EINVAL);
    if (src->bpc != dst->bpc || src->layout != dst->layout || src->h != dst->h || src->w <= 0 ||
        dst->w < src->w || dst->w > 2 * src->w + 16 || (src->bpc != 8 && src->bpc != 10 && src->bpc != 12))
        return fail(ctx, -EINVAL);
    // scale_fac / get_upscale_x0 (decode.rs:4644-4648, 4776-4778, 4872-4878)
    auto scale_fac = [](int ref_sz, int this_sz) { return ((ref_sz << 14) + (this_sz >> 1)) / this_sz; };
    auto upscale_x0 = [](int in_w, int out_w, int step) {
        const int err = out_w * step - (in_w << 14);
        const int x0 = (-((out_w - in_w) << 13) + (out_w >> 1)) / out_w + 128 - err / 2;
        return x0 & 0x3fff;
    };
    mi::SuperresArgs a;
    memset(&a, 0, sizeof(a));
    const int ss_hor = src->layout == 1 || src->layout == 2, ss_ver = src->layout == 1;
    const int in_cw = (src->w + ss_hor) >> ss_hor, out_cw = (dst->w + ss_hor) >> ss_hor;
    a.step[0] = scale_fac(src->w, dst->w);
    a.step[1] = scale_fac(in_cw, out_cw);
    a.start[0] = upscale_x0(src->w, dst->w, a.step[0]);
    a.start[1] = upscale_x0(in_cw, out_cw, a.step[1]);
    const int bw4 = ((src->w + 7) >> 3) << 1;   // f->bw
    a.nplanes = src->layout ? 3 : 1;
    for (int p = 0; p < a.nplanes; p++) {
        const int sh = p ? ss_hor : 0, sv = p ? ss_ver : 0;
        a.src[p] = (const uint8_t *)src->data[p];
        a.dst[p] = (uint8_t *)dst->data[p];
        a.src_w[p] = (4 * bw4 + sh) >> sh;
        a.dst_w[p] = (dst->w + sh) >> sh;
        a.h[p] = (src->h + sv) >> sv;
        a.chunks = std::max(a.chunks, (a.dst_w[p] + 255) / 256);
    }
    a.src_stride[0] = src->stride[0];
    a.src_stride[1] = src->stride[1];
    a.dst_stride[0] = dst->stride[0];
    a.dst_stride[1] = dst->stride[1];
    a.bpc = src->bpc;
    return mi::launch_superres(a, (hipStream_t)stream) ? fail(ctx, -EIO) : 0;
}

int mi_ipred_blocks(MiCtx *ctx, const MiPicture *pic, const MiIpredBlock *blocks, int n,
                    const void *edges, const int16_t *ac, const uint8_t *idx, void *stream) {
    if (!ctx || !pic || n < 0) return fail(ctx, -EINVAL);
    if (pic->bpc != 8 && pic->bpc != 10 && pic->bpc != 12) return fail(ctx, -EINVAL);
    if (!n) return 0;
    if (!blocks || !edges) return fail(ctx, -EINVAL);
    mi::IpredArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < 3; p++) a.dst[p] = (uint8_t *)pic->data[p];
    a.stride[0] = pic->stride[0];
    a.stride[1] = pic->stride[1];
    a.blocks = blocks;
    a.edges = (const uint8_t *)edges;
    a.ac = ac;
    a.idx = idx;
    a.bpc = pic->bpc;
    a.bdmax = (1 << pic->bpc) - 1;
    return mi::launch_ipred(a, n, (hipStream_t)stream) ? fail(ctx, -EIO) : 0;
}

int mi_intra_blocks(MiCtx *ctx, const MiPicture *pic, const MiIntraBlock *blocks, int n,
                    const int16_t *ac, const uint8_t *idx, const void *pal, void *stream) {
    if (!ctx || !pic || n < 0) return fail(ctx, -EINVAL);
    if (pic->bpc != 8 && pic->bpc != 10 && pic->bpc != 12) return fail(ctx, -EINVAL);
    if (!n) return 0;
    if (!blocks) return fail(ctx, -EINVAL);
    mi::IpredArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < 3; p++) a.dst[p] = (uint8_t *)pic->data[p];
    a.stride[0] = pic->stride[0];
    a.stride[1] = pic->stride[1];
    a.iblocks = blocks;
    a.ac = ac;
    a.idx = idx;
    a.pal = (const uint8_t *)pal;
    a.bpc = pic->bpc;
    a.bdmax = (1 << pic->bpc) - 1;
    return mi::launch_intra(a, n, (hipStream_t)stream) ? fail(ctx, -EIO) : 0;
}

int mi_intra_recon(MiCtx *ctx, const MiIntraFrame *frames, int nframes, unsigned flags, void *stream) {
    return mi_internal::intra_recon(ctx, frames, nframes, nullptr, 1, flags, stream, (flags & MI_IR_EDGE_GRANULES) != 0);
}

int mi_ctx_device_status(MiCtx *ctx, void *stream) {
    if (!ctx) return -EINVAL;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(ctx, -EIO);
    if (ctx->mc_err) {   // a one-grid MC hand-off wait gave up (mi_mc_frame_sync)
        int e = 0;
        if (hipMemcpy(&e, ctx->mc_err, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, -EIO);
        if (e) {
            if (hipMemset(ctx->mc_err, 0, sizeof(int)) != hipSuccess) return fail(ctx, -EIO);
            return fail(ctx, mc_err_code(e));
        }
    }
    if (!ctx->ir_words) return 0;
    int w[66];
    if (hipMemcpy(w, ctx->ir_words, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, -EIO);
    if (w[65]) {   // a kernel rejected (skipped) descriptors
        if (hipMemsetAsync(ctx->ir_words + 65, 0, sizeof(int), (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
            return fail(ctx, -EIO);
        return fail(ctx, -EINVAL);
    }
    if (getenv("MI_DEBUG"))
        fprintf(stderr, "mi_ctx_device_status: heads %d %d %d %d %d %d %d %d err %d\n", w[0], w[1], w[2], w[3], w[4],
                w[5], w[6], w[7], w[64]);
    // [64]: bit 0 a dependency wait gave up, bit 2 a launch left blocks untaken (a frame
    // whose XCD received no workgroup): set on the device by every launch, sticky until read
    if (w[64]) {
        if (hipMemsetAsync(ctx->ir_words + 64, 0, sizeof(int), (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
            return fail(ctx, -EIO);
        return fail(ctx, (w[64] & 1) ? -ETIMEDOUT : -EIO);
    }
    return 0;
}

int mi_deblock_frame(MiCtx *ctx, const MiPicture *pic, const MiLoopFilter *lf, void *stream) {
    if (!ctx || !pic || !lf) return fail(ctx, -EINVAL);
    ctx->dc_pending = 0;   // a deferral still pending is dropped: only mi_deblock_frame_dc adds it
    if (pic->bpc != 8 && pic->bpc != 10 && pic->bpc != 12) return fail(ctx, -EINVAL);
    if (!lf->filter_y) return 0;   // deblocking off for the frame (recon.rs:4047-4060)
    if (!lf->level || !lf->masks || lf->sb128w <= 0) return fail(ctx, -EINVAL);
    mi::LfArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < 3; p++) {
        a.plane[p] = (uint8_t *)pic->data[p];
        a.stride[p] = pic->stride[p ? 1 : 0];
    }
    a.level = (const uint32_t *)lf->level;
    a.b4_stride = lf->b4_stride;
    a.masks = lf->masks;
    a.w4 = (pic->w + 3) >> 2;
    a.h4 = (pic->h + 3) >> 2;
    a.sb128w = lf->sb128w;
    a.sb128h = (pic->h + 127) >> 7;
    if (a.sb128w != (pic->w + 127) >> 7 || a.b4_stride < (int64_t)a.sb128w * 32) return fail(ctx, -EINVAL);
    a.ss_hor = pic->layout == 1 || pic->layout == 2;
    a.ss_ver = pic->layout == 1;
    a.bdmax = (1 << pic->bpc) - 1;
    a.bdm8 = pic->bpc - 8;
    a.filter_uv = pic->layout != 0 && lf->filter_uv;
    memcpy(a.lim_e, lf->lim_e, 64);
    memcpy(a.lim_i, lf->lim_i, 64);
    const int nplanes = a.filter_uv ? 3 : 1;
    mi::LfArgs cols = a, rows = a;
    int nc = 0, nr = 0;
    for (int p = 0; p < 3; p++) {
        const int sh = p ? a.ss_hor : 0, sv = p ? a.ss_ver : 0;
        cols.blk_start[p] = nc;
        rows.blk_start[p] = nr;
        if (p >= nplanes) continue;
        cols.units_x[p] = (a.w4 + sh) >> sh;
        cols.rows[p] = (a.sb128h * 128) >> sv;
        nc += ((cols.units_x[p] + 63) / 64) * ((cols.rows[p] + 3) / 4);
        rows.units_x[p] = (a.sb128w * 128) >> sh;
        rows.rows[p] = p ? a.sb128h * (32 >> sv) : a.h4;
        nr += ((rows.units_x[p] + 63) / 64) * ((rows.rows[p] + 3) / 4);
    }
    cols.blk_start[3] = nc;
    rows.blk_start[3] = nr;
    const int r = mi::launch_deblock(cols, rows, pic->bpc, (hipStream_t)stream);
    return r ? fail(ctx, -EIO) : 0;
}

static int deblock_tiles(MiCtx *ctx, const MiPicture *src, const MiPicture *dst, const MiLoopFilter *lf,
                         void *stream, uint32_t dc_tag);

int mi_deblock_frame_to(MiCtx *ctx, const MiPicture *src, const MiPicture *dst, const MiLoopFilter *lf,
                        void *stream) {
    if (ctx) ctx->dc_pending = 0;   // as mi_deblock_frame: a pending deferral is dropped
    return deblock_tiles(ctx, src, dst, lf, stream, 0);
}

int mi_deblock_frame_dc(MiCtx *ctx, const MiPicture *src, const MiPicture *dst, const MiLoopFilter *lf,
                        void *stream) {
    if (!ctx) return -EINVAL;
    const uint32_t tag = ctx->dc_pending;
    if (tag) {
        // a tag fixed in a graph would let every replay add whatever entries then carry it: a
        // deferral made outside the capture is refused here and stays pending
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) return fail(ctx, -EIO);
        if (cap != hipStreamCaptureStatusNone) return fail(ctx, -EINVAL);
    }
    ctx->dc_pending = 0;
    if (tag && (!src || src->w != ctx->dc_w || src->h != ctx->dc_h || src->layout != ctx->dc_layout))
        return fail(ctx, -EINVAL);
    return deblock_tiles(ctx, src, dst, lf, stream, tag);
}

static int deblock_tiles(MiCtx *ctx, const MiPicture *src, const MiPicture *dst, const MiLoopFilter *lf,
                         void *stream, uint32_t dc_tag) {
    if (!ctx || !src || !dst || !lf) return fail(ctx, -EINVAL);
    if (src->bpc != 8 && src->bpc != 10 && src->bpc != 12) return fail(ctx, -EINVAL);
    if (!same_geometry(src, dst)) return fail(ctx, -EINVAL);
    if (src->data[0] == dst->data[0]) {
        if (dc_tag) return fail(ctx, -EINVAL);   // deferred DC needs the out-of-place tiles
        return mi_deblock_frame(ctx, dst, lf, stream);
    }
    const int sh = src->layout == 1 || src->layout == 2, sv = src->layout == 1;
    const int nplanes = src->layout == 0 ? 1 : 3;
    const size_t px = src->bpc == 8 ? 1 : 2;
    const int sb128w = (src->w + 127) >> 7, sb128h = (src->h + 127) >> 7;
    for (int p = 0; p < nplanes; p++)
        if (src->stride[p ? 1 : 0] % 16 || (uintptr_t)src->data[p] % 16 || (uintptr_t)dst->data[p] % 16 ||
            src->stride[p ? 1 : 0] < (ptrdiff_t)(((sb128w * 128) >> (p ? sh : 0)) * px))
            return fail(ctx, -EINVAL);
    const bool edges = lf->filter_y != 0;
    if (!edges && !dc_tag) {   // deblocking off for the frame: the output is the input
        for (int p = 0; p < nplanes; p++) {
            const size_t rows = (size_t)(sb128h * 128) >> (p ? sv : 0);
            const ptrdiff_t s = src->stride[p ? 1 : 0];
            if (hipMemcpyAsync(dst->data[p], src->data[p], rows * s, hipMemcpyDeviceToDevice,
                               (hipStream_t)stream) != hipSuccess)
                return fail(ctx, -EIO);
        }
        return 0;
    }
    if (edges && (!lf->level || !lf->masks || lf->sb128w != sb128w || lf->b4_stride < (int64_t)sb128w * 32))
        return fail(ctx, -EINVAL);
    mi::LfTileArgs a;
    memset(&a, 0, sizeof(a));
    a.level = (const uint32_t *)lf->level;
    a.b4_stride = lf->b4_stride;
    a.masks = lf->masks;
    a.sb128w = sb128w;
    a.w4 = (src->w + 3) >> 2;
    a.h4 = (src->h + 3) >> 2;
    a.ss_hor = sh;
    a.ss_ver = sv;
    a.bdmax = (1 << src->bpc) - 1;
    a.bdm8 = src->bpc - 8;
    const int filter_uv = edges && src->layout != 0 && lf->filter_uv;
    memcpy(a.lim_e, lf->lim_e, 64);
    memcpy(a.lim_i, lf->lim_i, 64);
    int n = 0;
    for (int p = 0; p < 3; p++) {
        a.tile_start[p] = n;
        if (p >= nplanes) continue;
        const int h = p ? sh : 0, v = p ? sv : 0;
        a.src[p] = (const uint8_t *)src->data[p];
        a.dst[p] = (uint8_t *)dst->data[p];
        a.stride[p] = src->stride[p ? 1 : 0];
        a.pw[p] = (sb128w * 128) >> h;
        a.ph[p] = (sb128h * 128) >> v;
        // filter_uv off: chroma tiles are copies (no edge codes); deblocking off (deferred DC
        // only): every tile is a copy plus its units' DC
        const bool off = !edges || (p && !filter_uv);
        a.cols_ux[p] = off ? 0 : (a.w4 + h) >> h;
        a.cols_rows[p] = off ? 0 : a.ph[p];
        a.rows_px[p] = off ? 0 : a.pw[p];
        a.rows_uy[p] = off ? 0 : p ? sb128h * (32 >> v) : a.h4;
        a.tiles_x[p] = (a.pw[p] + mi::kLfTW - 1) / mi::kLfTW;
        n += a.tiles_x[p] * ((a.ph[p] + mi::kLfTH - 1) / mi::kLfTH);
    }
    a.tile_start[3] = n;
    if (dc_tag) {
        const mi::DcMapGeom g = mi::dc_map_geom(src->w, src->h, src->layout);
        a.dc_map = ctx->dc_map;
        for (int p = 0; p < 3; p++) {
            a.dc_off[p] = g.off[p];
            a.dc_stride[p] = g.stride[p];
        }
        a.dc_tag = dc_tag;
    }
    return mi::launch_deblock_tiles(a, src->bpc, (hipStream_t)stream) ? fail(ctx, -EIO) : 0;
}

int mi_cdef_frame(MiCtx *ctx, const MiPicture *src, const MiPicture *dst, const MiCdef *cd,
                  void *stream) {
    if (!ctx || !src || !dst || !cd || !cd->masks) return fail(ctx, -EINVAL);
    if (src->bpc != dst->bpc || src->w != dst->w || src->h != dst->h || src->layout != dst->layout ||
        src->stride[0] != dst->stride[0] || src->stride[1] != dst->stride[1])
        return fail(ctx, -EINVAL);
    if (src->bpc != 8 && src->bpc != 10 && src->bpc != 12) return fail(ctx, -EINVAL);
    mi::CdefArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < 3; p++) {
        a.src[p] = (const uint8_t *)src->data[p];
        a.dst[p] = (uint8_t *)dst->data[p];
        a.stride[p] = src->stride[p ? 1 : 0];
    }
    a.masks = cd->masks;
    a.sb128w = cd->sb128w;
    if (a.sb128w != (src->w + 127) >> 7) return fail(ctx, -EINVAL);
    a.bw4 = ((src->w + 7) >> 3) << 1;
    a.bh4 = ((src->h + 7) >> 3) << 1;
    a.layout = src->layout;
    a.ss_hor = src->layout == 1 || src->layout == 2;
    a.ss_ver = src->layout == 1;
    a.bdm8 = src->bpc - 8;
    a.damping = cd->damping + a.bdm8;
    memcpy(a.y_strength, cd->y_strength, 8);
    memcpy(a.uv_strength, cd->uv_strength, 8);
    a.tiles_x = (a.bw4 * 4 + 63) / 64;
    a.order = cd->order;
    const int tiles_y = (a.bh4 * 4 + 63) / 64;
    const int r = mi::launch_cdef(a, a.tiles_x * tiles_y, src->bpc, (hipStream_t)stream);
    return r ? fail(ctx, -EIO) : 0;
}

// Costliest class first (cls[t] in 0 .. nclass-1, higher = costlier); within a class the items
// are dealt to the XCDs in contiguous picture runs: workgroup b runs on XCD b % 8, so XCD x takes
// one run of each class and neighbouring tiles share an L2 (the locality xcd_block gives the
// grid order: CDEF 39.2 us this way, 40.1 in xcd_block's grid order, 42.2 for a plain
// costliest-first order)
static void deal_classes(const std::vector<uint8_t> &cls, int nclass, int32_t *order) {
    const int nt = (int)cls.size();
    int b = 0;
    for (int c = nclass - 1; c >= 0; c--) {
        std::vector<int32_t> items;
        for (int t = 0; t < nt; t++)
            if (cls[t] == c) items.push_back(t);
        const int L = (int)items.size();
        int cnt[8] = {}, pos[8];
        for (int r = 0; r < L; r++) cnt[(b + r) & 7]++;
        for (int x = 0, acc = 0; x < 8; x++) {
            pos[x] = acc;
            acc += cnt[x];
        }
        for (int r = 0; r < L; r++) order[b + r] = items[pos[(b + r) & 7]++];
        b += L;
    }
}

int mi_cdef_tile_order(const MiAv1Filter *masks, int w, int h, int layout, const MiCdef *cd, int32_t *order, int n) {
    if (!masks || !cd || !order || w <= 0 || h <= 0 || layout < 0 || layout > 3) return -EINVAL;
    if (cd->sb128w != (w + 127) >> 7) return -EINVAL;
    const int bw4 = ((w + 7) >> 3) << 1, bh4 = ((h + 7) >> 3) << 1;
    const int tx = (bw4 * 4 + 63) / 64, ty = (bh4 * 4 + 63) / 64, nt = tx * ty;
    if (nt > n) return -EINVAL;
    // cost class per unit (cdef_kernel's own tests): 2 a primary strength (direction search and
    // filter), 1 a secondary one only, 0 nothing to filter (no strength, or every 8x8 skipped);
    // then a stable counting sort, costliest first
    std::vector<uint8_t> cls(nt, 0);
    for (int t = 0; t < nt; t++) {
        const int x = t % tx, y = t / tx;
        const MiAv1Filter &lf = masks[(y >> 1) * cd->sb128w + (x >> 1)];
        const int idx = lf.cdef_idx[(y & 1) * 2 + (x & 1)];
        if (idx < 0) continue;
        const int yl = cd->y_strength[idx], uvl = layout ? cd->uv_strength[idx] : 0;
        if (!yl && !uvl) continue;
        // the unit's 8x8 rows (16 per 128-px superblock row, half of them per 64-px unit) and
        // its half of each row's 32-bit noskip word
        unsigned any = 0;
        for (int r = 8 * (y & 1); r < 8 * (y & 1) + 8; r++)
            any |= ((unsigned)lf.noskip_mask[r][1] << 16 | lf.noskip_mask[r][0]) >> (16 * (x & 1)) & 0xffffu;
        if (!any) continue;
        cls[t] = (yl >> 2) || (uvl >> 2) ? 2 : 1;
    }
    deal_classes(cls, 3, order);
    return nt;
}

// The (plane, stripe, tile) grid of mi_lr_frame for a w x h picture (pw, ph, tw, tiles_x,
// blk_start of `a`); -EINVAL for unit sizes outside the bitstream's
static int lr_layout(int w, int h, int layout, const MiLr *lr, mi::LrArgs &a) {
    const int ss_hor = layout == 1 || layout == 2, ss_ver = layout == 1;
    for (int c = 0; c < 2; c++) {
        const int l2 = lr->unit_size_log2[c];
        if ((lr->restore_planes & (c ? 6 : 1)) && (l2 < 5 || l2 > 8)) return -EINVAL;
    }
    a.restore = lr->restore_planes;
    a.ss_hor = ss_hor;
    a.ss_ver = ss_ver;
    a.unit_log2[0] = lr->unit_size_log2[0];
    a.unit_log2[1] = lr->unit_size_log2[1];
    a.sb128w = lr->sb128w;
    const int nplanes = layout ? 3 : 1;
    int nb = 0;
    for (int p = 0; p < 3; p++) {
        a.blk_start[p] = nb;
        if (p >= nplanes) continue;
        const int sh = p ? ss_hor : 0, sv = p ? ss_ver : 0;
        a.pw[p] = (w + sh) >> sh;
        a.ph[p] = (h + sv) >> sv;
        const int us = 1 << lr->unit_size_log2[p ? 1 : 0];
        a.tw[p] = ((a.restore >> p) & 1) && us < 64 ? 32 : 64;
        a.tiles_x[p] = (a.pw[p] + a.tw[p] - 1) / a.tw[p];
        // stripes: 64 luma rows, the first 56 (lr_apply.rs:54)
        int stripes = 0;
        while ((stripes ? (64 * stripes - 8) >> sv : 0) < a.ph[p]) stripes++;
        nb += stripes * a.tiles_x[p];
    }
    a.blk_start[3] = nb;
    return 0;
}

int mi_lr_frame(MiCtx *ctx, const MiPicture *cdef, const MiPicture *deblocked, const MiPicture *dst,
                const MiLr *lr, void *stream) {
    if (!ctx || !cdef || !deblocked || !dst || !lr) return fail(ctx, -EINVAL);
    if (!same_geometry(cdef, deblocked) || !same_geometry(cdef, dst)) return fail(ctx, -EINVAL);
    if (cdef->bpc != 8 && cdef->bpc != 10 && cdef->bpc != 12) return fail(ctx, -EINVAL);
    if (lr->restore_planes && (!lr->lr_mask || lr->sb128w != (cdef->w + 127) >> 7)) return fail(ctx, -EINVAL);
    mi::LrArgs a;
    memset(&a, 0, sizeof(a));
    if (lr_layout(cdef->w, cdef->h, cdef->layout, lr, a)) return fail(ctx, -EINVAL);
    a.lr_mask = lr->lr_mask;
    a.bd = cdef->bpc;
    a.order = lr->order;
    for (int p = 0; p < (cdef->layout ? 3 : 1); p++) {
        a.src[p] = (const uint8_t *)cdef->data[p];
        a.lpf[p] = (const uint8_t *)deblocked->data[p];
        a.dst[p] = (uint8_t *)dst->data[p];
        a.stride[p] = cdef->stride[p ? 1 : 0];
        // lr.hip forms row offsets with one 24-bit multiply
        if (a.stride[p] <= 0 || a.stride[p] >= (1 << 24) || (int64_t)a.ph[p] * a.stride[p] >= (1LL << 32))
            return fail(ctx, -EINVAL);
    }
    const int r = mi::launch_lr(a, cdef->bpc, (hipStream_t)stream);
    return r ? fail(ctx, -EIO) : 0;
}

int mi_lr_tile_order(const MiAv1Restoration *mask, int w, int h, int layout, const MiLr *lr, int32_t *order,
                     int n) {
    if (!lr || !order || w <= 0 || h <= 0 || layout < 0 || layout > 3) return -EINVAL;
    if (lr->restore_planes && !mask) return -EINVAL;
    mi::LrArgs a;
    memset(&a, 0, sizeof(a));
    if (lr_layout(w, h, layout, lr, a) || a.blk_start[3] > n) return -EINVAL;
    // cost class per tile (lr_kernel's unit lookup): 3 self-guided with both radii, 2 with one
    // (sgr_params 10-15), 1 Wiener, 0 copy; then a stable counting sort, costliest first
    std::vector<uint8_t> cls(a.blk_start[3], 0);
    for (int p = 0; p < 3; p++) {
        if (!((a.restore >> p) & 1)) continue;
        const int ssh = p ? a.ss_hor : 0, ssv = p ? a.ss_ver : 0, pw = a.pw[p], ph = a.ph[p];
        const int us = 1 << a.unit_log2[p ? 1 : 0], nu = std::max(1, (pw + (us >> 1)) / us);
        for (int b = a.blk_start[p]; b < a.blk_start[p + 1]; b++) {
            const int lb = b - a.blk_start[p], k = lb / a.tiles_x[p], ti = lb - k * a.tiles_x[p];
            const int xu = std::min(ti * a.tw[p] / us, nu - 1) * us;
            int ay = ((64 * k) >> ssv) & ~(us - 1);
            if (ay && ay + (us >> 1) > ph) ay -= us;
            ay <<= ssv;
            const int t = mask[(ay >> 7) * a.sb128w + (xu >> (7 - ssh))].lr[p][(((ay >> 6) & 1) << 1) + ((xu >> (6 - ssh)) & 1)].type;
            cls[b] = t == 0 ? 0 : t == 2 ? 1 : t >= 3 && t - 3 < 10 ? 3 : t >= 3 ? 2 : 0;
        }
    }
    // (each class dealt to the XCDs in contiguous picture runs, as CDEF's order is, halves LR's
    // HBM reads, 68.0 -> 35.9 MB, but runs 35.0-35.8 us against 31.5-32.1: DESIGN.md, round 6)
    int start[5] = {};
    for (uint8_t c : cls) start[3 - c + 1]++;
    for (int c = 0; c < 4; c++) start[c + 1] += start[c];
    for (int b = 0; b < a.blk_start[3]; b++) order[start[3 - cls[b]]++] = b;
    return a.blk_start[3];
}

static int fg_setup(MiCtx *ctx, const MiPicture *in, const MiPicture *out, const MiFilmGrainData *data,
                    int is_id, mi::FgArgs &a) {
    if (int e = fg_tables()) return e;
    if (in->bpc != 8 && in->bpc != 10 && in->bpc != 12) return -EINVAL;
    if (!fg_data_ok(data)) return -EINVAL;
    memset(&a, 0, sizeof(a));
    a.data = *data;
    a.bpc = in->bpc;
    a.layout = in->layout;
    a.ss_x = in->layout == 1 || in->layout == 2;
    a.ss_y = in->layout == 1;
    a.w = in->w;
    a.h = in->h;
    a.is_id = is_id;
    a.nrows = (in->h + 31) >> 5;
    a.nblocks = (in->w + 31) >> 5;
    if (!ctx->fg_lut && hipMalloc(&ctx->fg_lut, 3 * 73 * 88 * sizeof(int16_t)) != hipSuccess) return -ENOMEM;
    if (!ctx->fg_scaling && hipMalloc(&ctx->fg_scaling, 3 * 4096) != hipSuccess) return -ENOMEM;
    const size_t ob = (size_t)a.nrows * a.nblocks;
    if (ob > ctx->fg_offsets_bytes) {
        if (ctx->fg_offsets) (void)hipFree(ctx->fg_offsets);
        ctx->fg_offsets = nullptr;
        if (hipMalloc(&ctx->fg_offsets, ob) != hipSuccess) return -ENOMEM;
        ctx->fg_offsets_bytes = ob;
    }
    a.lut = ctx->fg_lut;
    a.scaling = ctx->fg_scaling;
    a.offsets = ctx->fg_offsets;
    if (out) {
        if (!same_geometry(in, out)) return -EINVAL;
        const int nplanes = in->layout ? 3 : 1;
        int nb = 0;
        for (int p = 0; p < 3; p++) {
            a.blk_start[p] = nb;
            if (p >= nplanes) continue;
            a.src[p] = (const uint8_t *)in->data[p];
            a.dst[p] = (uint8_t *)out->data[p];
            a.stride[p] = in->stride[p ? 1 : 0];
            const int sh = p ? a.ss_x : 0, sv = p ? a.ss_y : 0;
            a.pw[p] = (in->w + sh) >> sh;
            a.ph[p] = (in->h + sv) >> sv;
            a.chunks[p] = (a.pw[p] + 511) / 512;   // 64-lane waves per row, 8 contiguous px per lane
            a.grain[p] = p == 0 ? data->num_y_points != 0
                                : (data->chroma_scaling_from_luma || data->num_uv_points[p - 1]);
            nb += (int)(((int64_t)a.chunks[p] * a.ph[p] + 4 * mi::kFgItems - 1) / (4 * mi::kFgItems));
        }
        a.blk_start[3] = nb;
    }
    return 0;
}

int mi_film_grain_prep(MiCtx *ctx, const MiPicture *in, const MiFilmGrainData *data, void *stream) {
    if (!ctx || !in || !data) return fail(ctx, -EINVAL);
    mi::FgArgs a;
    if (int e = fg_setup(ctx, in, nullptr, data, 0, a)) return fail(ctx, e);
    return mi::launch_fg(a, (hipStream_t)stream, true, false) ? fail(ctx, -EIO) : 0;
}

int mi_film_grain_apply(MiCtx *ctx, const MiPicture *in, const MiPicture *out, const MiFilmGrainData *data,
                        int mtrx_identity, void *stream) {
    if (!ctx || !in || !out || !data) return fail(ctx, -EINVAL);
    mi::FgArgs a;
    if (int e = fg_setup(ctx, in, out, data, mtrx_identity, a)) return fail(ctx, e);
    return mi::launch_fg(a, (hipStream_t)stream, false, true) ? fail(ctx, -EIO) : 0;
}

int mi_film_grain_frame(MiCtx *ctx, const MiPicture *in, const MiPicture *out, const MiFilmGrainData *data,
                        int mtrx_identity, void *stream) {
    if (!ctx || !in || !out || !data) return fail(ctx, -EINVAL);
    mi::FgArgs a;
    if (int e = fg_setup(ctx, in, out, data, mtrx_identity, a)) return fail(ctx, e);
    return mi::launch_fg(a, (hipStream_t)stream, true, true) ? fail(ctx, -EIO) : 0;
}
}  // extern "C"

namespace mi_internal {

// mi_intra_recon, and the strip form frame_exec.cpp uses for a single frame: with nstrips > 1
// the frame's blocks are grouped by strip (strip q = blocks [strip_start[q], strip_start[q+1]),
// each in dependency order), deps index the whole frame, and queue q (strip q) runs on XCD q.
int intra_recon(MiCtx *ctx, const MiIntraFrame *frames, int nframes, const int32_t *strip_start, int nstrips,
                unsigned flags, void *stream, bool granules) {
    if (!ctx || !frames || nframes < 1 || nframes > mi::kIrMaxFrames) return fail(ctx, -EINVAL);
    if (nstrips > 1 && (nframes != 1 || nstrips > 8 || !strip_start)) return fail(ctx, -EINVAL);
    const int bpc = frames[0].pic.bpc;
    if (bpc != 8 && bpc != 10 && bpc != 12) return fail(ctx, -EINVAL);
    size_t total = 0;
    for (int f = 0; f < nframes; f++) {
        const MiIntraFrame &fr = frames[f];
        if (fr.pic.bpc != bpc || fr.n < 0 || (fr.n && (!fr.blocks || !fr.tx || !fr.dep_start || !fr.coef)))
            return fail(ctx, -EINVAL);
        total += (size_t)fr.n;
    }
    if (nstrips > 1)
        for (int q = 0; q < nstrips; q++)
            if (strip_start[0] != 0 || strip_start[q + 1] < strip_start[q] || strip_start[nstrips] != frames[0].n)
                return fail(ctx, -EINVAL);
    if (int e = ctx_words(ctx, (hipStream_t)stream)) return fail(ctx, e);
    if (total > ctx->ir_done_n) {
        // an earlier launch on this context's stream may still poll the old flags
        if (ctx->ir_done && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(ctx, -EIO);
        if (ctx->ir_done) (void)hipFree(ctx->ir_done);
        ctx->ir_done = nullptr;
        ctx->ir_done_n = 0;
        if (hipMalloc(&ctx->ir_done, total * sizeof(uint32_t)) != hipSuccess) return fail(ctx, -ENOMEM);
        // stream-ordered, as ctx_words
        if (hipMemsetAsync(ctx->ir_done, 0, total * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess)
            return fail(ctx, -EIO);
        ctx->ir_done_n = total;
    }
    if (++ctx->ir_epoch == 0) ctx->ir_epoch = 1;   // done words hold the epoch of the last call
    hipStream_t s = (hipStream_t)stream;
    mi::IntraReconArgs a;
    memset(&a, 0, sizeof(a));
    // edge granules: one region per frame (mi::gran_count), zeroed once when (re)allocated
    std::vector<uint32_t> goff(nframes, 0);
    if (granules) {
        size_t ng = 0;
        for (int f = 0; f < nframes; f++) {
            const MiPicture &pic = frames[f].pic;
            goff[f] = (uint32_t)ng;
            ng += mi::gran_count((pic.w + 127) & ~127, (pic.h + 127) & ~127, pic.layout == 1 || pic.layout == 2,
                                 pic.layout == 1, pic.layout ? 3 : 1);
        }
        if (ng > 0xffffffffull) return fail(ctx, -EINVAL);
        if (ng > ctx->ir_gran_n) {
            if (ctx->ir_gran && hipStreamSynchronize(s) != hipSuccess) return fail(ctx, -EIO);
            if (ctx->ir_gran) (void)hipFree(ctx->ir_gran);
            ctx->ir_gran = nullptr;
            ctx->ir_gran_n = 0;
            if (hipMalloc((void **)&ctx->ir_gran, ng * 8) != hipSuccess) return fail(ctx, -ENOMEM);
            if (hipMemsetAsync(ctx->ir_gran, 0, ng * 8, s) != hipSuccess) return fail(ctx, -EIO);
            ctx->ir_gran_n = ng;
        }
        a.gran = ctx->ir_gran;
    }
    const int nq = nstrips > 1 ? nstrips : nframes;
    size_t off = 0;
    for (int q = 0; q < nq; q++) {
        const MiIntraFrame &fr = frames[nstrips > 1 ? 0 : q];
        const int s0 = nstrips > 1 ? strip_start[q] : 0;
        mi::IntraReconFrame &d = a.fr[q];
        for (int p = 0; p < 3; p++) d.ip.dst[p] = (uint8_t *)fr.pic.data[p];
        d.ip.stride[0] = fr.pic.stride[0];
        d.ip.stride[1] = fr.pic.stride[1];
        d.ip.iblocks = fr.blocks + s0;
        d.ip.ac = fr.ac;
        d.ip.idx = fr.idx;
        d.ip.pal = (const uint8_t *)fr.pal;
        d.ip.bpc = bpc;
        d.ip.bdmax = (1 << bpc) - 1;
        d.tx = fr.tx + s0;
        d.coef = (uint8_t *)fr.coef;
        d.dep_start = fr.dep_start + s0;
        d.deps = fr.deps;
        d.done = ctx->ir_done + off;
        d.base = s0;
        d.head = ctx->ir_words + q;
        d.n = nstrips > 1 ? strip_start[q + 1] - s0 : fr.n;
        d.pw = (uint16_t)((fr.pic.w + 127) & ~127);
        d.ph = (uint16_t)((fr.pic.h + 127) & ~127);
        d.ss_hor = fr.pic.layout == 1 || fr.pic.layout == 2;
        d.ss_ver = fr.pic.layout == 1;
        d.nplanes = fr.pic.layout ? 3 : 1;
        d.goff = goff[nstrips > 1 ? 0 : q];
        if (nstrips <= 1) off += (size_t)fr.n;
    }
    // queue heads and XCD worker ranks start from 0 in stream order
    if (hipMemsetAsync(ctx->ir_words, 0, 64 * sizeof(int), s) != hipSuccess ||
        hipMemsetAsync(ctx->ir_words + 72, 0, 8 * sizeof(int), s) != hipSuccess)
        return fail(ctx, -EIO);
    a.xcd_rank = ctx->ir_words + 72;
    a.err = ctx->ir_words + 64;
    a.desc_err = ctx->ir_words + 65;
#ifdef MI_IR_DEBUG
    static int *dbg = nullptr;
    if (!dbg && hipHostMalloc((void **)&dbg, 65536 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        return fail(ctx, -ENOMEM);
    memset(dbg, 0, 65536 * sizeof(int));
    int *ddbg = nullptr;
    (void)hipHostGetDevicePointer((void **)&ddbg, dbg, 0);
    a.dbg = ddbg;
    setenv("MI_IR_DBG_PTR", std::to_string((uintptr_t)dbg).c_str(), 1);
#endif
    static const bool tl_env = getenv("MI_IR_TIMELINE") != nullptr;
    if (tl_env) {
        if (ctx->ir_tl_n < ctx->ir_done_n) {
            if (ctx->ir_tl) (void)hipFree(ctx->ir_tl);
            ctx->ir_tl = nullptr;
            ctx->ir_tl_n = 0;
            if (hipMalloc((void **)&ctx->ir_tl, ctx->ir_done_n * 128) != hipSuccess) return fail(ctx, -ENOMEM);
            ctx->ir_tl_n = ctx->ir_done_n;
        }
        a.tl = (uintptr_t)ctx->ir_tl - (uintptr_t)ctx->ir_done * 32;
    }
    a.epoch = ctx->ir_epoch;
    a.nframes = nq;
    a.zero_coefs = (flags & MI_ITX_KEEP_COEFS) ? 0 : 1;
    // one-wave workers per XCD (VGPRs allow 2 per SIMD = 256 per XCD, LDS 7 per CU): one per
    // ~96 units of the busiest XCD's first queue, 128 to 192 (a worker that arrives after its
    // block's producer finished adds to the chain: 4K intra frames gain 25 % from 128 to 192;
    // 352x288 frames lose 15 % at 64), plus 64 per extra queue the XCD serves
    const int per_xcd = (nq + 7) / 8;
    int n_xcd = 0;
    for (int q = 0; q < nq && q < 8; q++) n_xcd = std::max(n_xcd, a.fr[q].n);
    const int wpx = std::min(256, std::max(128, std::min(192, n_xcd / 96)) + 64 * (per_xcd - 1));
    return mi::launch_intra_recon(a, bpc, wpx, s) ? fail(ctx, -EIO) : 0;
}

}  // namespace mi_internal
