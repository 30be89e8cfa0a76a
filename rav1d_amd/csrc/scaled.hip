// scaled.hip — mi_display_scaled (include/mi_av1out.h): a shown picture as cropped, resized
// semi-planar YUV at a chosen depth, up to 8 rungs of a transcode ladder per call. The resize is
// the separable 18-bit filter of resize.h (the triangle, or with mi_display_scaled_rs a cubic: its
// signed sums are clamped to [0, Ms] by CUBIC, a compile-time switch of both passes that leaves
// the triangle's instantiations as they were) run in the YUV domain: every plane on its own,
// at its own resolution, the chroma siting in the taps (a co-sited axis takes the (4o+1) / (4i+1)
// form of the formula), so there is no chroma upsample and no matrix.
//
// Launches on the caller's stream, all scratch in one context-owned allocation of its own (the
// tensor output's tables are never these):
//   taps_kernel          (resize.h) the tap tables of every axis of every rung (up to four axes
//                        per rung: luma x, luma y, chroma x, chroma y); skipped when the scratch
//                        holds the tables of the same rungs;
//   per rung:
//   scaled_h_kernel      one workgroup per (plane row of the crop, segment of output columns); the
//                        U and V rows of a chroma row go together. The lanes stage the run of the
//                        row the segment's taps reach in LDS (display.h load_run: one vector per 8
//                        samples), then a lane owns output columns and filters from LDS into `mid`
//                        (u16). The segment is sized on the host so that the taps fit kTensorSeg.
//                        Rows outside the crop are not read;
//   scaled_v_kernel      a lane owns 4 adjacent output columns of one output row (of U and V
//                        both): per tap one 8-byte load of `mid` per channel and a wave-uniform
//                        weight; then the depth conversion and the store, Y as one vector of 4
//                        samples, UV as one vector of 4 interleaved pairs, where the pointer and
//                        the stride allow, else sample by sample.
// Luma and chroma of a rung share each launch: the first blocks are luma's.
//
// mi_display_scaled_tm is the same call on the tone-mapped picture Q: one launch of yuv_tm.hip's
// kernel writes Q as planes of dst_bpc into a scratch picture of the context's, after the grain
// step and in front of the passes, which read it in place of the source.
#include <algorithm>
#include <cerrno>
#include <cstring>

#include "resize.h"

namespace mi {
namespace {

// ---- horizontal pass ----
template <typename Px, int NC, bool CUBIC>
__device__ __forceinline__ void h_pass(const ScaledPlane &p, int r, int seg, uint16_t (&tile)[2][kTensorSeg], [[maybe_unused]] int maxs) {
    const int o0 = seg * p.ob, o1 = min(o0 + p.ob, p.ow) - 1;
    const int *hs = p.htab, *hc = hs + p.ow, *hk = hc + p.ow;
    // plane columns [lo, hi) the segment's taps read, inside the crop whatever the tables hold;
    // the tile starts at the 8-column run of lo
    const int lo = p.px + min(max(hs[o0], 0), p.pcw - 1), hi = p.px + min(max(hs[o1] + hc[o1], 1), p.pcw);
    const int xa = lo & ~7, x0 = xa + 8 * (int)threadIdx.x;
    if (x0 < hi && x0 - xa + 8 <= kTensorSeg) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            int v[8];
            load_run<Px, 8>(p.src[c] + (int64_t)(p.py + r) * p.sstride, x0, p.pw, (p.svec >> c) & 1, v);
            *reinterpret_cast<uint4 *>(&tile[c][x0 - xa]) = pack8(v);
        }
    }
    __syncthreads();
    // the crop's columns as tile columns, held inside the tile
    const int lo_i = max(p.px - xa, 0), hi_i = min(p.px - xa + p.pcw - 1, kTensorSeg - 1);
    for (int o = o0 + (int)threadIdx.x; o <= o1; o += 256) {
        const int base = hs[o] + p.px - xa;
        const int *k = hk + o;
        int acc[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = kTensorHalf;
#pragma unroll 4
        for (int j = 0; j < p.th; j++) h_tap<NC>(tile, base + j, lo_i, hi_i, k[(int64_t)j * p.ow], acc);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            int v = acc[c] >> kTensorS;
            if constexpr (CUBIC) v = min(max(v, 0), maxs);
            p.mid[((int64_t)c * p.pch + r) * p.mstride + o] = (uint16_t)v;
        }
    }
}

template <bool CUBIC> struct ScaledSel { using type = ScaledArgs; };
template <> struct ScaledSel<true> { using type = ScaledCubicArgs; };
template <bool CUBIC> using ScaledParam = typename ScaledSel<CUBIC>::type;
template <bool CUBIC>
__device__ __forceinline__ int clamp_max(const ScaledParam<CUBIC> &a) {
    if constexpr (CUBIC)
        return a.maxs;
    else
        return 0;   // (not read)
}

template <typename Px, bool CUBIC>
__global__ __launch_bounds__(256) void scaled_h_kernel(const ScaledParam<CUBIC> a) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[2][kTensorSeg];
    const int r = blockIdx.x, seg = blockIdx.y;
    if (r < a.p[0].pch) {   // (block-uniform: every lane of a workgroup meets the barrier or none)
        if (seg < a.p[0].segs) h_pass<Px, 1, CUBIC>(a.p[0], r, seg, tile, clamp_max<CUBIC>(a));
    } else if (a.nplanes > 1 && r - a.p[0].pch < a.p[1].pch) {
        if (seg < a.p[1].segs) h_pass<Px, 2, CUBIC>(a.p[1], r - a.p[0].pch, seg, tile, clamp_max<CUBIC>(a));
    }
}

// ---- vertical pass, depth, store ----
template <typename Dx, int NC, bool CUBIC>
__device__ __forceinline__ void v_pass(const ScaledArgs &a, const ScaledPlane &p, int oy, int xb, [[maybe_unused]] int maxs) {
    const int x0 = (xb * 256 + (int)threadIdx.x) * 4;
    if (x0 >= p.ow) return;
    const int *vs = p.vtab, *vk = vs + 2 * p.oh;
    // (rows of mid are 16-byte aligned and x0 is a multiple of 4; columns past ow are padding)
    const int s = vs[oy];
    const uint16_t *m = p.mid + x0;
    const int64_t plane = (int64_t)p.pch * p.mstride;
    int acc[NC][4];
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[c][i] = kTensorHalf;
#pragma unroll 4
    for (int j = 0; j < p.tv; j++)
        v_tap<NC>(m, plane, min(max(s + j, 0), p.pch - 1) * p.mstride, vk[(int64_t)j * p.oh + oy], acc);
    // samples in store order: Y0 .. Y3, or U0 V0 .. U3 V3
    uint32_t e[4 * NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int v = acc[c][i] >> kTensorS;
            if constexpr (CUBIC) v = min(max(v, 0), maxs);
            if (a.down) v = min(a.maxd, (v + (1 << (a.down - 1))) >> a.down);
            e[NC * i + c] = (uint32_t)(v << a.up);
        }
    Dx *d = reinterpret_cast<Dx *>(p.dst + (int64_t)oy * p.dstride) + NC * x0;
    if (p.dvec && x0 + 4 <= p.ow) {
        if constexpr (sizeof(Dx) == 1) {
            const uint32_t w0 = e[0] | (e[1] << 8) | (e[2] << 16) | (e[3] << 24);
            if constexpr (NC == 1)
                *reinterpret_cast<uint32_t *>(d) = w0;
            else
                *reinterpret_cast<uint2 *>(d) = make_uint2(w0, e[4] | (e[5] << 8) | (e[6] << 16) | (e[7] << 24));
        } else {
            if constexpr (NC == 1)
                *reinterpret_cast<uint2 *>(d) = make_uint2(e[0] | (e[1] << 16), e[2] | (e[3] << 16));
            else
                *reinterpret_cast<uint4 *>(d) = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16),
                                                           e[6] | (e[7] << 16));
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4 * NC; i++)
            if (x0 + i / NC < p.ow) d[i] = (Dx)e[i];
    }
}

template <typename Dx, bool CUBIC>
__global__ __launch_bounds__(256) void scaled_v_kernel(const ScaledParam<CUBIC> a) {
    const int n0 = a.p[0].xblocks * a.p[0].oh;
    int b = blockIdx.x;
    if (b < n0) {
        v_pass<Dx, 1, CUBIC>(a, a.p[0], b / a.p[0].xblocks, b % a.p[0].xblocks, clamp_max<CUBIC>(a));
    } else if (a.nplanes > 1) {
        b -= n0;
        if (b < a.p[1].xblocks * a.p[1].oh) v_pass<Dx, 2, CUBIC>(a, a.p[1], b / a.p[1].xblocks, b % a.p[1].xblocks, clamp_max<CUBIC>(a));
    }
}

template <bool CUBIC>
int launch_passes(const ScaledArgs &args, int src_bpc, int dst_bpc, hipStream_t s) {
    ScaledParam<CUBIC> a;
    static_cast<ScaledArgs &>(a) = args;
    if constexpr (CUBIC) a.maxs = (1 << src_bpc) - 1;
    const bool chroma = a.nplanes > 1;
    const dim3 hgrid(a.p[0].pch + (chroma ? a.p[1].pch : 0), chroma ? std::max(a.p[0].segs, a.p[1].segs) : a.p[0].segs);
    if (src_bpc == 8)
        scaled_h_kernel<uint8_t, CUBIC><<<hgrid, 256, 0, s>>>(a);
    else
        scaled_h_kernel<uint16_t, CUBIC><<<hgrid, 256, 0, s>>>(a);
    if (hipGetLastError() != hipSuccess) return -1;
    const unsigned vgrid = (unsigned)a.p[0].xblocks * (unsigned)a.p[0].oh + (chroma ? (unsigned)a.p[1].xblocks * (unsigned)a.p[1].oh : 0u);
    if (dst_bpc == 8)
        scaled_v_kernel<uint8_t, CUBIC><<<vgrid, 256, 0, s>>>(a);
    else
        scaled_v_kernel<uint16_t, CUBIC><<<vgrid, 256, 0, s>>>(a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

int launch_scaled(const ScaledArgs &a, int src_bpc, int dst_bpc, hipStream_t s, bool cubic) {
    return cubic ? launch_passes<true>(a, src_bpc, dst_bpc, s) : launch_passes<false>(a, src_bpc, dst_bpc, s);
}

}  // namespace mi

namespace {

// one plane group of one rung, on the host: the crop and output extents, the tap phases, and
// where its tables and its part of `mid` lie in the scratch
struct PlaneGeom {
    int px, py, pcw, pch, ow, oh, phx, phy, th, tv;
    int64_t mstride;
    size_t htab, vtab, mid;   // byte offsets
};

// the tone map and the target of mi_display_scaled_tm (either may be NULL: it rejects that)
struct YuvTm { const MiToneMap *tm; const MiYuvTarget *target; };

// mi_display_scaled (rs NULL), mi_display_scaled_rs and, with `yt`, mi_display_scaled_tm: the same
// passes over the tone-mapped picture Q (yuv_tm.hip), which a kernel in front of them writes into
// the context's scratch picture
int display_scaled(MiCtx *ctx, const MiPicture *in, const MiScaledImage *outs, int n_outs, const MiColorInfo *color,
                   const MiResample *rs, const MiFilmGrainData *fg, void *stream, const YuvTm *yt = nullptr) {
    if (!in || !outs || n_outs < 1 || n_outs > 8) return -EINVAL;
    if (int e = mi::display_check_picture(in)) return e;
    if (int e = mi::display_check_strides(in)) return e;
    const int sh = in->layout == 1 || in->layout == 2, sv = in->layout == 1;
    const int nplanes = in->layout ? 2 : 1;

    PlaneGeom g[8][2];
    for (int r = 0; r < n_outs; r++) {
        const MiScaledImage &o = outs[r];
        if (!o.data[0] || (in->layout && !o.data[1])) return -EINVAL;
        if (o.w < 1 || o.h < 1 || o.w > 65536 || o.h > 65536) return -EINVAL;
        if (o.bpc != 8 && o.bpc != 10 && o.bpc != 12) return -EINVAL;
        const ptrdiff_t es = o.bpc == 8 ? 1 : 2;
        const int ocw = (o.w + sh) >> sh, och = (o.h + sv) >> sv;
        for (int p = 0; p < nplanes; p++) {
            const int64_t row = (p ? 2 * (int64_t)ocw : (int64_t)o.w) * es;
            if ((int64_t)o.stride[p] < row || o.stride[p] % es) return -EINVAL;
            if ((uintptr_t)o.data[p] % (uintptr_t)es) return -EINVAL;
        }
        int cx, cy, cw, ch;
        if (int e = mi::display_crop(in, o.crop_x, o.crop_y, o.crop_w, o.crop_h, cx, cy, cw, ch)) return e;
        // on the chroma grid: an even origin, and an odd extent only up to the picture's edge
        // (the whole picture passes)
        if ((sh && (cx & 1)) || (sv && (cy & 1))) return -EINVAL;
        if (sh && (cw & 1) && cx + cw != in->w) return -EINVAL;
        if (sv && (ch & 1) && cy + ch != in->h) return -EINVAL;
        g[r][0] = PlaneGeom{cx, cy, cw, ch, o.w, o.h, 2, 2, 0, 0, 0, 0, 0, 0};
        g[r][1] = PlaneGeom{cx >> sh, cy >> sv, (cw + sh) >> sh, (ch + sv) >> sv, ocw, och, sh ? 4 : 2, 0, 0, 0, 0, 0, 0, 0};
        for (int p = 0; p < nplanes; p++)
            if ((int64_t)g[r][p].pcw > 64 * (int64_t)g[r][p].ow || (int64_t)g[r][p].pch > 64 * (int64_t)g[r][p].oh) return -EINVAL;
    }
    const int chr = color ? color->chr : 0;
    if (chr < 0 || chr > 2) return -EINVAL;
    mi::Filter flt;
    if (int e = mi::resample_check(rs, flt)) return e;
    const int radius = mi::filter_radius(flt);
    mi::DisplayArgs ya;
    mi::YuvArgs yf;
    memset(&ya, 0, sizeof(ya));
    memset(&yf, 0, sizeof(yf));
    if (yt)
        if (int e = mi::yuv_tm_check(in, color, yt->tm, yt->target, ctx && ctx->hlg, ya, yf)) return e;
    if (!ctx) return -EINVAL;

    // the scratch: every rung's tables (they stay while the axes stay), then one `mid` the rungs
    // use in turn (they are ordered on the stream)
    size_t tab_bytes = 0, mid_bytes = 0;
    for (int r = 0; r < n_outs; r++) {
        g[r][1].phy = sv && chr == 2 ? 4 : 2;
        size_t mid = 0;
        for (int p = 0; p < nplanes; p++) {
            PlaneGeom &q = g[r][p];
            q.th = mi::tap_cap(q.pcw, q.ow, radius);
            q.tv = mi::tap_cap(q.pch, q.oh, radius);
            q.mstride = ((int64_t)q.ow + 7) & ~(int64_t)7;
            q.htab = tab_bytes;
            tab_bytes += (size_t)(q.th + 2) * q.ow * sizeof(int);
            q.vtab = tab_bytes;
            tab_bytes += (size_t)(q.tv + 2) * q.oh * sizeof(int);
            q.mid = mid;
            mid += (size_t)(p ? 2 : 1) * q.pch * q.mstride * sizeof(uint16_t);
        }
        mid_bytes = std::max(mid_bytes, mid);
    }
    tab_bytes = (tab_bytes + 255) & ~(size_t)255;

    // allocations first: a call that fails has launched nothing
    MiResizeScratch &sc = ctx->scal;
    if (!sc.ensure(tab_bytes + mid_bytes)) return ctx->last_error = -ENOMEM;
    mi::TapList tl;
    memset(&tl, 0, sizeof(tl));
    for (int r = 0; r < n_outs; r++)
        for (int p = 0; p < nplanes; p++) {
            const PlaneGeom &q = g[r][p];
            tl.ax[tl.n++] = mi::TapAxis{q.pcw, q.ow, q.phx, q.th, (int *)(sc.p + q.htab)};
            tl.ax[tl.n++] = mi::TapAxis{q.pch, q.oh, q.phy, q.tv, (int *)(sc.p + q.vtab)};
        }
    mi::tap_filter(tl, flt);
    const bool taps = !sc.holds(tl);
    mi::ToneHlgArgs ta;
    MiPicture q;
    if (yt) {
        if (int e = mi::yuv_tm_scratch(ctx, in, yt->tm->dst_bpc, &q)) return e;
        if (int e = mi::tone_prepare(ctx, yt->tm, color, in->bpc, (hipStream_t)stream, ta)) return e;
    }
    MiPicture src = *in;
    if (fg)
        if (int e = mi::display_grain(ctx, in, &src, fg, color, stream)) return e;
    if (yt) {   // the rungs read Q: the (grained) source through the tone map, at dst_bpc
        if (mi::yuv_tm_picture(src, color, ya, ta, yf, &q, nullptr, nullptr, q.bpc, (hipStream_t)stream)) return ctx->last_error = -EIO;
        src = q;
    }

    sc.forget();
    if (taps && mi::launch_taps(tl, (hipStream_t)stream)) return ctx->last_error = -EIO;
    for (int r = 0; r < n_outs; r++) {
        const MiScaledImage &o = outs[r];
        mi::ScaledArgs a;
        memset(&a, 0, sizeof(a));
        a.nplanes = nplanes;
        a.down = o.bpc < src.bpc ? src.bpc - o.bpc : 0;
        a.up = (o.bpc > src.bpc ? o.bpc - src.bpc : 0) + (o.bpc > 8 ? 16 - o.bpc : 0);
        a.maxd = (1 << o.bpc) - 1;
        const uintptr_t es = o.bpc == 8 ? 1 : 2;
        for (int p = 0; p < nplanes; p++) {
            const PlaneGeom &q = g[r][p];
            mi::ScaledPlane &sp = a.p[p];
            for (int c = 0; c < (p ? 2 : 1); c++) {
                sp.src[c] = (const uint8_t *)src.data[p + c];
                if (mi::aligned_to(src.data[p + c], src.stride[p], 16)) sp.svec |= 1 << c;
            }
            sp.sstride = src.stride[p];
            sp.pw = p ? (in->w + sh) >> sh : in->w;
            sp.px = q.px, sp.py = q.py, sp.pcw = q.pcw, sp.pch = q.pch, sp.ow = q.ow, sp.oh = q.oh;
            sp.htab = (const int *)(sc.p + q.htab);
            sp.vtab = (const int *)(sc.p + q.vtab);
            sp.th = q.th, sp.tv = q.tv;
            sp.mid = (uint16_t *)(sc.p + tab_bytes + q.mid);
            sp.mstride = q.mstride;
            sp.ob = mi::seg_outputs(q.pcw, q.ow, radius);
            sp.segs = (q.ow + sp.ob - 1) / sp.ob;
            sp.xblocks = (q.ow + 1023) / 1024;
            sp.dst = (uint8_t *)o.data[p];
            sp.dstride = o.stride[p];
            sp.dvec = mi::aligned_to(o.data[p], o.stride[p], (p ? 8 : 4) * es);
        }
        if (mi::launch_scaled(a, src.bpc, o.bpc, (hipStream_t)stream, flt.filter == MI_RS_CUBIC)) return ctx->last_error = -EIO;
    }
    sc.keep(tl);
    return 0;
}

}  // namespace

extern "C" int mi_display_scaled(MiCtx *ctx, const MiPicture *in, const MiScaledImage *outs, int n_outs,
                                 const MiColorInfo *color, const MiFilmGrainData *fg, void *stream) {
    return display_scaled(ctx, in, outs, n_outs, color, nullptr, fg, stream);
}

extern "C" int mi_display_scaled_rs(MiCtx *ctx, const MiPicture *in, const MiScaledImage *outs, int n_outs,
                                    const MiColorInfo *color, const MiResample *rs, const MiFilmGrainData *fg, void *stream) {
    return display_scaled(ctx, in, outs, n_outs, color, rs, fg, stream);
}

extern "C" int mi_display_scaled_tm(MiCtx *ctx, const MiPicture *in, const MiScaledImage *outs, int n_outs,
                                    const MiColorInfo *color, const MiToneMap *tm, const MiYuvTarget *target,
                                    const MiResample *rs, const MiFilmGrainData *fg, void *stream) {
    const YuvTm yt = {tm, target};
    return display_scaled(ctx, in, outs, n_outs, color, rs, fg, stream, &yt);
}
