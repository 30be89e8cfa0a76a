// display.hip — mi_display_picture (include/mi_av1out.h): a shown picture for a consumer on the
// device. The decoder's pictures are planar in the 128-aligned allocator geometry and carry no
// film grain; this pass writes the visible w x h tight into the caller's memory as semi-planar
// YUV (NV12 / P010 and their 4:2:2 / 4:4:4 kin) or as R'G'B' (planar, or packed with alpha),
// after mi_film_grain_frame when the frame has grain.
//
// display_kernel is a pure streaming pass (4:2:0: 1.5 W H B read, 3 or 4 W H B written). One lane
// owns 8 luma columns of one row unit: one luma row, or for 4:2:0 the row pair 2j, 2j+1 that
// shares chroma row j, so the chroma rows j-1, j, j+1 the pair interpolates from are loaded once
// into registers (4 samples and one halo sample each) and serve both rows. Loads and stores are
// one vector per run (8 B for 8 u8 samples, 16 B otherwise) where the plane's pointer and stride
// are 16-byte aligned and the run lies inside the row; any other run is done sample by sample
// with clamped source columns. Packed RGBA, whose runs are 2 or 4 vectors long, goes through a
// per-wave LDS hand-off so that a store instruction writes 1 KB contiguously (rgb_row).
//
// mi_display_picture_tm is the same kernel with the colour-volume stage (display.h tone_run: two
// table gathers per channel around a 3 x 3 float32 matrix) between the matrix and the store, a
// compile-time switch; its destination samples have the type of dst_bpc, not the source's. The
// instantiations without the stage are the code they were before it existed, and those with it the
// code they were before the third mode, HLG sources (the OOTF gain between lut_in and the matrix).
#include <cerrno>
#include <cmath>
#include <cstring>

#include "display.h"

namespace mi {
namespace {

// 8 pixels of luma row `row` to R'G'B' samples of type Px (the destination's: the source's own
// type, or with the colour-volume stage TM the type of dst_bpc)
template <typename Px, int FMT, int TM>
__device__ __forceinline__ void rgb_row(const DisplayArgs &a, const ToneParam<TM> &tm, const float *lin, int row, int x0,
                                        const int (&y)[8], const int (&cu)[8], const int (&cv)[8]) {
    int R[8], G[8], B[8];
    convert_run(a, y, cu, cv, R, G, B);
    int alpha = a.maxv;
    if constexpr (TM) {
        tone_run(tm, lin, R, G, B);
        alpha = tm.maxd;
    }
    if constexpr (FMT == MI_OUT_RGB_PLANAR) {
        store_run<Px, 8>(a.dst[0] + row * a.dstride[0], x0, a.w, a.dvec & 1, R);
        store_run<Px, 8>(a.dst[1] + row * a.dstride[1], x0, a.w, (a.dvec >> 1) & 1, G);
        store_run<Px, 8>(a.dst[2] + row * a.dstride[2], x0, a.w, (a.dvec >> 2) & 1, B);
    } else {
        int o[32];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            o[4 * k] = R[k];
            o[4 * k + 1] = G[k];
            o[4 * k + 2] = B[k];
            o[4 * k + 3] = alpha;
        }
        uint8_t *drow = a.dst[0] + row * a.dstride[0];
        // A lane's run is 32 samples (2 or 4 16-B vectors), so lane-owned stores would put each
        // store instruction's 64 vectors 32 or 64 B apart. Where the wave's 64 runs all lie inside
        // the row of an aligned plane (wave-uniform: a wave is one row unit's 512 columns), the
        // wave hands its runs through LDS and consecutive lanes store consecutive vectors.
        constexpr int kVec = 32 * (int)sizeof(Px) / 16;
        const int xw = x0 - 8 * (int)threadIdx.x;   // the wave's first column
        if ((a.dvec & 1) && xw + 512 <= a.w) {
            __shared__ uint4 tile[4][64 * kVec];
            uint4 *t = tile[threadIdx.y];
#pragma unroll
            for (int i = 0; i < kVec; i++) {
                uint32_t q[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int k = 4 * i + j;   // 32-bit word k of the run
                    if constexpr (sizeof(Px) == 1)
                        q[j] = (uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 8) | ((uint32_t)o[4 * k + 2] << 16) |
                               ((uint32_t)o[4 * k + 3] << 24);
                    else
                        q[j] = (uint32_t)o[2 * k] | ((uint32_t)o[2 * k + 1] << 16);
                }
                t[threadIdx.x * kVec + i] = make_uint4(q[0], q[1], q[2], q[3]);
            }
            // the wave's own LDS traffic is ordered; keep the compiler from moving it
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            uint4 *d = reinterpret_cast<uint4 *>(drow + (int64_t)xw * 4 * (int)sizeof(Px));
#pragma unroll
            for (int i = 0; i < kVec; i++) d[i * 64 + threadIdx.x] = t[i * 64 + threadIdx.x];
            // (the next row's hand-off rewrites the tile)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else {
            store_run<Px, 32>(drow, 4 * x0, 4 * a.w, a.dvec & 1, o);
        }
    }
}

// Px: the source samples; Dx: the destination samples (Px unless TM); TM: the colour-volume
// stage after the matrix (RGB formats): kToneNone, kToneTable, or kToneHlg with the HLG gain
template <typename Px, typename Dx, int FMT, int TM>
__global__ __launch_bounds__(256) void display_kernel(const DisplayArgs a, const ToneParam<TM> tm) {
    [[maybe_unused]] const float *lin = nullptr;
    if constexpr (TM) {   // (before any lane leaves: every lane fills the table and meets the barrier)
        __shared__ __attribute__((aligned(16))) float lut[tone_lds<ToneParam<TM>>()];
        tone_stage(tm, lut, threadIdx.y * 64 + threadIdx.x, 256);
        __syncthreads();
        lin = lut;
    }
    const int cx = blockIdx.x * 64 + threadIdx.x, u = blockIdx.y * 4 + threadIdx.y;
    if (cx >= a.chunks || u >= a.units) return;
    const int x0 = cx * 8, nrows = 1 + a.ss_ver, r0 = u * nrows;
    int y[2][8];
    load_run<Px, 8>(a.src[0] + r0 * a.sstride[0], x0, a.w, a.svec & 1, y[0]);
    if (a.ss_ver) {
        load_run<Px, 8>(a.src[0] + min(r0 + 1, a.h - 1) * a.sstride[0], x0, a.w, a.svec & 1, y[1]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) y[1][k] = y[0][k];   // (not used)
    }

    if constexpr (FMT == MI_OUT_SEMIPLANAR) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            if (r < nrows && r0 + r < a.h) {
                int o[8];
#pragma unroll
                for (int k = 0; k < 8; k++) o[k] = y[r][k] << a.shift;
                store_run<Px, 8>(a.dst[0] + (int64_t)(r0 + r) * a.dstride[0], x0, a.w, a.dvec & 1, o);
            }
        }
        if (a.mono) return;
        // chroma row u (the row unit is a chroma row for 4:2:0, a luma row otherwise)
        uint8_t *drow = a.dst[1] + u * a.dstride[1];
        const uint8_t *urow = a.src[1] + u * a.sstride[1], *vrow = a.src[2] + u * a.sstride[1];
        if (a.ss_hor) {
            int cu[4], cv[4], o[8];
            load_run<Px, 4>(urow, x0 >> 1, a.cw, (a.svec >> 1) & 1, cu);
            load_run<Px, 4>(vrow, x0 >> 1, a.cw, (a.svec >> 2) & 1, cv);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                o[2 * k] = cu[k] << a.shift;
                o[2 * k + 1] = cv[k] << a.shift;
            }
            store_run<Px, 8>(drow, x0, 2 * a.cw, (a.dvec >> 1) & 1, o);
        } else {
            int cu[8], cv[8], o[16];
            load_run<Px, 8>(urow, x0, a.cw, (a.svec >> 1) & 1, cu);
            load_run<Px, 8>(vrow, x0, a.cw, (a.svec >> 2) & 1, cv);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                o[2 * k] = cu[k] << a.shift;
                o[2 * k + 1] = cv[k] << a.shift;
            }
            store_run<Px, 16>(drow, 2 * x0, 2 * a.cw, (a.dvec >> 1) & 1, o);
        }
    } else {
        int cu[2][8] = {}, cv[2][8] = {};
        if (!a.mono) {
            upsample<Px>(a, 1, u, x0, cu);
            upsample<Px>(a, 2, u, x0, cv);
        }
        rgb_row<Dx, FMT, TM>(a, tm, lin, r0, x0, y[0], cu[0], cv[0]);
        if (a.ss_ver && r0 + 1 < a.h) rgb_row<Dx, FMT, TM>(a, tm, lin, r0 + 1, x0, y[1], cu[1], cv[1]);
    }
}

template <typename Px>
int launch_px(const DisplayArgs &a, int format, hipStream_t s) {
    const dim3 block(64, 4), grid((a.chunks + 63) / 64, (a.units + 3) / 4);
    switch (format) {
    case MI_OUT_SEMIPLANAR: display_kernel<Px, Px, MI_OUT_SEMIPLANAR, kToneNone><<<grid, block, 0, s>>>(a, NoTone()); break;
    case MI_OUT_RGB_PLANAR: display_kernel<Px, Px, MI_OUT_RGB_PLANAR, kToneNone><<<grid, block, 0, s>>>(a, NoTone()); break;
    default: display_kernel<Px, Px, MI_OUT_RGBA_PACKED, kToneNone><<<grid, block, 0, s>>>(a, NoTone()); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <typename Px, typename Dx, int TM>
int launch_tm(const DisplayArgs &a, const ToneParam<TM> &tm, int format, hipStream_t s) {
    const dim3 block(64, 4), grid((a.chunks + 63) / 64, (a.units + 3) / 4);
    if (format == MI_OUT_RGB_PLANAR)
        display_kernel<Px, Dx, MI_OUT_RGB_PLANAR, TM><<<grid, block, 0, s>>>(a, tm);
    else
        display_kernel<Px, Dx, MI_OUT_RGBA_PACKED, TM><<<grid, block, 0, s>>>(a, tm);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int TM>
int launch_tm_px(const DisplayArgs &a, const ToneParam<TM> &tm, int bpc, int dst_bpc, int format, hipStream_t s) {
    if (bpc == 8)
        return dst_bpc == 8 ? launch_tm<uint8_t, uint8_t, TM>(a, tm, format, s) : launch_tm<uint8_t, uint16_t, TM>(a, tm, format, s);
    return dst_bpc == 8 ? launch_tm<uint16_t, uint8_t, TM>(a, tm, format, s) : launch_tm<uint16_t, uint16_t, TM>(a, tm, format, s);
}

}  // namespace

int launch_display(const DisplayArgs &a, int bpc, int format, hipStream_t s) {
    return bpc == 8 ? launch_px<uint8_t>(a, format, s) : launch_px<uint16_t>(a, format, s);
}

int launch_display_tm(const DisplayArgs &a, const ToneHlgArgs &tm, int bpc, int dst_bpc, int format, hipStream_t s) {
    return tm.lut_gain ? launch_tm_px<kToneHlg>(a, tm, bpc, dst_bpc, format, s)
                       : launch_tm_px<kToneTable>(a, tm, bpc, dst_bpc, format, s);
}


// (Kr, Kb) of Dav1dMatrixCoefficients: 0 supported, -ENOTSUP (a matrix that is no Kr / Kb
// matrix: YCgCo, BT.2020 constant luminance, SMPTE 2085, chromaticity-derived, ICtCp) or -EINVAL
int matrix_k(int mtrx, double *kr, double *kb) {
    switch (mtrx) {
    case 1: *kr = 0.2126; *kb = 0.0722; return 0;    // BT.709
    case 4: *kr = 0.30; *kb = 0.11; return 0;        // FCC
    case 5:                                          // BT.470BG
    case 6: *kr = 0.299; *kb = 0.114; return 0;      // BT.601
    case 7: *kr = 0.212; *kb = 0.087; return 0;      // SMPTE 240
    case 9: *kr = 0.2627; *kb = 0.0593; return 0;    // BT.2020 non-constant luminance
    case 8: case 10: case 11: case 12: case 13: case 14: return -ENOTSUP;
    default: return -EINVAL;
    }
}

int round_fix(double v) { return (int)floor(v * (double)(1 << kDispS) + 0.5); }

int display_check_picture(const MiPicture *in) {
    if (!in->data[0] || in->w <= 0 || in->h <= 0 || in->w > 65536 || in->h > 65536 || in->layout < 0 || in->layout > 3 ||
        (in->bpc != 8 && in->bpc != 10 && in->bpc != 12) || in->stride[0] <= 0)
        return -EINVAL;
    if (in->layout && (!in->data[1] || !in->data[2] || in->stride[1] <= 0)) return -EINVAL;
    return 0;
}

int display_check_strides(const MiPicture *in) {
    const int pxb = in->bpc == 8 ? 1 : 2, ss_hor = in->layout == 1 || in->layout == 2;
    if ((int64_t)in->stride[0] < (int64_t)in->w * pxb ||
        (in->layout && (int64_t)in->stride[1] < (int64_t)((in->w + ss_hor) >> ss_hor) * pxb))
        return -EINVAL;
    return 0;
}

int display_crop(const MiPicture *in, int crop_x, int crop_y, int crop_w, int crop_h, int &cx, int &cy, int &cw, int &ch) {
    cx = 0, cy = 0, cw = in->w, ch = in->h;
    if (crop_w || crop_h) {
        cx = crop_x, cy = crop_y, cw = crop_w, ch = crop_h;
        if (cx < 0 || cy < 0 || cw < 1 || ch < 1 || (int64_t)cx + cw > in->w || (int64_t)cy + ch > in->h) return -EINVAL;
    }
    return 0;
}

int display_color(const MiPicture *in, const MiColorInfo *color, DisplayArgs &a) {
    if (!color || color->mtrx == 2 || (color->range != 0 && color->range != 1)) return -EINVAL;
    if (color->mtrx == 0) {
        if (in->layout != 3) return -EINVAL;
        a.identity = 1;
        return 0;
    }
    double kr, kb;
    if (int e = matrix_k(color->mtrx, &kr, &kb)) return e;
    const int b = in->bpc;
    const double m = (double)((1 << b) - 1), kg = 1.0 - kr - kb;
    const double kc = color->range ? 1.0 : m / (double)(224 << (b - 8));
    a.yo = color->range ? 0 : 16 << (b - 8);
    a.ky = color->range ? 1 << kDispS : round_fix(m / (double)(219 << (b - 8)));
    a.crv = round_fix(2.0 * (1.0 - kr) * kc);
    a.cbu = round_fix(2.0 * (1.0 - kb) * kc);
    a.cgu = round_fix(2.0 * kb * (1.0 - kb) / kg * kc);
    a.cgv = round_fix(2.0 * kr * (1.0 - kr) / kg * kc);
    return 0;
}

int display_grain(MiCtx *ctx, const MiPicture *in, MiPicture *src, const MiFilmGrainData *fg, const MiColorInfo *color,
                  void *stream) {
    // the grained picture, in the geometry of `in`
    const int ss_ver = in->layout == 1;
    const size_t ah = ((size_t)in->h + 127) & ~(size_t)127;
    const size_t ybytes = ((size_t)in->stride[0] * ah + 255) & ~(size_t)255;
    const size_t cbytes = in->layout ? ((size_t)in->stride[1] * (ah >> ss_ver) + 255) & ~(size_t)255 : 0;
    if (ybytes + 2 * cbytes > ctx->disp_fg_bytes) {
        if (ctx->disp_fg) (void)hipFree(ctx->disp_fg);   // (waits for the work that reads it)
        ctx->disp_fg = nullptr;
        ctx->disp_fg_bytes = 0;
        if (hipMalloc(&ctx->disp_fg, ybytes + 2 * cbytes) != hipSuccess) return ctx->last_error = -ENOMEM;
        ctx->disp_fg_bytes = ybytes + 2 * cbytes;
    }
    src->data[0] = ctx->disp_fg;
    src->data[1] = in->layout ? ctx->disp_fg + ybytes : nullptr;
    src->data[2] = in->layout ? ctx->disp_fg + ybytes + cbytes : nullptr;
    return mi_film_grain_frame(ctx, in, src, fg, color && color->mtrx == 0, stream);
}

void display_source(const MiPicture &src, const MiColorInfo *color, DisplayArgs &a) {
    const int ss_hor = src.layout == 1 || src.layout == 2, ss_ver = src.layout == 1;
    for (int p = 0; p < (src.layout ? 3 : 1); p++) {
        a.src[p] = (const uint8_t *)src.data[p];
        if (aligned_to(src.data[p], src.stride[p ? 1 : 0], 16)) a.svec |= 1 << p;
    }
    a.sstride[0] = src.stride[0];
    a.sstride[1] = src.stride[1];
    a.w = src.w;
    a.h = src.h;
    a.cw = (src.w + ss_hor) >> ss_hor;
    a.ch = (src.h + ss_ver) >> ss_ver;
    a.ss_hor = ss_hor;
    a.ss_ver = ss_ver;
    a.mono = src.layout == 0;
    a.coloc = color && color->chr == 2;
    a.half = 1 << (src.bpc - 1);
    a.maxv = (1 << src.bpc) - 1;
}

}  // namespace mi

namespace {

// mi_display_picture (tone false; tm not read) and mi_display_picture_tm (tone true)
int display_picture(MiCtx *ctx, const MiPicture *in, const MiDisplayImage *out, const MiColorInfo *color, bool tone,
                    const MiToneMap *tm, const MiFilmGrainData *fg, void *stream) {
    if (!in || !out) return -EINVAL;
    if (int e = mi::display_check_picture(in)) return e;
    if (out->w != in->w || out->h != in->h) return -EINVAL;
    // the output depth: the source's, or with the colour-volume stage dst_bpc (checked below)
    if (tone ? out->bpc != 8 && out->bpc != 10 && out->bpc != 12 : out->bpc != in->bpc) return -EINVAL;
    if (out->format != MI_OUT_SEMIPLANAR && out->format != MI_OUT_RGB_PLANAR && out->format != MI_OUT_RGBA_PACKED)
        return -EINVAL;
    if (tone && out->format == MI_OUT_SEMIPLANAR) return -ENOTSUP;
    const int ss_hor = in->layout == 1 || in->layout == 2, ss_ver = in->layout == 1;
    const int dpxb = out->bpc == 8 ? 1 : 2;   // bytes of a destination sample
    const int cw = (in->w + ss_hor) >> ss_hor, ch = (in->h + ss_ver) >> ss_ver;
    // destination planes and the samples a row of each holds
    const int ndst = out->format == MI_OUT_RGB_PLANAR ? 3 : out->format == MI_OUT_SEMIPLANAR && in->layout ? 2 : 1;
    for (int p = 0; p < ndst; p++) {
        const int64_t samples = out->format == MI_OUT_RGBA_PACKED ? 4 * (int64_t)in->w
                              : out->format == MI_OUT_SEMIPLANAR && p ? 2 * (int64_t)cw : in->w;
        if (!out->data[p] || out->stride[p] < samples * dpxb) return -EINVAL;
        if (((uintptr_t)out->data[p] | (uintptr_t)out->stride[p]) & (uintptr_t)(dpxb - 1)) return -EINVAL;
    }
    if (int e = mi::display_check_strides(in)) return e;

    mi::DisplayArgs a;
    memset(&a, 0, sizeof(a));
    if (out->format != MI_OUT_SEMIPLANAR)
        if (int e = mi::display_color(in, color, a)) return e;
    if (tone) {
        if (int e = mi::tone_check(tm, color, ctx && ctx->hlg)) return e;
        if (out->bpc != tm->dst_bpc) return -EINVAL;
    }
    if (!ctx) return -EINVAL;

    // allocations and the table upload first: a call that fails there has launched nothing
    mi::ToneHlgArgs ta;
    if (tone)
        if (int e = mi::tone_prepare(ctx, tm, color, in->bpc, (hipStream_t)stream, ta)) return e;
    MiPicture src = *in;
    if (fg)
        if (int e = mi::display_grain(ctx, in, &src, fg, color, stream)) return e;

    mi::display_source(src, color, a);
    for (int p = 0; p < ndst; p++) {
        a.dst[p] = (uint8_t *)out->data[p];
        a.dstride[p] = out->stride[p];
        if (mi::aligned_to(out->data[p], out->stride[p], 16)) a.dvec |= 1 << p;
    }
    a.shift = out->format == MI_OUT_SEMIPLANAR && in->bpc > 8 ? 16 - in->bpc : 0;
    a.chunks = (in->w + 7) >> 3;
    a.units = ss_ver ? ch : in->h;
    if (tone ? mi::launch_display_tm(a, ta, in->bpc, out->bpc, out->format, (hipStream_t)stream)
             : mi::launch_display(a, in->bpc, out->format, (hipStream_t)stream))
        return ctx->last_error = -EIO;
    return 0;
}

}  // namespace

extern "C" int mi_display_picture(MiCtx *ctx, const MiPicture *in, const MiDisplayImage *out, const MiColorInfo *color,
                                  const MiFilmGrainData *fg, void *stream) {
    return display_picture(ctx, in, out, color, false, nullptr, fg, stream);
}

extern "C" int mi_display_picture_tm(MiCtx *ctx, const MiPicture *in, const MiDisplayImage *out, const MiColorInfo *color,
                                     const MiToneMap *tm, const MiFilmGrainData *fg, void *stream) {
    return display_picture(ctx, in, out, color, true, tm, fg, stream);
}
