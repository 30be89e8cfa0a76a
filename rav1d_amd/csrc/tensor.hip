// tensor.hip — mi_display_tensor (include/mi_av1out.h): a shown picture as the cropped, resized,
// normalised R'G'B' tensor an ML consumer on the device reads, in one pass over the decoded planes.
// The picture is the one MI_OUT_RGB_PLANAR gives (display.h: the same loads, chroma upsampler and
// matrix); the resize is the separable 18-bit filter of resize.h (the triangle, or with
// mi_display_tensor_rs a cubic), both axes centred, horizontal pass first.
//
// Three launches on the caller's stream, all scratch in one context-owned allocation:
//   taps_kernel          (resize.h) the tap tables of the two axes; skipped when the context's
//                        scratch still holds them (the call before had this geometry);
//   tensor_h_kernel      one workgroup per (row unit, segment of output columns). A row unit is a
//                        luma row, or for 4:2:0 the row pair sharing a chroma row, as in
//                        display_kernel. A lane converts 8 source columns of the unit to R'G'B'
//                        once, into LDS (one 16-byte write per row and channel); then a lane owns
//                        (row, output column) items and filters the three channels from LDS into
//                        `mid`, crop_h x out_w u16 per channel. The segment is sized on the host so
//                        that the source columns its taps reach fit kTensorSeg. Rows outside the
//                        crop are not read (the upsampler still reads the chroma rows around it);
//   tensor_v_kernel      a lane owns 4 adjacent output columns of one output row: per tap one
//                        8-byte load of `mid` per channel (coalesced along x) and a wave-uniform
//                        weight, the sums in registers; then finish and store in the
//                        destination's order, as whole vectors where the pointer and strides allow.
//
// mi_display_tensor_tm: the colour-volume stage (display.h tone_run) runs in the tile fill of
// tensor_h_kernel, a compile-time switch (none, the table stage, the table stage with the HLG gain),
// so the passes resize the tone-mapped picture at dst_bpc.
// A cubic's taps are signed: CUBIC, a compile-time switch of both passes, clamps what the shift
// gives to [0, M]; the triangle's instantiations are the code they were without it.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>

#include <hip/hip_fp16.h>

#include "resize.h"

namespace mi {
namespace {

// 8 pixels of one row to R'G'B' (with TM: through the colour-volume stage, to samples of dst_bpc),
// one 16-byte LDS write per channel at column `col` of the tile
template <int TM>
__device__ __forceinline__ void tile_row(const DisplayArgs &a, const ToneParam<TM> &tm, const float *lin, const int (&y)[8],
                                         const int (&cu)[8], const int (&cv)[8], uint16_t (&tile)[3][kTensorSeg], int col) {
    int R[8], G[8], B[8];
    convert_run(a, y, cu, cv, R, G, B);
    if constexpr (TM) tone_run(tm, lin, R, G, B);
    *reinterpret_cast<uint4 *>(&tile[0][col]) = pack8(R);
    *reinterpret_cast<uint4 *>(&tile[1][col]) = pack8(G);
    *reinterpret_cast<uint4 *>(&tile[2][col]) = pack8(B);
}

// ---- horizontal pass ----
template <typename Px, int TM, bool CUBIC>
__global__ __launch_bounds__(256) void tensor_h_kernel(const TensorArgs t, const ToneParam<TM> tm) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[2][3][kTensorSeg];
    [[maybe_unused]] const float *lin = nullptr;
    if constexpr (TM) {
        __shared__ __attribute__((aligned(16))) float lut[tone_lds<ToneParam<TM>>()];
        tone_stage(tm, lut, threadIdx.x, 256);
        __syncthreads();
        lin = lut;
    }
    const DisplayArgs &a = t.d;
    const int u = t.u0 + blockIdx.x, nrows = 1 + a.ss_ver, r0 = u * nrows;
    const int o0 = blockIdx.y * t.ob, o1 = min(o0 + t.ob, t.ow) - 1;
    const int *hs = t.tab, *hc = hs + t.ow, *hk = hc + t.ow;
    // picture columns [lo, hi) the segment's taps read; the tile starts at the 8-column run of lo
    const int lo = t.cx + max(hs[o0], 0), hi = t.cx + min(hs[o1] + hc[o1], t.cw);
    const int xa = lo & ~7, x0 = xa + 8 * (int)threadIdx.x;
    // bit r: row r0 + r is a row of the crop
    const int rows = (int)(r0 >= t.cy && r0 < t.cy + t.ch) | (int)(nrows == 2 && r0 + 1 >= t.cy && r0 + 1 < t.cy + t.ch) << 1;
    if (x0 < hi && x0 - xa + 8 <= kTensorSeg) {
        int y[2][8] = {}, cu[2][8] = {}, cv[2][8] = {};
        if (rows & 1) load_run<Px, 8>(a.src[0] + r0 * a.sstride[0], x0, a.w, a.svec & 1, y[0]);
        if (rows & 2) load_run<Px, 8>(a.src[0] + (r0 + 1) * a.sstride[0], x0, a.w, a.svec & 1, y[1]);
        if (!a.mono) {
            upsample<Px>(a, 1, u, x0, cu);
            upsample<Px>(a, 2, u, x0, cv);
        }
        if (rows & 1) tile_row<TM>(a, tm, lin, y[0], cu[0], cv[0], tile[0], x0 - xa);
        if (rows & 2) tile_row<TM>(a, tm, lin, y[1], cu[1], cv[1], tile[1], x0 - xa);
    }
    __syncthreads();
    // a lane owns (row, output column) items and filters the three channels' samples
    const int nout = o1 - o0 + 1;
    for (int it = threadIdx.x; it < nout * 2; it += 256) {
        const int r = it >= nout, o = o0 + it - r * nout;
        if (!((rows >> r) & 1)) continue;
        const int base = hs[o] + t.cx - xa, lo_i = t.cx - xa, hi_i = min(t.cx - xa + t.cw - 1, kTensorSeg - 1);
        const int *k = hk + o;
        int acc[3] = {kTensorHalf, kTensorHalf, kTensorHalf};
#pragma unroll 4
        for (int j = 0; j < t.th; j++) h_tap<3>(tile[r], base + j, lo_i, hi_i, k[(int64_t)j * t.ow], acc);
        uint16_t *m = t.mid + (int64_t)(r0 + r - t.cy) * t.mstride + o;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            int v = acc[c] >> kTensorS;
            if constexpr (CUBIC) v = min(max(v, 0), (256 << t.shift) - 1);
            m[(int64_t)c * t.ch * t.mstride] = (uint16_t)v;
        }
    }
}

// ---- vertical pass, finish, store ----
template <int DT> struct Elem { using type = uint16_t; };
template <> struct Elem<MI_T_U8> { using type = uint8_t; };
template <> struct Elem<MI_T_F32> { using type = uint32_t; };

// fl32(fl32(v * s) + b): two separately rounded float32 operations. (__fmul_rn and __fadd_rn are a
// plain * and + in this toolchain's headers, which the default contraction fuses into one FMA; the
// pragma is what keeps the product rounded.)
__device__ __forceinline__ float scale_bias(float v, float s, float b) {
#pragma clang fp contract(off)
    const float p = v * s;
    return p + b;
}

template <int DT>
__device__ __forceinline__ typename Elem<DT>::type finish(const TensorArgs &t, int v, int c) {
    if constexpr (DT == MI_T_U8) {
        return (uint8_t)(t.shift ? min(255, (v + (1 << (t.shift - 1))) >> t.shift) : v);
    } else {
        const float f = scale_bias((float)v, t.scale[c], t.bias[c]);
        if constexpr (DT == MI_T_F32) {
            return __float_as_uint(f);
        } else if constexpr (DT == MI_T_F16) {
            return __half_as_ushort(__float2half_rn(f));
        } else {   // bfloat16: the float32 bits rounded to nearest-even (f is never a NaN)
            const uint32_t b = __float_as_uint(f);
            return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
        }
    }
}

// 4 adjacent elements as one store; p is aligned to 4 elements
template <typename E>
__device__ __forceinline__ void store4(uint8_t *p, const E (&e)[4]) {
    if constexpr (sizeof(E) == 1)
        *reinterpret_cast<uint32_t *>(p) = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) | ((uint32_t)e[3] << 24);
    else if constexpr (sizeof(E) == 2)
        *reinterpret_cast<uint2 *>(p) = make_uint2((uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16));
    else
        *reinterpret_cast<uint4 *>(p) = make_uint4(e[0], e[1], e[2], e[3]);
}

template <int DT, int ORDER, bool CUBIC>
__global__ __launch_bounds__(256) void tensor_v_kernel(const TensorArgs t) {
    using E = typename Elem<DT>::type;
    const int xb = blockIdx.x % t.xblocks, oy = blockIdx.x / t.xblocks;
    const int x0 = (xb * 256 + (int)threadIdx.x) * 4;
    if (x0 >= t.ow) return;
    const int *vs = t.tab + (int64_t)(t.th + 2) * t.ow, *vk = vs + 2 * t.oh;
    // (rows of mid are 16-byte aligned and x0 is a multiple of 4; columns past ow are padding)
    const int s = vs[oy];
    const uint16_t *m = t.mid + x0;
    const int64_t plane = (int64_t)t.ch * t.mstride;
    int acc[3][4];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[c][i] = kTensorHalf;
#pragma unroll 4
    for (int j = 0; j < t.tv; j++)
        v_tap<3>(m, plane, min(max(s + j, 0), t.ch - 1) * t.mstride, vk[(int64_t)j * t.oh + oy], acc);
    E e[3][4];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int v = acc[c][i] >> kTensorS;
            if constexpr (CUBIC) v = min(max(v, 0), (256 << t.shift) - 1);
            e[c][i] = finish<DT>(t, v, c);
        }
    const bool whole = t.vec && x0 + 4 <= t.ow;
    uint8_t *drow = t.dst + oy * t.dstride[1];
    if constexpr (ORDER == kTensorCHW) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            uint8_t *p = drow + c * t.dstride[0] + (int64_t)x0 * (int)sizeof(E);
            if (whole) {
                store4<E>(p, e[c]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (x0 + i < t.ow) reinterpret_cast<E *>(p)[i] = e[c][i];
            }
        }
    } else if constexpr (ORDER == kTensorHWC) {
        uint8_t *p = drow + (int64_t)x0 * 3 * (int)sizeof(E);
        E f[12];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int c = 0; c < 3; c++) f[3 * i + c] = e[c][i];
        if (whole) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const E g[4] = {f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
                store4<E>(p + 4 * q * (int)sizeof(E), g);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 12; i++)
                if (x0 + i / 3 < t.ow) reinterpret_cast<E *>(p)[i] = f[i];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x0 + i < t.ow) *reinterpret_cast<E *>(drow + c * t.dstride[0] + (x0 + i) * t.dstride[2]) = e[c][i];
    }
}

template <int DT, bool CUBIC>
void launch_v(const TensorArgs &t, int order, dim3 grid, hipStream_t s) {
    switch (order) {
    case kTensorCHW: tensor_v_kernel<DT, kTensorCHW, CUBIC><<<grid, 256, 0, s>>>(t); break;
    case kTensorHWC: tensor_v_kernel<DT, kTensorHWC, CUBIC><<<grid, 256, 0, s>>>(t); break;
    default: tensor_v_kernel<DT, kTensorAny, CUBIC><<<grid, 256, 0, s>>>(t); break;
    }
}

template <bool CUBIC>
int launch_passes(const TensorArgs &t, int bpc, int order, hipStream_t s, const ToneHlgArgs *tm) {
    const dim3 hgrid(t.units, t.segs);
    if (tm && tm->lut_gain) {
        if (bpc == 8)
            tensor_h_kernel<uint8_t, kToneHlg, CUBIC><<<hgrid, 256, 0, s>>>(t, *tm);
        else
            tensor_h_kernel<uint16_t, kToneHlg, CUBIC><<<hgrid, 256, 0, s>>>(t, *tm);
    } else if (tm) {
        if (bpc == 8)
            tensor_h_kernel<uint8_t, kToneTable, CUBIC><<<hgrid, 256, 0, s>>>(t, *tm);
        else
            tensor_h_kernel<uint16_t, kToneTable, CUBIC><<<hgrid, 256, 0, s>>>(t, *tm);
    } else if (bpc == 8) {
        tensor_h_kernel<uint8_t, kToneNone, CUBIC><<<hgrid, 256, 0, s>>>(t, NoTone());
    } else {
        tensor_h_kernel<uint16_t, kToneNone, CUBIC><<<hgrid, 256, 0, s>>>(t, NoTone());
    }
    if (hipGetLastError() != hipSuccess) return -1;
    const dim3 vgrid((unsigned)t.xblocks * (unsigned)t.oh);
    switch (t.dtype) {
    case MI_T_U8: launch_v<MI_T_U8, CUBIC>(t, order, vgrid, s); break;
    case MI_T_F16: launch_v<MI_T_F16, CUBIC>(t, order, vgrid, s); break;
    case MI_T_BF16: launch_v<MI_T_BF16, CUBIC>(t, order, vgrid, s); break;
    default: launch_v<MI_T_F32, CUBIC>(t, order, vgrid, s); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

int launch_tensor(const TensorArgs &t, int bpc, int order, hipStream_t s, const ToneHlgArgs *tm, bool cubic) {
    return cubic ? launch_passes<true>(t, bpc, order, s, tm) : launch_passes<false>(t, bpc, order, s, tm);
}

}  // namespace mi

namespace {

// mi_display_tensor (tone false; tm not read), mi_display_tensor_tm (tone true) and, with a
// filter, mi_display_tensor_rs
int display_tensor(MiCtx *ctx, const MiPicture *in, const MiTensorImage *out, const MiColorInfo *color, bool tone,
                   const MiToneMap *tm, const MiResample *rs, const MiFilmGrainData *fg, void *stream) {
    if (!in || !out) return -EINVAL;
    if (int e = mi::display_check_picture(in)) return e;
    if (int e = mi::display_check_strides(in)) return e;
    const int ss_ver = in->layout == 1;
    // destination
    if (!out->data || out->w < 1 || out->h < 1 || out->w > 65536 || out->h > 65536) return -EINVAL;
    if (out->dtype != MI_T_U8 && out->dtype != MI_T_F16 && out->dtype != MI_T_BF16 && out->dtype != MI_T_F32)
        return -EINVAL;
    const ptrdiff_t es = out->dtype == MI_T_U8 ? 1 : out->dtype == MI_T_F32 ? 4 : 2;
    for (int i = 0; i < 3; i++)
        if (out->stride[i] <= 0 || out->stride[i] % es) return -EINVAL;
    if ((uintptr_t)out->data % (uintptr_t)es) return -EINVAL;
    int cx, cy, cw, ch;
    if (int e = mi::display_crop(in, out->crop_x, out->crop_y, out->crop_w, out->crop_h, cx, cy, cw, ch)) return e;
    if ((int64_t)cw > 64 * (int64_t)out->w || (int64_t)ch > 64 * (int64_t)out->h) return -EINVAL;
    if (out->dtype != MI_T_U8)
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(out->scale[c]) || !std::isfinite(out->bias[c])) return -EINVAL;

    mi::Filter flt;
    if (int e = mi::resample_check(rs, flt)) return e;

    mi::TensorArgs t;
    memset(&t, 0, sizeof(t));
    if (int e = mi::display_color(in, color, t.d)) return e;
    if (tone)
        if (int e = mi::tone_check(tm, color, ctx && ctx->hlg)) return e;
    if (!ctx) return -EINVAL;

    // geometry of the passes and of the scratch
    const int ow = out->w, oh = out->h;
    t.cx = cx, t.cy = cy, t.cw = cw, t.ch = ch, t.ow = ow, t.oh = oh;
    const int radius = mi::filter_radius(flt);
    t.th = mi::tap_cap(cw, ow, radius);
    t.tv = mi::tap_cap(ch, oh, radius);
    t.mstride = ((int64_t)ow + 7) & ~(int64_t)7;
    t.ob = mi::seg_outputs(cw, ow, radius);
    t.segs = (ow + t.ob - 1) / t.ob;
    t.u0 = cy >> ss_ver;
    t.units = ((cy + ch - 1) >> ss_ver) - t.u0 + 1;
    t.xblocks = (ow + 1023) / 1024;
    const size_t tab_bytes = (((size_t)(t.th + 2) * ow + (size_t)(t.tv + 2) * oh) * sizeof(int) + 255) & ~(size_t)255;
    const size_t mid_bytes = (size_t)3 * ch * t.mstride * sizeof(uint16_t);

    // allocations first: a call that fails has launched nothing
    MiResizeScratch &sc = ctx->tens;
    if (!sc.ensure(tab_bytes + mid_bytes)) return ctx->last_error = -ENOMEM;
    t.tab = (int *)sc.p;
    t.mid = (uint16_t *)(sc.p + tab_bytes);
    mi::TapList tl;
    memset(&tl, 0, sizeof(tl));
    tl.ax[tl.n++] = mi::TapAxis{cw, ow, 2, t.th, t.tab};
    tl.ax[tl.n++] = mi::TapAxis{ch, oh, 2, t.tv, t.tab + (int64_t)(t.th + 2) * ow};
    mi::tap_filter(tl, flt);
    const bool taps = !sc.holds(tl);
    mi::ToneHlgArgs ta;
    if (tone)
        if (int e = mi::tone_prepare(ctx, tm, color, in->bpc, (hipStream_t)stream, ta)) return e;
    MiPicture src = *in;
    if (fg)
        if (int e = mi::display_grain(ctx, in, &src, fg, color, stream)) return e;

    mi::display_source(src, color, t.d);
    t.dst = (uint8_t *)out->data;
    for (int i = 0; i < 3; i++) t.dstride[i] = out->stride[i];
    t.dtype = out->dtype;
    t.shift = (tone ? tm->dst_bpc : in->bpc) - 8;   // the picture the passes resize has this depth
    for (int c = 0; c < 3; c++) t.scale[c] = out->scale[c], t.bias[c] = out->bias[c];
    // the two fast orders, and whether every run of 4 elements is an aligned vector
    int order = mi::kTensorAny;
    const uintptr_t v4 = (uintptr_t)(4 * es - 1);
    if (out->stride[2] == es) {
        order = mi::kTensorCHW;
        t.vec = !(((uintptr_t)out->data | (uintptr_t)out->stride[0] | (uintptr_t)out->stride[1]) & v4);
    } else if (out->stride[0] == es && out->stride[2] == 3 * es) {
        order = mi::kTensorHWC;
        t.vec = !(((uintptr_t)out->data | (uintptr_t)out->stride[1]) & v4);
    }
    sc.forget();
    if ((taps && mi::launch_taps(tl, (hipStream_t)stream)) ||
        mi::launch_tensor(t, in->bpc, order, (hipStream_t)stream, tone ? &ta : nullptr, flt.filter == MI_RS_CUBIC))
        return ctx->last_error = -EIO;
    sc.keep(tl);
    return 0;
}

}  // namespace

extern "C" int mi_display_tensor(MiCtx *ctx, const MiPicture *in, const MiTensorImage *out, const MiColorInfo *color,
                                 const MiFilmGrainData *fg, void *stream) {
    return display_tensor(ctx, in, out, color, false, nullptr, nullptr, fg, stream);
}

extern "C" int mi_display_tensor_tm(MiCtx *ctx, const MiPicture *in, const MiTensorImage *out, const MiColorInfo *color,
                                    const MiToneMap *tm, const MiFilmGrainData *fg, void *stream) {
    return display_tensor(ctx, in, out, color, true, tm, nullptr, fg, stream);
}

extern "C" int mi_display_tensor_rs(MiCtx *ctx, const MiPicture *in, const MiTensorImage *out, const MiColorInfo *color,
                                    const MiToneMap *tm, const MiResample *rs, const MiFilmGrainData *fg, void *stream) {
    return display_tensor(ctx, in, out, color, tm != nullptr, tm, rs, fg, stream);
}
