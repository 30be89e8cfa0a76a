// display.h — what the device outputs share. All of them (display.hip mi_display_picture,
// tensor.hip mi_display_tensor, scaled.hip mi_display_scaled): the checks of the source picture
// and of a crop, the film-grain step, vector loads and stores of a plane run. The R'G'B' outputs
// (mi_display_picture, mi_display_tensor) and the tone-mapped YUV outputs that continue from their
// picture (yuv_tm.hip mi_display_yuv_tm, mi_display_scaled_tm): the host side of the conversion (colour checks and
// 14-bit coefficients, the source half of DisplayArgs) and its device side (the integer chroma
// upsampler, the matrix, the colour-volume stage), so both compute the same picture. The resize of
// the tensor and scaled outputs is resize.h.
#pragma once
#include <type_traits>

#include "mi_av1out.h"
#include "ctx.h"

namespace mi {

constexpr int kDispS = 14;   // fixed-point fraction bits of the matrix

// ---- host (display.hip) ----
// The source picture `in` (not NULL): plane pointers, extents in 1..65536, layout, bpc, strides
// present (display_check_picture), and strides that hold a row (display_check_strides; after the
// former). 0 or -EINVAL.
int display_check_picture(const MiPicture *in);
int display_check_strides(const MiPicture *in);
// The crop rectangle of an output in luma pixels: the whole picture when crop_w and crop_h are
// both 0, else the rectangle, which must lie inside the picture. 0 or -EINVAL.
int display_crop(const MiPicture *in, int crop_x, int crop_y, int crop_w, int crop_h, int &cx, int &cy, int &cw, int &ch);
// The film-grain step of a call with grain: points `src` (a copy of `in`) at the context's
// grained scratch picture in the geometry of `in`, allocating or growing it (-ENOMEM with
// last_error set; nothing launched), then mi_film_grain_frame into it on `stream` (its errors).
// `color` may be NULL.
int display_grain(MiCtx *ctx, const MiPicture *in, MiPicture *src, const MiFilmGrainData *fg, const MiColorInfo *color,
                  void *stream);
inline bool aligned_to(const void *p, ptrdiff_t stride, uintptr_t n) { return (((uintptr_t)p | (uintptr_t)stride) & (n - 1)) == 0; }
// The colour rules of the RGB formats: -EINVAL for NULL `color`, mtrx 2 or reserved, a range that
// is not 0 / 1, identity without 4:4:4; -ENOTSUP for matrices 8 and 10-14; else 0 with a.identity
// or a.yo / a.ky / a.crv / a.cbu / a.cgu / a.cgv set. No device work.
int display_color(const MiPicture *in, const MiColorInfo *color, DisplayArgs &a);
// (Kr, Kb) of a Dav1dMatrixCoefficients value, the one table of both directions of the matrix: 0,
// -ENOTSUP (defined, but no Kr / Kb matrix: 8, 10-14) or -EINVAL (0, 2, reserved)
int matrix_k(int mtrx, double *kr, double *kb);
// v in 14-bit fixed point, rounded to nearest
int round_fix(double v);
// The source half of DisplayArgs: planes, strides, vector-load flags, sizes, siting, H and M.
void display_source(const MiPicture &src, const MiColorInfo *color, DisplayArgs &a);

// ---- host (tonemap.cpp) ----
// The rules of the colour-volume stage for `tm` and the source description in `color` (not NULL):
// 0, -EINVAL or -ENOTSUP as include/mi_av1out.h lists them; `hlg`: trc 18 is a source (the flag of
// the context, mi_ctx_enable_hlg; false without one). No device work.
int tone_check(const MiToneMap *tm, const MiColorInfo *color, bool hlg);
// The context's device tables for (tm, color, src_bpc), all checked before: built and uploaded on
// `s` when they differ from the ones it holds. 0, -ENOMEM or -EIO (with last_error set).
// t.lut_gain is nullptr unless the source is HLG.
int tone_prepare(MiCtx *ctx, const MiToneMap *tm, const MiColorInfo *color, int src_bpc, hipStream_t s, ToneHlgArgs &t);

// ---- host (yuv_tm.hip) ----
// The rules of the tone-mapped YUV outputs beyond their plain entries': -EINVAL for NULL `tm` or
// `target`, the colour rules of the RGB formats (display_color) and of the stage (tone_check), then
// -EINVAL for a target matrix that is no Kr / Kb matrix or a range that is not 0 / 1; else 0 with
// the inverse matrix in `a` and the forward coefficients in `f`; `hlg` as for tone_check. No device work.
int yuv_tm_check(const MiPicture *in, const MiColorInfo *color, const MiToneMap *tm, const MiYuvTarget *target,
                 bool hlg, DisplayArgs &a, YuvArgs &f);
// The context's scratch picture for Q of `in` at dst_bpc in *q (planar, 128-byte aligned rows),
// allocated or grown: 0 or -ENOMEM (with last_error set). Nothing launched.
int yuv_tm_scratch(MiCtx *ctx, const MiPicture *in, int dst_bpc, MiPicture *q);
// Enqueue Q of `src` (the source, grained where the call has grain) on `s`: into the planes of `q`
// (planar) or into dst[0] = Y and dst[1] = interleaved UV with the strides given (q NULL). `a` and
// `f` from yuv_tm_check, `tm` from tone_prepare. 0 or -1.
int yuv_tm_picture(const MiPicture &src, const MiColorInfo *color, DisplayArgs a, const ToneHlgArgs &tm, const YuvArgs &f,
                   const MiPicture *q, void *const dst[2], const ptrdiff_t dstride[2], int dst_bpc, hipStream_t s);

// ---- device ----

// The stage reads lut_in from the workgroup's copy in LDS and lut_out (128 KB) from global memory.
// lut_in was measured both ways (the colour-volume stage): from LDS the calls take
// 0.74 - 0.80 of the time they take with lut_in in global memory at 10 bits, 0.69 - 0.74 at 12.
constexpr int kToneIn = 4096;   // entries of lut_in at 12 bits

// the workgroup's copy of lut_in: every thread calls it, a barrier follows
__device__ __forceinline__ void tone_stage(const ToneArgs &tm, float *lds, int tid, int nthreads) {
    for (int i = 4 * tid; i < tm.n_in; i += 4 * nthreads)
        *reinterpret_cast<float4 *>(lds + i) = *reinterpret_cast<const float4 *>(tm.lut_in + i);
}

// The HLG stage (Tone = ToneHlgArgs) reads lut_gain (6152 B) from the workgroup's copy in LDS too,
// behind lut_in in one array; kHlgGainLds false reads it from global memory like lut_out (the switch
// the two were timed with: DESIGN.md, HLG sources: from LDS the HLG calls take 0.92 - 0.98 of the
// time they take with lut_gain in global memory, 4K10).
#ifndef MI_HLG_GAIN_GLOBAL
constexpr bool kHlgGainLds = true;
#else
constexpr bool kHlgGainLds = false;
#endif
constexpr int kToneGainPad = (kToneGain + 3) & ~3;   // whole float4s: the device table is padded to it
// floats of the workgroup's table array
template <typename Tone> constexpr int tone_lds() {
    return kToneIn + (std::is_same_v<Tone, ToneHlgArgs> && kHlgGainLds ? kToneGainPad : 0);
}
// the HLG workgroup's copy of lut_gain at lds + kToneIn: every thread calls it, before the barrier
__device__ __forceinline__ void tone_stage(const ToneHlgArgs &tm, float *lds, int tid, int nthreads) {
    tone_stage(static_cast<const ToneArgs &>(tm), lds, tid, nthreads);
    if constexpr (kHlgGainLds)
        for (int i = 4 * tid; i < kToneGainPad; i += 4 * nthreads)
            *reinterpret_cast<float4 *>(lds + kToneIn + i) = *reinterpret_cast<const float4 *>(tm.lut_gain + i);
}

constexpr uint32_t kGainU0 = 103u << 23, kGainU1 = 127u << 23;   // the bits of 2^-24 and of 1.0

// 8 pixels of source-coded R'G'B' to destination-coded R'G'B', in place; `lin` is the workgroup's
// copy of lut_in (and, for HLG, of lut_gain behind it). Every float32 operation is rounded on its
// own: the pragma keeps the compiler from contracting the products and sums into fused
// multiply-adds (as scale_bias in tensor.hip).
template <typename Tone>
__device__ __forceinline__ void tone_run(const Tone &tm, const float *lin, int (&R)[8], int (&G)[8], int (&B)[8]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 8; k++) {
        // (the matrix clips to [0, Ms]; the identity hands samples on, which a valid picture
        // keeps in that range: the min holds the index inside the table whatever the planes hold)
        const int top = tm.n_in - 1;
        float r = lin[min(R[k], top)], g = lin[min(G[k], top)], b = lin[min(B[k], top)];
        if constexpr (std::is_same_v<Tone, ToneHlgArgs>) {
            // the OOTF gain of the luminance: node and fraction are the bits of Y (a negative or
            // tiny Y clamps to node 0, Y above 1 to the last node, whose neighbour is entry 1537)
            const float y0 = tm.yw[0] * r, y1 = tm.yw[1] * g, y2 = tm.yw[2] * b;
            const float ys = y0 + y1;
            const float Y = ys + y2;
            const uint32_t u = min(max(__float_as_uint(Y), kGainU0), kGainU1), d = u - kGainU0;
            const float *gt = kHlgGainLds ? lin + kToneIn : tm.lut_gain;
            const float g0 = gt[d >> 17], g1 = gt[(d >> 17) + 1];
            const float f = (float)(d & 0x1ffffu) * 0x1p-17f;
            const float dg = g1 - g0;
            const float fd = f * dg;
            const float gain = g0 + fd;
            r = r * gain;
            g = g * gain;
            b = b * gain;
        }
        int o[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float p0 = tm.m[3 * c] * r, p1 = tm.m[3 * c + 1] * g, p2 = tm.m[3 * c + 2] * b;
            const float s = p0 + p1;
            const float t = fminf(fmaxf(s + p2, 0.0f), 1.0f);
            const float q = t * 65535.0f;
            o[c] = (int)tm.lut_out[(int)(q + 0.5f)];
        }
        R[k] = o[0];
        G[k] = o[1];
        B[k] = o[2];
    }
}

// N samples of a plane row from column x0, columns clamped to pw - 1
template <typename Px, int N>
__device__ __forceinline__ void load_run(const uint8_t *row, int x0, int pw, bool vec, int (&v)[N]) {
    const Px *p = reinterpret_cast<const Px *>(row);
    constexpr int kBytes = N * (int)sizeof(Px);
    static_assert(kBytes == 4 || kBytes == 8 || kBytes == 16, "one vector per run");
    if (vec && x0 + N <= pw) {
        uint32_t q[kBytes / 4];
        if constexpr (kBytes == 16) {
            const uint4 t = *reinterpret_cast<const uint4 *>(p + x0);
            q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
        } else if constexpr (kBytes == 8) {
            const uint2 t = *reinterpret_cast<const uint2 *>(p + x0);
            q[0] = t.x; q[1] = t.y;
        } else {
            q[0] = *reinterpret_cast<const uint32_t *>(p + x0);
        }
#pragma unroll
        for (int k = 0; k < N; k++)
            v[k] = sizeof(Px) == 1 ? (int)((q[k >> 2] >> (8 * (k & 3))) & 0xff) : (int)((q[k >> 1] >> (16 * (k & 1))) & 0xffff);
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = (int)p[min(x0 + k, pw - 1)];
    }
}

// N samples to a destination row at sample s0; the row holds `limit` samples
template <typename Px, int N>
__device__ __forceinline__ void store_run(uint8_t *row, int s0, int limit, bool vec, const int (&v)[N]) {
    Px *p = reinterpret_cast<Px *>(row);
    constexpr int kBytes = N * (int)sizeof(Px);
    static_assert(kBytes == 4 || kBytes == 8 || kBytes % 16 == 0, "whole vectors per run");
    if (vec && s0 + N <= limit) {
        uint32_t q[kBytes / 4];
#pragma unroll
        for (int i = 0; i < kBytes / 4; i++) {
            if constexpr (sizeof(Px) == 1)
                q[i] = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) |
                       ((uint32_t)v[4 * i + 3] << 24);
            else
                q[i] = (uint32_t)v[2 * i] | ((uint32_t)v[2 * i + 1] << 16);
        }
        if constexpr (kBytes == 4) {
            *reinterpret_cast<uint32_t *>(p + s0) = q[0];
        } else if constexpr (kBytes == 8) {
            *reinterpret_cast<uint2 *>(p + s0) = make_uint2(q[0], q[1]);
        } else {
#pragma unroll
            for (int i = 0; i < kBytes / 16; i++)
                reinterpret_cast<uint4 *>(p + s0)[i] = make_uint4(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; k++)
            if (s0 + k < limit) p[s0 + k] = (Px)v[k];
    }
}

// chroma columns cx0 .. cx0 + 3 of one row and, in `halo`, column cx0 + 4 (the right neighbour
// of the last odd luma column)
template <typename Px>
__device__ __forceinline__ void load5(const uint8_t *row, int cx0, int cw, bool vec, int (&v)[4], int &halo) {
    load_run<Px, 4>(row, cx0, cw, vec, v);
    halo = (int)reinterpret_cast<const Px *>(row)[min(cx0 + 4, cw - 1)];
}

// the vertical pass of 4:2:0 for one column: c = row j, cp = row max(j-1, 0), cn = row min(j+1, ch-1)
__device__ __forceinline__ void vert420(bool coloc, int cp, int c, int cn, int &even, int &odd) {
    even = coloc ? c : (cp + 3 * c + 2) >> 2;
    odd = coloc ? (c + cn + 1) >> 1 : (3 * c + cn + 2) >> 2;
}

// the horizontal pass over 4 columns and their halo
__device__ __forceinline__ void horz(const int (&v)[4], int halo, int (&o)[8]) {
    o[0] = v[0]; o[1] = (v[0] + v[1] + 1) >> 1;
    o[2] = v[1]; o[3] = (v[1] + v[2] + 1) >> 1;
    o[4] = v[2]; o[5] = (v[2] + v[3] + 1) >> 1;
    o[6] = v[3]; o[7] = (v[3] + halo + 1) >> 1;
}

// chroma plane p at luma resolution for the lane's 8 columns of row unit u: up[r] = luma row
// u * (1 + ss_ver) + r. The vertical pass gives integer rows, the horizontal pass runs over them.
template <typename Px>
__device__ __forceinline__ void upsample(const DisplayArgs &a, int p, int u, int x0, int (&up)[2][8]) {
    const uint8_t *base = a.src[p];
    const int64_t st = a.sstride[1];
    const bool vec = (a.svec >> p) & 1;
    int t0[8], t1[8];   // (both rows are always set, and stored to `up` in one place, so that
                        // they stay in registers; t1 is used by 4:2:0 only)
    if (!a.ss_hor) {   // 4:4:4
        load_run<Px, 8>(base + u * st, x0, a.cw, vec, t0);
#pragma unroll
        for (int k = 0; k < 8; k++) t1[k] = t0[k];
    } else {
        const int cx0 = x0 >> 1;
        int c[4], hc, e[4], he, o[4], ho;
        load5<Px>(base + u * st, cx0, a.cw, vec, c, hc);
        if (!a.ss_ver) {   // 4:2:2
#pragma unroll
            for (int k = 0; k < 4; k++) e[k] = o[k] = c[k];
            he = ho = hc;
        } else {
            int cn[4], hn, cp[4], hp;
            load5<Px>(base + min(u + 1, a.ch - 1) * st, cx0, a.cw, vec, cn, hn);
            // (co-located: the row above is not needed; re-reading row u keeps one code path)
            load5<Px>(base + (a.coloc ? u : max(u - 1, 0)) * st, cx0, a.cw, vec, cp, hp);
#pragma unroll
            for (int k = 0; k < 4; k++) vert420(a.coloc, cp[k], c[k], cn[k], e[k], o[k]);
            vert420(a.coloc, hp, hc, hn, he, ho);
        }
        horz(e, he, t0);
        horz(o, ho, t1);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        up[0][k] = t0[k];
        up[1][k] = t1[k];
    }
}

// 8 pixels (luma and chroma at luma resolution) to R'G'B'
__device__ __forceinline__ void convert_run(const DisplayArgs &a, const int (&y)[8], const int (&cu)[8],
                                            const int (&cv)[8], int (&R)[8], int (&G)[8], int (&B)[8]) {
    constexpr int kRound = 1 << (kDispS - 1);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (a.identity) {
            G[k] = y[k];
            B[k] = cu[k];
            R[k] = cv[k];
        } else {
            const int l = a.ky * (y[k] - a.yo) + kRound;
            int rr = l, gg = l, bb = l;
            if (!a.mono) {
                const int cb = cu[k] - a.half, cr = cv[k] - a.half;
                rr += a.crv * cr;
                gg -= a.cgu * cb + a.cgv * cr;
                bb += a.cbu * cb;
            }
            R[k] = min(max(rr >> kDispS, 0), a.maxv);
            G[k] = min(max(gg >> kDispS, 0), a.maxv);
            B[k] = min(max(bb >> kDispS, 0), a.maxv);
        }
    }
}

}  // namespace mi
