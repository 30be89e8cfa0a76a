// yuv_tm.hip — mi_display_yuv_tm and the first step of mi_display_scaled_tm (include/mi_av1out.h,
// "the picture Q"): a shown picture through the colour-volume stage and back to Y'CbCr in a target
// matrix and range at the source's own chroma subsampling, in one pass over the decoded planes.
//
// yuv_tm_kernel keeps display_kernel's lane: 8 luma columns of one row unit (one luma row, or for
// 4:2:0 the row pair that shares a chroma row), a 64 x 4 block, lut_in in LDS. Per luma row it runs
// display.h's upsampler, inverse matrix and tone_run, then the forward matrix in 14-bit integers to
// Y and to full-resolution chroma U4, V4; Y is stored, the chroma is decimated with the siting in
// the taps, one rounding per output sample, and stored as interleaved UV pairs (semi-planar,
// MSB-aligned) or as planes (the scratch picture the scaled passes read).
//
// The decimation reads tone-mapped neighbours of the lane's run:
//   the column to the left (4:2:0, 4:2:2): a wave is one row unit's run of 64 chunks, and its lane 0
//     stores nothing: it recomputes the last chunk of the wave before it, so that every storing
//     lane takes the column from the lane to its left with one cross-lane move per value (a block
//     covers 63 chunks = 504 columns; 1 / 64 of the lanes compute twice);
//   the row above (4:2:0 co-located): the odd row of the row unit above, which the wave above in
//     the block has computed: every wave leaves its odd row's U4, V4 in LDS (16 B per plane and
//     lane), a barrier, and waves 1 - 3 read the wave above; wave 0 of a block, whose unit above
//     belongs to another block, recomputes that one luma row (half a unit more for a quarter of
//     the waves).
// No lane leaves before the end of the chroma path: lanes outside the picture run on clamped
// coordinates and skip the stores.
#include <cerrno>
#include <cmath>
#include <cstring>

#include "display.h"

namespace mi {
namespace {

constexpr int kYuvChunks = 63;   // the chunks a wave stores: lanes 1 .. 63

// 8 pixels of a luma row (luma, chroma at luma resolution) to tone-mapped R'G'B' as the RGB
// formats of mi_display_picture_tm compute it, then the forward matrix: Y, U4, V4
template <typename Tone>
__device__ __forceinline__ void forward_run(const DisplayArgs &a, const Tone &tm, const YuvArgs &f, const float *lin,
                                            const int (&y)[8], const int (&cu)[8], const int (&cv)[8], int (&Y)[8],
                                            int (&U)[8], int (&V)[8]) {
    int R[8], G[8], B[8];
    convert_run(a, y, cu, cv, R, G, B);
    tone_run(tm, lin, R, G, B);
    constexpr int kRound = 1 << (kDispS - 1);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        Y[k] = min(max(((f.yr * R[k] + f.yg * G[k] + f.yb * B[k] + kRound) >> kDispS) + f.yo, 0), f.maxd);
        U[k] = min(max(((f.ur * R[k] + f.ug * G[k] + f.ub * B[k] + kRound) >> kDispS) + f.half, 0), f.maxd);
        V[k] = min(max(((f.vr * R[k] + f.vg * G[k] + f.vb * B[k] + kRound) >> kDispS) + f.half, 0), f.maxd);
    }
}

// The (1, 2, 1) sums of a row's 4 chroma outputs over luma columns 2i-1, 2i, 2i+1, unrounded.
// `c` holds columns x0 .. x0 + 7 and c[7] of the lane to the left is the column before them
// (every lane of the wave calls this); the first column of the picture and the last clamp.
__device__ __forceinline__ void hsum(const int (&c)[8], int x0, int w, int (&o)[4]) {
    int left = __shfl_up(c[7], 1);
    if (x0 == 0) left = c[0];
#pragma unroll
    for (int k = 0; k < 4; k++)
        o[k] = (k ? c[2 * k - 1] : left) + 2 * c[2 * k] + (x0 + 2 * k + 1 < w ? c[2 * k + 1] : c[2 * k]);
}

__device__ __forceinline__ uint4 pack8(const int (&v)[8]) {
    return make_uint4((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16),
                      (uint32_t)v[4] | ((uint32_t)v[5] << 16), (uint32_t)v[6] | ((uint32_t)v[7] << 16));
}

__device__ __forceinline__ void unpack8(const uint4 q, int (&v)[8]) {
    v[0] = q.x & 0xffff; v[1] = q.x >> 16; v[2] = q.y & 0xffff; v[3] = q.y >> 16;
    v[4] = q.z & 0xffff; v[5] = q.z >> 16; v[6] = q.w & 0xffff; v[7] = q.w >> 16;
}

// N chroma samples of row `row` from chroma column c0: U and V as planes, or as interleaved pairs
template <typename Dx, bool PLANAR, int N>
__device__ __forceinline__ void store_uv(const DisplayArgs &a, const YuvArgs &f, int row, int c0, const int (&u)[N], const int (&v)[N]) {
    if constexpr (PLANAR) {
        store_run<Dx, N>(a.dst[1] + (int64_t)row * a.dstride[1], c0, a.cw, (a.dvec >> 1) & 1, u);
        store_run<Dx, N>(a.dst[2] + (int64_t)row * a.dstride[2], c0, a.cw, (a.dvec >> 2) & 1, v);
    } else {
        int o[2 * N];
#pragma unroll
        for (int k = 0; k < N; k++) {
            o[2 * k] = u[k] << f.shift;
            o[2 * k + 1] = v[k] << f.shift;
        }
        store_run<Dx, 2 * N>(a.dst[1] + (int64_t)row * a.dstride[1], 2 * c0, 2 * a.cw, (a.dvec >> 1) & 1, o);
    }
}

// Px: the source samples; Dx: the destination samples (of dst_bpc); PLANAR: the scratch picture
// (LSB-aligned planes), else semi-planar (MSB-aligned, interleaved UV); TM: kToneTable, or kToneHlg
// with the HLG gain in the stage
template <typename Px, typename Dx, bool PLANAR, int TM>
__global__ __launch_bounds__(256) void yuv_tm_kernel(const DisplayArgs a, const ToneParam<TM> tm, const YuvArgs f) {
    __shared__ __attribute__((aligned(16))) float lut[tone_lds<ToneParam<TM>>()];
    __shared__ uint4 above[4][64][2];   // a wave's odd row: U4, V4 as 8 u16 each
    tone_stage(tm, lut, threadIdx.y * 64 + threadIdx.x, 256);
    __syncthreads();
    const float *lin = lut;
    const int cxr = (int)blockIdx.x * kYuvChunks + (int)threadIdx.x - 1, ur = (int)blockIdx.y * 4 + (int)threadIdx.y;
    const bool active = threadIdx.x > 0 && cxr < a.chunks && ur < a.units;
    // (lanes that store nothing stay inside the picture, so that their loads do)
    const int cx = min(max(cxr, 0), a.chunks - 1), u = min(ur, a.units - 1);
    const int x0 = cx * 8, nrows = 1 + a.ss_ver, r0 = u * nrows;
    const int yshift = PLANAR ? 0 : f.shift;

    int y[2][8];
    load_run<Px, 8>(a.src[0] + r0 * a.sstride[0], x0, a.w, a.svec & 1, y[0]);
    if (a.ss_ver) {
        load_run<Px, 8>(a.src[0] + min(r0 + 1, a.h - 1) * a.sstride[0], x0, a.w, a.svec & 1, y[1]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) y[1][k] = y[0][k];   // (not used)
    }
    int cu[2][8] = {}, cv[2][8] = {};
    if (!a.mono) {
        upsample<Px>(a, 1, u, x0, cu);
        upsample<Px>(a, 2, u, x0, cv);
    }

    // the unit's rows: Y out, U4 / V4 kept (e: the even or only row, o: the odd row of 4:2:0)
    int Y[8], ue[8], ve[8], uo[8], vo[8];
    forward_run(a, tm, f, lin, y[0], cu[0], cv[0], Y, ue, ve);
    if (active) {
        int o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) o[k] = Y[k] << yshift;
        store_run<Dx, 8>(a.dst[0] + (int64_t)r0 * a.dstride[0], x0, a.w, a.dvec & 1, o);
    }
    if (a.ss_ver && r0 + 1 < a.h) {
        forward_run(a, tm, f, lin, y[1], cu[1], cv[1], Y, uo, vo);
        if (active) {
            int o[8];
#pragma unroll
            for (int k = 0; k < 8; k++) o[k] = Y[k] << yshift;
            store_run<Dx, 8>(a.dst[0] + (int64_t)(r0 + 1) * a.dstride[0], x0, a.w, a.dvec & 1, o);
        }
    } else {
        // row min(2j+1, h-1) of the last unit of an odd height is row 2j
#pragma unroll
        for (int k = 0; k < 8; k++) {
            uo[k] = ue[k];
            vo[k] = ve[k];
        }
    }
    if (a.mono) return;   // (block-uniform, as every branch around the barrier below)

    if (!a.ss_hor) {   // 4:4:4: U = U4, V = V4
        if (active) store_uv<Dx, PLANAR, 8>(a, f, u, x0, ue, ve);
        return;
    }
    int su[4], sv[4], shift = 2;   // the weighted sums and log2 of the weights' sum
    hsum(ue, x0, a.w, su);
    hsum(ve, x0, a.w, sv);
    if (a.ss_ver) {
        int t[4];
        if (a.coloc) {
            // rows 2j-1, 2j, 2j+1 with (1, 2, 1): the row above is the odd row of the unit above
            int ua[8], va[8];
            above[threadIdx.y][threadIdx.x][0] = pack8(uo);
            above[threadIdx.y][threadIdx.x][1] = pack8(vo);
            __syncthreads();
            if (u == 0) {   // row max(2j-1, 0) of the first unit is row 0
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    ua[k] = ue[k];
                    va[k] = ve[k];
                }
            } else if (threadIdx.y > 0) {
                unpack8(above[threadIdx.y - 1][threadIdx.x][0], ua);
                unpack8(above[threadIdx.y - 1][threadIdx.x][1], va);
            } else {   // the unit above is another block's: its odd row again
                int ya[8], ca[2][8], da[2][8], yd[8];
                load_run<Px, 8>(a.src[0] + (r0 - 1) * a.sstride[0], x0, a.w, a.svec & 1, ya);
                upsample<Px>(a, 1, u - 1, x0, ca);
                upsample<Px>(a, 2, u - 1, x0, da);
                forward_run(a, tm, f, lin, ya, ca[1], da[1], yd, ua, va);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                su[k] *= 2;
                sv[k] *= 2;
            }
            hsum(ua, x0, a.w, t);
#pragma unroll
            for (int k = 0; k < 4; k++) su[k] += t[k];
            hsum(va, x0, a.w, t);
#pragma unroll
            for (int k = 0; k < 4; k++) sv[k] += t[k];
            shift = 4;
        } else {
            shift = 3;   // rows 2j, 2j+1 with (1, 1)
        }
        hsum(uo, x0, a.w, t);
#pragma unroll
        for (int k = 0; k < 4; k++) su[k] += t[k];
        hsum(vo, x0, a.w, t);
#pragma unroll
        for (int k = 0; k < 4; k++) sv[k] += t[k];
    }
    const int half = 1 << (shift - 1);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        su[k] = (su[k] + half) >> shift;
        sv[k] = (sv[k] + half) >> shift;
    }
    if (active) store_uv<Dx, PLANAR, 4>(a, f, u, x0 >> 1, su, sv);
}

template <typename Px, typename Dx, int TM>
int launch_px(const DisplayArgs &a, const ToneParam<TM> &tm, const YuvArgs &f, bool planar, hipStream_t s) {
    const dim3 block(64, 4), grid((a.chunks + kYuvChunks - 1) / kYuvChunks, (a.units + 3) / 4);
    if (planar)
        yuv_tm_kernel<Px, Dx, true, TM><<<grid, block, 0, s>>>(a, tm, f);
    else
        yuv_tm_kernel<Px, Dx, false, TM><<<grid, block, 0, s>>>(a, tm, f);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int TM>
int launch_tm(const DisplayArgs &a, const ToneParam<TM> &tm, const YuvArgs &f, int bpc, int dst_bpc, bool planar, hipStream_t s) {
    if (bpc == 8)
        return dst_bpc == 8 ? launch_px<uint8_t, uint8_t, TM>(a, tm, f, planar, s) : launch_px<uint8_t, uint16_t, TM>(a, tm, f, planar, s);
    return dst_bpc == 8 ? launch_px<uint16_t, uint8_t, TM>(a, tm, f, planar, s) : launch_px<uint16_t, uint16_t, TM>(a, tm, f, planar, s);
}

}  // namespace

int launch_yuv_tm(const DisplayArgs &a, const ToneHlgArgs &tm, const YuvArgs &f, int bpc, int dst_bpc, bool planar, hipStream_t s) {
    return tm.lut_gain ? launch_tm<kToneHlg>(a, tm, f, bpc, dst_bpc, planar, s)
                       : launch_tm<kToneTable>(a, tm, f, bpc, dst_bpc, planar, s);
}

int yuv_tm_check(const MiPicture *in, const MiColorInfo *color, const MiToneMap *tm, const MiYuvTarget *target,
                 bool hlg, DisplayArgs &a, YuvArgs &f) {
    if (!tm || !target) return -EINVAL;
    if (int e = display_color(in, color, a)) return e;
    if (int e = tone_check(tm, color, hlg)) return e;
    double kr, kb;
    // (the caller chooses the target: a value without a Kr / Kb matrix is malformed, not unsupported)
    if (matrix_k(target->mtrx, &kr, &kb) || (target->range != 0 && target->range != 1)) return -EINVAL;
    const int d = tm->dst_bpc;
    const double md = (double)((1 << d) - 1), kg = 1.0 - kr - kb;
    const double sy = target->range ? 1.0 : (double)(219 << (d - 8)) / md;
    const double sc = target->range ? 1.0 : (double)(224 << (d - 8)) / md;
    f.yr = round_fix(kr * sy);
    f.yb = round_fix(kb * sy);
    f.yg = round_fix(sy) - f.yr - f.yb;
    f.ur = -round_fix(sc * kr / (2.0 * (1.0 - kb)));
    f.ug = -round_fix(sc * kg / (2.0 * (1.0 - kb)));
    f.ub = -(f.ur + f.ug);
    f.vg = -round_fix(sc * kg / (2.0 * (1.0 - kr)));
    f.vb = -round_fix(sc * kb / (2.0 * (1.0 - kr)));
    f.vr = -(f.vg + f.vb);
    f.yo = target->range ? 0 : 16 << (d - 8);
    f.half = 1 << (d - 1);
    f.maxd = (1 << d) - 1;
    f.shift = d > 8 ? 16 - d : 0;
    return 0;
}

int yuv_tm_scratch(MiCtx *ctx, const MiPicture *in, int dst_bpc, MiPicture *q) {
    const int ss_hor = in->layout == 1 || in->layout == 2, ss_ver = in->layout == 1;
    const size_t es = dst_bpc == 8 ? 1 : 2;
    const size_t cw = ((size_t)in->w + ss_hor) >> ss_hor, ch = ((size_t)in->h + ss_ver) >> ss_ver;
    const size_t ystride = ((size_t)in->w * es + 127) & ~(size_t)127, cstride = (cw * es + 127) & ~(size_t)127;
    const size_t ybytes = (ystride * (size_t)in->h + 255) & ~(size_t)255;
    const size_t cbytes = in->layout ? (cstride * ch + 255) & ~(size_t)255 : 0;
    if (ybytes + 2 * cbytes > ctx->disp_q_bytes) {
        if (ctx->disp_q) (void)hipFree(ctx->disp_q);   // (waits for the work that reads it)
        ctx->disp_q = nullptr;
        ctx->disp_q_bytes = 0;
        if (hipMalloc(&ctx->disp_q, ybytes + 2 * cbytes) != hipSuccess) return ctx->last_error = -ENOMEM;
        ctx->disp_q_bytes = ybytes + 2 * cbytes;
    }
    *q = *in;
    q->bpc = dst_bpc;
    q->data[0] = ctx->disp_q;
    q->data[1] = in->layout ? ctx->disp_q + ybytes : nullptr;
    q->data[2] = in->layout ? ctx->disp_q + ybytes + cbytes : nullptr;
    q->stride[0] = (ptrdiff_t)ystride;
    q->stride[1] = in->layout ? (ptrdiff_t)cstride : 0;
    return 0;
}

int yuv_tm_picture(const MiPicture &src, const MiColorInfo *color, DisplayArgs a, const ToneHlgArgs &tm, const YuvArgs &f,
                   const MiPicture *q, void *const dst[2], const ptrdiff_t dstride[2], int dst_bpc, hipStream_t s) {
    display_source(src, color, a);
    const int ndst = src.layout ? (q ? 3 : 2) : 1;
    for (int p = 0; p < ndst; p++) {
        void *d = q ? q->data[p] : dst[p];
        const ptrdiff_t st = q ? q->stride[p ? 1 : 0] : dstride[p];
        a.dst[p] = (uint8_t *)d;
        a.dstride[p] = st;
        if (aligned_to(d, st, 16)) a.dvec |= 1 << p;
    }
    a.chunks = (src.w + 7) >> 3;
    a.units = src.layout == 1 ? (src.h + 1) >> 1 : src.h;
    return launch_yuv_tm(a, tm, f, src.bpc, dst_bpc, q != nullptr, s);
}

}  // namespace mi

extern "C" int mi_display_yuv_tm(MiCtx *ctx, const MiPicture *in, const MiDisplayImage *out, const MiColorInfo *color,
                                 const MiToneMap *tm, const MiYuvTarget *target, const MiFilmGrainData *fg, void *stream) {
    if (!in || !out) return -EINVAL;
    if (int e = mi::display_check_picture(in)) return e;
    if (out->w != in->w || out->h != in->h) return -EINVAL;
    if (out->bpc != 8 && out->bpc != 10 && out->bpc != 12) return -EINVAL;
    if (out->format != MI_OUT_SEMIPLANAR) return -EINVAL;
    const int ss_hor = in->layout == 1 || in->layout == 2;
    const int dpxb = out->bpc == 8 ? 1 : 2;
    const int ndst = in->layout ? 2 : 1;
    for (int p = 0; p < ndst; p++) {
        const int64_t samples = p ? 2 * (int64_t)((in->w + ss_hor) >> ss_hor) : in->w;
        if (!out->data[p] || out->stride[p] < samples * dpxb) return -EINVAL;
        if (((uintptr_t)out->data[p] | (uintptr_t)out->stride[p]) & (uintptr_t)(dpxb - 1)) return -EINVAL;
    }
    if (int e = mi::display_check_strides(in)) return e;
    mi::DisplayArgs a;
    mi::YuvArgs f;
    memset(&a, 0, sizeof(a));
    memset(&f, 0, sizeof(f));
    if (int e = mi::yuv_tm_check(in, color, tm, target, ctx && ctx->hlg, a, f)) return e;
    if (out->bpc != tm->dst_bpc) return -EINVAL;
    if (!ctx) return -EINVAL;

    // allocations and the table upload first: a call that fails there has launched nothing
    mi::ToneHlgArgs ta;
    if (int e = mi::tone_prepare(ctx, tm, color, in->bpc, (hipStream_t)stream, ta)) return e;
    MiPicture src = *in;
    if (fg)
        if (int e = mi::display_grain(ctx, in, &src, fg, color, stream)) return e;
    void *const dst[2] = {out->data[0], out->data[1]};
    const ptrdiff_t dstride[2] = {out->stride[0], out->stride[1]};
    if (mi::yuv_tm_picture(src, color, a, ta, f, nullptr, dst, dstride, out->bpc, (hipStream_t)stream))
        return ctx->last_error = -EIO;
    return 0;
}
