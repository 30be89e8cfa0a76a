// resize.h — the separable resize that tensor.hip (mi_display_tensor, on R'G'B') and scaled.hip
// (mi_display_scaled, on the YUV planes) share: the 18-bit integer taps of include/mi_av1out.h in
// both sitings, of the triangle and of the Mitchell-Netravali cubics (MiResample), and the kernel
// that writes their tables, the host's sizes of the tables and of a segment of the horizontal
// pass, and what the two passes do per tap. The two tap generators are host and device code from
// one source, so mi_resample_taps (resample.cpp) gives on the host what the table kernel writes. The
// callers keep their kernels: what fills the tile of the horizontal pass and what the vertical
// pass does with its sums are theirs, and so is the loop over the taps itself, `#pragma unroll 4`
// in the kernel's own body: in a shared function the same loop compiles to other code (the scaled
// passes' grew by a fifth and ran 2 % slower, profiles/resize_refactor_ab.json).
//
// A tap table of an axis n_in -> n_out (TapAxis, common.h) is start[n_out] count[n_out]
// k[cap][n_out]: output o reads sample clamp(start[o] + j, 0, n_in - 1) with weight k[j][o]. Slots
// j >= count[o] hold zero weights and both passes run all `cap` of them: with one trip count the
// loops unroll and the loads of several taps are in flight together.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>

#include "display.h"

namespace mi {

constexpr int kTensorS = 18;      // fraction bits of a tap
constexpr int kTensorSeg = 2048;  // source columns one workgroup of the horizontal pass holds

// ---- host ----
// The filter of a call: *rs checked (-EINVAL: a filter outside the list, a cubic's b or c not
// finite or outside [0, 1]); NULL is the triangle. A triangle's b and c are not read, and are zero
// here so that they never tell two triangle calls apart.
struct Filter { int filter; float b, c; };
inline int resample_check(const MiResample *rs, Filter &f) {
    f = Filter{MI_RS_TRIANGLE, 0.f, 0.f};
    if (!rs || rs->filter == MI_RS_TRIANGLE) return 0;
    if (rs->filter != MI_RS_CUBIC) return -EINVAL;
    if (!std::isfinite(rs->b) || !std::isfinite(rs->c) || rs->b < 0.f || rs->b > 1.f || rs->c < 0.f || rs->c > 1.f) return -EINVAL;
    f = Filter{MI_RS_CUBIC, rs->b, rs->c};
    return 0;
}
// the support's radius in units of the widened sample pitch
inline int filter_radius(const Filter &f) { return f.filter == MI_RS_CUBIC ? 2 : 1; }

// the most taps an output of the axis has: 2 radius ceil(max(n_in, n_out) / n_out) + 1
inline int tap_cap(int n_in, int n_out, int radius = 1) {
    return 2 * radius * ((std::max(n_in, n_out) + n_out - 1) / n_out) + 1;
}

// The outputs per segment of the horizontal pass: ob consecutive outputs reach at most
// (ob - 1) n_in / n_out + 2 radius max(n_in / n_out, 1) + 1 source columns (either phase), and the
// tile spends up to 15 more on its 8-column runs.
inline int seg_outputs(int n_in, int n_out, int radius = 1) {
    const int64_t room = (int64_t)(kTensorSeg - 20) * n_out - 2 * radius * (int64_t)std::max(n_in, n_out);
    return (int)std::min<int64_t>(room / n_in + 1, 1024);
}

inline void tap_filter(TapList &t, const Filter &f) { t.filter = f.filter, t.b = f.b, t.c = f.c; }

// ---- taps ----
// Output o of an axis n_in -> n_out with phase P (2: centred, 4: co-sited): Rr = P max(n_in, n_out),
// C = (P o + 1) n_in, wt_i = Rr - |C - (P i + 1) n_out| over every integer i, taps where wt_i > 0.
__host__ __device__ __forceinline__ int64_t sited_wt(int64_t rr, int64_t c, int64_t n_out, int64_t ph, int64_t i) {
    const int64_t d = c - (ph * i + 1) * n_out;
    return rr - (d < 0 ? -d : d);
}

static __host__ __device__ void sited_taps(const TapAxis &ax, int o) {
    const int n_in = ax.n_in, n_out = ax.n_out, cap = ax.cap;
    int *start = ax.tab, *count = start + n_out, *k = count + n_out;
    const int64_t ph = ax.phase, rr = ph * (int64_t)(n_in > n_out ? n_in : n_out), c = (ph * (int64_t)o + 1) * n_in, np = ph * (int64_t)n_out;
    // floor((C - Rr) / P n_out) - 1 is left of the support: (P i + 1) n_out <= C - Rr there
    const int64_t a = c - rr;
    int64_t i0 = (a >= 0 ? a / np : -((-a + np - 1) / np)) - 1;
    while (sited_wt(rr, c, n_out, ph, i0) <= 0) i0++;
    int n = 0, best = 0;
    int64_t wsum = 0, wbest = 0;
    while (n < cap) {
        const int64_t w = sited_wt(rr, c, n_out, ph, i0 + n);
        if (w <= 0) break;
        wsum += w;
        if (w > wbest) {   // the first tap with the largest weight
            wbest = w;
            best = n;
        }
        n++;
    }
    int64_t ksum = 0;
    for (int j = 0; j < n; j++) {
        const int64_t kj = ((sited_wt(rr, c, n_out, ph, i0 + j) << kTensorS) + wsum / 2) / wsum;
        k[(int64_t)j * n_out + o] = (int)kj;
        ksum += kj;
    }
    k[(int64_t)best * n_out + o] += (int)(((int64_t)1 << kTensorS) - ksum);
    for (int j = n; j < cap; j++) k[(int64_t)j * n_out + o] = 0;
    start[o] = (int)i0;
    count[o] = n;
}

// The Mitchell-Netravali cubic (b, c) on the same grid (MI_RS_CUBIC of include/mi_av1out.h):
// d_i = |C - (P i + 1) n_out|, taps where d_i < 2 Rr, the weight six times the kernel at t = d_i / Rr
// in float64, every operation rounded on its own in the order the header writes.
struct CubicPoly { double n3, n2, n0, f3, f2, f1, f0; };   // near (d < Rr: no linear term) and far piece

__host__ __device__ __forceinline__ CubicPoly cubic_poly(float bf, float cf) {
#pragma clang fp contract(off)
    const double b = (double)bf, c = (double)cf;
    CubicPoly p;
    p.n3 = 12.0 - 9.0 * b - 6.0 * c;
    p.n2 = -18.0 + 12.0 * b + 6.0 * c;
    p.n0 = 6.0 - 2.0 * b;
    p.f3 = -b - 6.0 * c;
    p.f2 = 6.0 * b + 30.0 * c;
    p.f1 = -12.0 * b - 48.0 * c;
    p.f0 = 8.0 * b + 24.0 * c;
    return p;
}

__host__ __device__ __forceinline__ int64_t sited_dist(int64_t c, int64_t n_out, int64_t ph, int64_t i) {
    const int64_t d = c - (ph * i + 1) * n_out;
    return d < 0 ? -d : d;
}

__host__ __device__ __forceinline__ double cubic_wt(const CubicPoly &p, int64_t d, int64_t rr) {
#pragma clang fp contract(off)
    const double t = (double)d / (double)rr;
    if (d < rr) return ((p.n3 * t + p.n2) * t + 0.0) * t + p.n0;
    return ((p.f3 * t + p.f2) * t + p.f1) * t + p.f0;
}

static __host__ __device__ void cubic_taps(const TapAxis &ax, float b, float c_mn, int o) {
#pragma clang fp contract(off)
    const int n_in = ax.n_in, n_out = ax.n_out, cap = ax.cap;
    int *start = ax.tab, *count = start + n_out, *k = count + n_out;
    if (n_in == n_out) {   // the identity, whatever b is
        k[o] = 1 << kTensorS;
        for (int j = 1; j < cap; j++) k[(int64_t)j * n_out + o] = 0;
        start[o] = o;
        count[o] = 1;
        return;
    }
    const CubicPoly p = cubic_poly(b, c_mn);
    const int64_t ph = ax.phase, rr = ph * (int64_t)(n_in > n_out ? n_in : n_out), c = (ph * (int64_t)o + 1) * n_in, np = ph * (int64_t)n_out;
    // floor((C - 2 Rr) / P n_out) - 1 is left of the support: (P i + 1) n_out <= C - 2 Rr there
    const int64_t a = c - 2 * rr;
    int64_t i0 = (a >= 0 ? a / np : -((-a + np - 1) / np)) - 1;
    while (sited_dist(c, n_out, ph, i0) >= 2 * rr) i0++;
    int n = 0, best = 0;
    double wsum = 0.0, wbest = 0.0;
    while (n < cap) {
        const int64_t d = sited_dist(c, n_out, ph, i0 + n);
        if (d >= 2 * rr) break;
        const double w = cubic_wt(p, d, rr);
        wsum = wsum + w;   // ascending i
        if (n == 0 || w > wbest) {   // the first tap with the largest weight
            wbest = w;
            best = n;
        }
        n++;
    }
    int64_t ksum = 0;
    for (int j = 0; j < n; j++) {
        const double q = cubic_wt(p, sited_dist(c, n_out, ph, i0 + j), rr) / wsum;
        const int64_t kj = (int64_t)floor(q * 262144.0 + 0.5);
        k[(int64_t)j * n_out + o] = (int)kj;
        ksum += kj;
    }
    k[(int64_t)best * n_out + o] += (int)(((int64_t)1 << kTensorS) - ksum);
    for (int j = n; j < cap; j++) k[(int64_t)j * n_out + o] = 0;
    start[o] = (int)i0;
    count[o] = n;
}

// one lane per output position of every axis of the list, so the tables are ordered on the stream
// and no host buffer is involved. A kernel per filter, and the filter beside the axes, not in
// them: the triangle's kernel (the calls without a MiResample) is the code it was and reads the
// arguments it read before there was a second generator. With the float64 code in one kernel its
// launch took half a microsecond longer, and with 16 more bytes per axis a quarter, which a call
// that rebuilds its tables every time (a ladder as single calls) pays per call.
template <bool CUBIC>
static __global__ __launch_bounds__(256) void taps_kernel(const TapList t) {
    int i = blockIdx.x * 256 + threadIdx.x;
    for (int a = 0; a < t.n; a++) {
        if (i < t.ax[a].n_out) {
            if constexpr (CUBIC)
                cubic_taps(t.ax[a], t.b, t.c, i);
            else
                sited_taps(t.ax[a], i);
            return;
        }
        i -= t.ax[a].n_out;
    }
}

static inline int launch_taps(const TapList &t, hipStream_t s) {
    int64_t n = 0;
    for (int a = 0; a < t.n; a++) n += t.ax[a].n_out;
    if (t.filter == MI_RS_CUBIC)
        taps_kernel<true><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(t);
    else
        taps_kernel<false><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(t);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the passes ----
// eight 16-bit samples as one 16-byte vector (an LDS write of the tile fill)
__device__ __forceinline__ uint4 pack8(const int (&v)[8]) {
    return make_uint4((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16),
                      (uint32_t)v[4] | ((uint32_t)v[5] << 16), (uint32_t)v[6] | ((uint32_t)v[7] << 16));
}

// The sums of both passes start at one half, so that the shift by kTensorS rounds.
constexpr int kTensorHalf = 1 << (kTensorS - 1);

// Horizontal pass, one tap of one output column over NC rows of the tile: weight kj and tile
// column clamp(col, lo_i, hi_i), the crop column clamp(start + j, 0, n_in - 1) as a tile column.
// hi_i is held inside the tile by the caller; that bound binds only for zero-weight slots: the
// host sizes ob so that an output's taps fit.
template <int NC>
__device__ __forceinline__ void h_tap(const uint16_t (*tile)[kTensorSeg], int col, int lo_i, int hi_i, int kj, int (&acc)[NC]) {
    const int idx = min(max(col, lo_i), hi_i);
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] += kj * (int)tile[c][idx];
}

// Vertical pass, one tap of 4 adjacent output columns of NC channels: one 8-byte load of `mid`
// per channel (m: channel 0 at the lane's first column, a multiple of 4; `plane` u16 between
// channels, `row` u16 to the tap's row) and the wave-uniform weight kj.
template <int NC>
__device__ __forceinline__ void v_tap(const uint16_t *m, int64_t plane, int64_t row, int kj, int (&acc)[NC][4]) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const uint2 q = *reinterpret_cast<const uint2 *>(m + c * plane + row);
        acc[c][0] += kj * (int)(q.x & 0xffff);
        acc[c][1] += kj * (int)(q.x >> 16);
        acc[c][2] += kj * (int)(q.y & 0xffff);
        acc[c][3] += kj * (int)(q.y >> 16);
    }
}

}  // namespace mi
