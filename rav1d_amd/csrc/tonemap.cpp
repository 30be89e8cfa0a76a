// tonemap.cpp — the host side of the colour-volume stage (include/mi_av1out.h, MiToneMap): the
// rules, the three tables in double precision (mi_tonemap_tables), for HLG sources the luminance
// row and the OOTF gain table beside them (mi_tonemap_tables_hlg), and the context's device copy
// of them, rebuilt and uploaded on the caller's stream only when the description changes. The
// device side is tone_run (display.h), inside display_kernel, tensor_h_kernel and yuv_tm_kernel.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>

#include "display.h"

namespace mi {
namespace {

constexpr int kOutN = 65536;   // entries of lut_out

// 0 for the primaries the stage converts, else -ENOTSUP (defined) or -EINVAL (2, reserved)
int pri_class(int pri) {
    switch (pri) {
    case 1: case 5: case 6: case 7: case 9: case 12: return 0;
    case 4: case 8: case 10: case 11: case 22: return -ENOTSUP;
    default: return -EINVAL;
    }
}

enum { kCurve709 = 0, kCurveSrgb = 1, kCurvePq = 2, kCurveHlg = 3 };

// the curve of a source trc in *curve, or -ENOTSUP (defined; HLG unless `hlg`) or -EINVAL (2,
// reserved)
int trc_class(int trc, int *curve, bool hlg) {
    switch (trc) {
    case 1: case 6: case 14: case 15: *curve = kCurve709; return 0;
    case 13: *curve = kCurveSrgb; return 0;
    case 16: *curve = kCurvePq; return 0;
    case 18: *curve = kCurveHlg; return hlg ? 0 : -ENOTSUP;
    case 4: case 5: case 7: case 8: case 9: case 10: case 11: case 12: case 17: return -ENOTSUP;
    default: return -EINVAL;
    }
}

bool peak_ok(float p) { return std::isfinite(p) && p >= 1.0f && p <= 10000.0f; }

// ---- ST 2084 ----
constexpr double kM1 = 2610.0 / 16384.0, kM2 = 2523.0 / 32.0, kC1 = 3424.0 / 4096.0, kC2 = 2413.0 / 128.0,
                 kC3 = 2392.0 / 128.0;

double pq_inv_eotf(double nits) {
    const double y = pow(nits / 10000.0, kM1);
    return pow((kC1 + kC2 * y) / (1.0 + kC3 * y), kM2);
}

double pq_eotf(double e) {
    const double p = pow(e, 1.0 / kM2);
    return 10000.0 * pow(fmax(p - kC1, 0.0) / (kC2 - kC3 * p), 1.0 / kM1);
}

// ---- ARIB STD-B67 (HLG) ----
constexpr double kHlgA = 0.17883277, kHlgB = 1.0 - 4.0 * kHlgA;

// the inverse OETF: the scene-linear signal in [0, 1] of x in [0, 1]
double hlg_inv_oetf(double x) {
    const double c = 0.5 - kHlgA * log(4.0 * kHlgA);
    return x <= 0.5 ? x * x / 3.0 : fmin((exp((x - c) / kHlgA) + kHlgB) / 12.0, 1.0);
}

// linear light in [0, 1] of source code value x in [0, 1]
double linear_of(int curve, double x, double src_peak, double dst_peak) {
    if (curve == kCurve709) return x < 0.081 ? x / 4.5 : pow((x + 0.099) / 1.099, 1.0 / 0.45);
    if (curve == kCurveSrgb) return x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4);
    if (curve == kCurveHlg) return hlg_inv_oetf(x);
    // PQ through the BT.2390 EETF (black level 0)
    const double ns = pq_inv_eotf(src_peak), nd = pq_inv_eotf(dst_peak);
    const double e1 = fmin(x / ns, 1.0), max_lum = fmin(nd / ns, 1.0), ks = 1.5 * max_lum - 0.5;
    double e2 = e1;
    if (ks < 1.0 && e1 >= ks) {
        const double t = (e1 - ks) / (1.0 - ks), t2 = t * t, t3 = t2 * t;
        e2 = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * max_lum;
    }
    return fmin(pq_eotf(e2 * ns) / dst_peak, 1.0);
}

double oetf(int dst_trc, double l) {
    if (dst_trc == 1) return l < 0.018 ? 4.5 * l : 1.099 * pow(l, 0.45) - 0.099;
    return l <= 0.0031308 ? 12.92 * l : 1.055 * pow(l, 1.0 / 2.4) - 0.055;
}

// ---- primaries ----
// RGB -> XYZ of H.273 primaries with D65 white: the columns (x, y, 1 - x - y) / y of R, G, B,
// scaled so that R = G = B = 1 gives the white point
void rgb_to_xyz(int pri, double (&m)[3][3]) {
    double xy[3][2];
    switch (pri) {
    case 1: xy[0][0] = 0.640, xy[0][1] = 0.330, xy[1][0] = 0.300, xy[1][1] = 0.600, xy[2][0] = 0.150, xy[2][1] = 0.060; break;
    case 5: xy[0][0] = 0.64, xy[0][1] = 0.33, xy[1][0] = 0.29, xy[1][1] = 0.60, xy[2][0] = 0.15, xy[2][1] = 0.06; break;
    case 6: case 7: xy[0][0] = 0.630, xy[0][1] = 0.340, xy[1][0] = 0.310, xy[1][1] = 0.595, xy[2][0] = 0.155, xy[2][1] = 0.070; break;
    case 9: xy[0][0] = 0.708, xy[0][1] = 0.292, xy[1][0] = 0.170, xy[1][1] = 0.797, xy[2][0] = 0.131, xy[2][1] = 0.046; break;
    default: xy[0][0] = 0.680, xy[0][1] = 0.320, xy[1][0] = 0.265, xy[1][1] = 0.690, xy[2][0] = 0.150, xy[2][1] = 0.060; break;   // 12
    }
    double p[3][3];   // p[row][primary]
    for (int c = 0; c < 3; c++) {
        p[0][c] = xy[c][0] / xy[c][1];
        p[1][c] = 1.0;
        p[2][c] = (1.0 - xy[c][0] - xy[c][1]) / xy[c][1];
    }
    const double w[3] = {0.3127 / 0.3290, 1.0, (1.0 - 0.3127 - 0.3290) / 0.3290};
    // s = inv(p) w by Cramer's rule
    const double det = p[0][0] * (p[1][1] * p[2][2] - p[1][2] * p[2][1]) - p[0][1] * (p[1][0] * p[2][2] - p[1][2] * p[2][0]) +
                       p[0][2] * (p[1][0] * p[2][1] - p[1][1] * p[2][0]);
    for (int c = 0; c < 3; c++) {
        double q[3][3];
        memcpy(q, p, sizeof(q));
        for (int r = 0; r < 3; r++) q[r][c] = w[r];
        const double dc = q[0][0] * (q[1][1] * q[2][2] - q[1][2] * q[2][1]) - q[0][1] * (q[1][0] * q[2][2] - q[1][2] * q[2][0]) +
                          q[0][2] * (q[1][0] * q[2][1] - q[1][1] * q[2][0]);
        for (int r = 0; r < 3; r++) m[r][c] = p[r][c] * dc / det;
    }
}

void invert3(const double (&a)[3][3], double (&o)[3][3]) {
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;   // cofactor of (c, r)
            o[r][c] = (a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1]) / det;
        }
}

// the three tables, each from what it depends on alone; every argument checked before
void tone_table_in(const MiToneMap &tm, int trc, int src_bpc, float *lut_in) {
    int curve = kCurve709;
    (void)trc_class(trc, &curve, true);
    const int n = 1 << src_bpc;
    const double ms = (double)(n - 1);
    // (the running maximum: the BT.709 curve's two segments, with the constants as rounded in the
    // standard, meet 5.5e-5 apart at x = 0.081, which at 12 bits is more than one code's step)
    double top = 0.0;
    for (int v = 0; v < n; v++) {
        top = v == 0 ? 0.0 : fmax(top, linear_of(curve, (double)v / ms, tm.src_peak, tm.dst_peak));
        const float f = (float)top;
        lut_in[v] = std::fpclassify(f) == FP_SUBNORMAL ? 0.0f : f;
    }
}

void tone_table_m(int dst_pri, int pri, float *m) {
    if (pri == dst_pri) {
        for (int i = 0; i < 9; i++) m[i] = i % 4 == 0 ? 1.0f : 0.0f;
    } else {
        double s[3][3], d[3][3], di[3][3];
        rgb_to_xyz(pri, s);
        rgb_to_xyz(dst_pri, d);
        invert3(d, di);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) m[3 * r + c] = (float)(di[r][0] * s[0][c] + di[r][1] * s[1][c] + di[r][2] * s[2][c]);
    }
}

void tone_table_out(int dst_trc, int dst_bpc, uint16_t *lut_out) {
    const double md = (double)((1 << dst_bpc) - 1);
    for (int i = 0; i < kOutN; i++) lut_out[i] = (uint16_t)floor(oetf(dst_trc, (double)i / 65535.0) * md + 0.5);
}

// HLG: the Y row of RGB -> XYZ of the source primaries
void tone_table_yw(int pri, float *yw) {
    double s[3][3];
    rgb_to_xyz(pri, s);
    for (int c = 0; c < 3; c++) yw[c] = (float)s[1][c];
}

// HLG: the OOTF gain Y^(gamma - 1) at the nodes of lut_gain, gamma = 1.2 * 1.111^log2(Lw / 1000)
// (BT.2100-2 note 5, the extended range). Node k is the float32 of bit pattern
// min(U0 + (k << 17), U1), U0 = 2^-24 and U1 = 1.0: entries 1536 and 1537 are exactly 1.
void tone_table_gain(float dst_peak, float *lut_gain) {
    const double gamma = 1.2 * pow(1.111, log2((double)dst_peak / 1000.0));
    const uint32_t u0 = 103u << 23, u1 = 127u << 23;
    for (int k = 0; k < kToneGain; k++) {
        const uint32_t u = std::min(u0 + ((uint32_t)k << 17), u1);
        float y;
        memcpy(&y, &u, sizeof(y));
        lut_gain[k] = (float)pow((double)y, gamma - 1.0);
    }
}

void tone_tables(const MiToneMap &tm, int pri, int trc, int src_bpc, float *lut_in, float *m, uint16_t *lut_out) {
    tone_table_in(tm, trc, src_bpc, lut_in);
    tone_table_m(tm.dst_pri, pri, m);
    tone_table_out(tm.dst_trc, tm.dst_bpc, lut_out);
}

}  // namespace

int tone_check(const MiToneMap *tm, const MiColorInfo *color, bool hlg) {
    if (!tm || !color) return -EINVAL;
    if (tm->dst_pri != 1 && tm->dst_pri != 9 && tm->dst_pri != 12) return -EINVAL;
    if (tm->dst_trc != 1 && tm->dst_trc != 13) return -EINVAL;
    if (tm->dst_bpc != 8 && tm->dst_bpc != 10 && tm->dst_bpc != 12) return -EINVAL;
    // -EINVAL of either field before -ENOTSUP of the other: a malformed description is reported as such
    int curve = kCurve709;
    const int pe = pri_class(color->pri), te = trc_class(color->trc, &curve, hlg);
    if (pe == -EINVAL || te == -EINVAL) return -EINVAL;
    if (pe || te) return -ENOTSUP;
    if (curve == kCurvePq && (!peak_ok(tm->src_peak) || !peak_ok(tm->dst_peak))) return -EINVAL;
    // (HLG is scene-referred: dst_peak is the display the OOTF renders for, src_peak is not read)
    if (curve == kCurveHlg && !peak_ok(tm->dst_peak)) return -EINVAL;
    return 0;
}

int tone_prepare(MiCtx *ctx, const MiToneMap *tm, const MiColorInfo *color, int src_bpc, hipStream_t s, ToneHlgArgs &t) {
    int curve = kCurve709;
    (void)trc_class(color->trc, &curve, true);
    const bool hlg = curve == kCurveHlg;
    // the key: what the tables depend on (sources other than PQ do not read the peaks: the
    // dst_peak of an HLG source is the key of lut_gain alone)
    MiToneMap k = *tm;
    if (curve != kCurvePq) k.src_peak = k.dst_peak = 0.0f;
    int32_t gain_key = 0;
    memcpy(&gain_key, &tm->dst_peak, sizeof(float));
    int32_t key[8] = {k.dst_pri, k.dst_trc, k.dst_bpc, 0, 0, color->pri, color->trc, src_bpc};
    memcpy(&key[3], &k.src_peak, sizeof(float));
    memcpy(&key[4], &k.dst_peak, sizeof(float));
    const size_t out_bytes = (size_t)kOutN * sizeof(uint16_t), in_bytes = (size_t)kToneIn * sizeof(float);
    const size_t gain_bytes = (size_t)kToneGainPad * sizeof(float);   // (behind lut_in, padded to whole float4s)
    if (!ctx->tone_dev) {
        if (hipMalloc(&ctx->tone_dev, out_bytes + in_bytes + gain_bytes) != hipSuccess) {
            ctx->tone_dev = nullptr;
            return ctx->last_error = -ENOMEM;
        }
    }
    // What each table depends on: lut_out on (dst_trc, dst_bpc), lut_in on the peaks, the source
    // trc and depth, m on the two primaries. A change of peaks alone (a caller that follows the
    // stream's light level) rebuilds and uploads lut_in only: lut_out is 65536 pow() and 128 KB.
    const int32_t *old = ctx->tone_key;
    const bool out_stale = !ctx->tone_valid || key[1] != old[1] || key[2] != old[2];
    const bool in_stale = !ctx->tone_valid || key[3] != old[3] || key[4] != old[4] || key[6] != old[6] || key[7] != old[7];
    const bool m_stale = !ctx->tone_valid || key[0] != old[0] || key[5] != old[5];
    // lut_gain is HLG's alone and keyed on its own: PQ and SDR calls in between leave it in place,
    // and a change of dst_peak rebuilds its 1538 entries and neither of the big tables
    const bool gain_stale = hlg && (!ctx->tone_gain_valid || gain_key != ctx->tone_gain_key);
    if (out_stale || in_stale || gain_stale) {
        // Build into the staging buffer whose turn it is. The upload before the last one read it;
        // wait for that one only if it is still pending (two buffers: a change of tables behind
        // another does not wait for the stream).
        const int i = ctx->tone_slot;
        if (!ctx->tone_host[i]) {
            if (hipHostMalloc((void **)&ctx->tone_host[i], out_bytes + in_bytes + gain_bytes, hipHostMallocDefault) != hipSuccess) {
                ctx->tone_host[i] = nullptr;
                return ctx->last_error = -ENOMEM;
            }
            if (hipEventCreateWithFlags(&ctx->tone_ev[i], hipEventDisableTiming) != hipSuccess) {
                ctx->tone_ev[i] = nullptr;
                return ctx->last_error = -ENOMEM;
            }
        }
        if (ctx->tone_ev_pending[i]) {
            if (hipEventSynchronize(ctx->tone_ev[i]) != hipSuccess) return ctx->last_error = -EIO;
            ctx->tone_ev_pending[i] = false;
        }
        uint8_t *h = ctx->tone_host[i];
        if (out_stale || in_stale) {
            ctx->tone_valid = false;
            if (out_stale) tone_table_out(k.dst_trc, k.dst_bpc, (uint16_t *)h);
            if (in_stale) tone_table_in(k, color->trc, src_bpc, (float *)(h + out_bytes));
            // (the tables are adjacent, on the host as on the device: one copy of what changed)
            const size_t from = out_stale ? 0 : out_bytes;
            const size_t to = in_stale ? out_bytes + ((size_t)sizeof(float) << src_bpc) : out_bytes;
            if (hipMemcpyAsync(ctx->tone_dev + from, h + from, to - from, hipMemcpyHostToDevice, s) != hipSuccess)
                return ctx->last_error = -EIO;
        }
        if (gain_stale) {
            ctx->tone_gain_valid = false;
            float *g = (float *)(h + out_bytes + in_bytes);
            tone_table_gain(tm->dst_peak, g);
            for (int j = kToneGain; j < kToneGainPad; j++) g[j] = 1.0f;
            if (hipMemcpyAsync(ctx->tone_dev + out_bytes + in_bytes, g, gain_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
                return ctx->last_error = -EIO;
            ctx->tone_gain_key = gain_key;
            ctx->tone_gain_valid = true;
        }
        if (hipEventRecord(ctx->tone_ev[i], s) != hipSuccess) {
            // without the event the buffer's reuse cannot be ordered: let the upload finish now
            (void)hipStreamSynchronize(s);
        } else {
            ctx->tone_ev_pending[i] = true;
        }
        ctx->tone_slot = i ^ 1;
    }
    if (m_stale) {
        tone_table_m(k.dst_pri, color->pri, ctx->tone_m);
        tone_table_yw(color->pri, ctx->tone_yw);
    }
    memcpy(ctx->tone_key, key, sizeof(key));
    ctx->tone_valid = true;
    t.lut_out = (const uint16_t *)ctx->tone_dev;
    t.lut_in = (const float *)(ctx->tone_dev + out_bytes);
    memcpy(t.m, ctx->tone_m, sizeof(t.m));
    t.n_in = 1 << src_bpc;
    t.maxd = (1 << tm->dst_bpc) - 1;
    t.lut_gain = hlg ? (const float *)(ctx->tone_dev + out_bytes + in_bytes) : nullptr;
    memcpy(t.yw, ctx->tone_yw, sizeof(t.yw));
    return 0;
}

}  // namespace mi

extern "C" int mi_tonemap_tables(const MiToneMap *tm, const MiColorInfo *color, int src_bpc, float *lut_in, float m[9],
                                 uint16_t *lut_out) {
    if (!lut_in || !m || !lut_out || (src_bpc != 8 && src_bpc != 10 && src_bpc != 12)) return -EINVAL;
    if (int e = mi::tone_check(tm, color, false)) return e;
    mi::tone_tables(*tm, color->pri, color->trc, src_bpc, lut_in, m, lut_out);
    return 0;
}

extern "C" int mi_tonemap_tables_hlg(const MiToneMap *tm, const MiColorInfo *color, int src_bpc, float *lut_in, float m[9],
                                     uint16_t *lut_out, float yw[3], float *lut_gain) {
    if (!lut_in || !m || !lut_out || !yw || !lut_gain || (src_bpc != 8 && src_bpc != 10 && src_bpc != 12)) return -EINVAL;
    if (!tm || !color || color->trc != 18) return -EINVAL;
    if (int e = mi::tone_check(tm, color, true)) return e;
    mi::tone_tables(*tm, color->pri, color->trc, src_bpc, lut_in, m, lut_out);
    mi::tone_table_yw(color->pri, yw);
    mi::tone_table_gain(tm->dst_peak, lut_gain);
    return 0;
}

extern "C" int mi_ctx_enable_hlg(MiCtx *ctx, int on) {
    if (!ctx) return -EINVAL;
    ctx->hlg = on != 0;
    return 0;
}

extern "C" int mi_light_level_stats(const uint32_t *hist, int bpc, double percentile, MiLightLevel *out) {
    if (!hist || !out || (bpc != 8 && bpc != 10 && bpc != 12)) return -EINVAL;
    if (!(percentile > 0.0 && percentile <= 100.0)) return -EINVAL;
    const int n = 1 << bpc;
    uint64_t total = 0;
    for (int c = 0; c < n; c++) total += hist[c];
    if (!total) return -EINVAL;
    const double want = ceil(percentile / 100.0 * (double)total), top = (double)(n - 1);
    uint64_t cum = 0;
    int max_code = 0, pct_code = -1;
    double sum = 0.0, max_nits = 0.0, pct_nits = 0.0;
    for (int c = 0; c < n; c++) {
        if (!hist[c]) continue;
        const double nits = mi::pq_eotf((double)c / top);
        cum += hist[c];
        sum += (double)hist[c] * nits;
        max_code = c;
        max_nits = nits;
        if (pct_code < 0 && (double)cum >= want) {
            pct_code = c;
            pct_nits = nits;
        }
    }
    if (pct_code < 0) {   // (the product rounded above N: the last pixel it is)
        pct_code = max_code;
        pct_nits = max_nits;
    }
    out->max_code = max_code;
    out->pct_code = pct_code;
    out->max_nits = max_nits;
    out->pct_nits = pct_nits;
    out->avg_nits = sum / (double)total;
    return 0;
}
