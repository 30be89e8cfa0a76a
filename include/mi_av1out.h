/*
 * mi_av1out.h — the output side of the decode path: displayed pictures from the device to the
 * host (film grain fused with the copy) and the reference's output muxers.
 *
 * Two libraries implement it:
 *   - librav1d_amd.so (gfx950): mi_host_picture_alloc / _free, mi_output_picture, and the
 *     output that stays on the device, mi_display_picture, mi_display_tensor,
 *     mi_display_scaled and the tone-mapped mi_display_yuv_tm / mi_display_scaled_tm;
 *   - libmi_av1dec.so (host C++): the muxers mi_muxer_* (no GPU code).
 *
 * Reference: the CLI's output stage (tools/output/output.rs), its muxers md5
 * (tools/output/md5.rs:541-637), yuv (tools/output/yuv.rs) and y4m2 (tools/output/y4m2.rs),
 * and the film-grain application rav1d runs on the picture it returns to the caller
 * (rav1d_apply_grain, src/fg_apply.rs:272-284; src/lib.rs output_picture_ready).
 *
 * Errors: 0 or a negative errno, as in mi_av1dsp.h.
 */
#ifndef MI_AV1OUT_H
#define MI_AV1OUT_H

#include <stddef.h>
#include <stdint.h>

#include "mi_av1dsp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device -> host (librav1d_amd.so) ---------------------------------------------------- */

/* A picture in pinned, device-mapped host memory with the default-allocator geometry of the
 * device pictures (src/picture.rs:98-115: 128-aligned planes, +64 B on strides that are a
 * multiple of 1024), so a kernel can write it directly over PCIe. */
int  mi_host_picture_alloc(int w, int h, int layout, int bpc, MiPicture *pic);
void mi_host_picture_free(MiPicture *pic);

/* Enqueue the output of one displayed picture on `stream`: `out` (from mi_host_picture_alloc,
 * same geometry as `in`) receives `in` with film grain applied when `fg` is non-NULL — the
 * grain kernel stores its output straight into the host picture, so the grain pass and the
 * device-to-host copy are one pass over the picture — or a plain copy of the visible w x h
 * area otherwise. The host may read `out` once the stream is synchronised. */
int mi_output_picture(MiCtx *ctx, const MiPicture *in, const MiPicture *out,
                      const MiFilmGrainData *fg, int mtrx_identity, void *stream);

/* ---- muxers (libmi_av1dec.so) ----------------------------------------------------------- */

/* What a muxer's header needs (Dav1dPictureParameters + the sequence / frame header fields
 * y4m2 reads: seq_hdr.chr, frame_hdr.render_width / render_height). */
typedef struct MiOutParams {
    int32_t w, h, bpc, layout;
    int32_t chr;                  /* Dav1dChromaSamplePosition: 0 unknown, 1 vertical, 2 colocated */
    int32_t render_w, render_h;
} MiOutParams;

/* The sequence header's colour description (Dav1dSequenceHeader: include/dav1d/headers.rs), with
 * the values of Dav1dColorPrimaries, Dav1dTransferCharacteristics, Dav1dMatrixCoefficients,
 * color_range (0 limited, 1 full) and Dav1dChromaSamplePosition (0 unknown, 1 vertical,
 * 2 colocated). 2 is "unspecified" for pri, trc and mtrx. */
typedef struct MiColorInfo { int32_t pri, trc, mtrx, range, chr; } MiColorInfo;

typedef struct MiMuxer MiMuxer;

/* name: "md5", "yuv", "y4m2" or "null" (tools/output/output.rs muxer table). file: a path, or
 * "-" for stdout, or NULL (md5 only: keep the digest for mi_muxer_digest / mi_muxer_verify).
 * fps: numerator, denominator (y4m2 header). -EINVAL on an unknown muxer, -EIO if the file
 * cannot be opened. */
int  mi_muxer_open(MiMuxer **out, const char *name, const char *file, const MiOutParams *p,
                   const unsigned fps[2]);
/* Write one displayed picture (host memory; rows of w << (bpc > 8) bytes per plane, the
 * visible area only, little-endian pixels). */
int  mi_muxer_write(MiMuxer *m, const MiPicture *pic);
/* md5: finish the hash and compare with a 32-hex-digit string (md5_verify): 0 equal, 1
 * different, -1 string too short; other muxers -EINVAL. */
int  mi_muxer_verify(MiMuxer *m, const char *md5_str);
/* md5: finish the hash and write the 32 hex digits + NUL to out (what md5_close prints). */
int  mi_muxer_digest(MiMuxer *m, char out[33]);
/* Write the trailer (md5: the digest line), close the file, free the muxer. */
void mi_muxer_close(MiMuxer *m);

/* ---- device display output (librav1d_amd.so) --------------------------------------------- */

/* A shown picture for a consumer on the device: tight (no 128-alignment; the strides are the
 * caller's, only w x h is written), with film grain, as semi-planar YUV or as R'G'B'.
 *
 * MI_OUT_SEMIPLANAR: data[0] = Y, data[1] = interleaved UV at the source's own subsampling
 *   (NV12 / P010 for 4:2:0, NV16 / P210 for 4:2:2, NV24 for 4:4:4; 4:0:0 writes Y only).
 *   8 bpc: u8; 10 / 12 bpc: u16, MSB-aligned (v << (16 - bpc), the P010 / P012 convention).
 * MI_OUT_RGB_PLANAR: data[0..2] = the R, G, B planes, w x h each; u8 at 8 bpc, else u16
 *   LSB-aligned; full range at the source bit depth.
 * MI_OUT_RGBA_PACKED: data[0] = h x w x 4 samples of the same type, A = 2^bpc - 1.
 *
 * The RGB formats upsample the chroma with integer arithmetic and clamped indices, the vertical
 * pass first (cw x ch = the chroma plane size):
 *   vertical, 4:2:0, chr == 2 (co-located): row 2j = c[j], row 2j+1 = (c[j] + c[min(j+1, ch-1)] + 1) >> 1;
 *   vertical, 4:2:0, chr 0 or 1 (centred):  row 2j = (c[max(j-1, 0)] + 3 c[j] + 2) >> 2,
 *                                            row 2j+1 = (3 c[j] + c[min(j+1, ch-1)] + 2) >> 2;
 *   horizontal, 4:2:0 and 4:2:2: column 2i = c[i], column 2i+1 = (c[i] + c[min(i+1, cw-1)] + 1) >> 1.
 * and convert with 14-bit fixed-point coefficients computed on the host from color->mtrx
 * (1, 4, 5, 6, 7, 9), color->range and the bit depth (b = bpc, M = 2^b - 1, H = 2^(b-1), S = 14;
 * limited: Yo = 16 << (b-8), ky = round(2^S M / (219 << (b-8))), kc = M / (224 << (b-8)); full:
 * Yo = 0, ky = 2^S, kc = 1; crv = round(2^S 2(1-Kr) kc), cbu = round(2^S 2(1-Kb) kc),
 * cgu = round(2^S 2 Kb(1-Kb)/Kg kc), cgv = round(2^S 2 Kr(1-Kr)/Kg kc), Kg = 1 - Kr - Kb):
 *   R = clip((ky (y-Yo) + crv (v-H) + 2^(S-1)) >> S, 0, M)
 *   G = clip((ky (y-Yo) - cgu (u-H) - cgv (v-H) + 2^(S-1)) >> S, 0, M)
 *   B = clip((ky (y-Yo) + cbu (u-H) + 2^(S-1)) >> S, 0, M)
 * mtrx 0 (identity, 4:4:4 only): G = Y, B = U, R = V. 4:0:0: R = G = B from the luma term. No
 * transfer-function or primaries conversion: the output is R'G'B' in the stream's primaries
 * (mi_display_picture_tm and mi_display_tensor_tm below add that stage). */
enum { MI_OUT_SEMIPLANAR = 0, MI_OUT_RGB_PLANAR = 1, MI_OUT_RGBA_PACKED = 2 };
typedef struct MiDisplayImage {
    void *data[3]; ptrdiff_t stride[3];   /* bytes; any device-accessible memory */
    int32_t w, h, format, bpc;            /* w x h = the visible size of `in` */
} MiDisplayImage;

/* Enqueue the display output of `in` on `stream` (never synchronises). With `fg`, film grain is
 * applied first (mi_film_grain_frame, mtrx_identity = color && color->mtrx == 0) into a scratch
 * picture the context owns (allocated on first use, kept while the geometry stays the same) and
 * the conversion reads that. `color` may be NULL for MI_OUT_SEMIPLANAR.
 * Every check precedes any device work: -EINVAL for a null or malformed argument, a size or bpc
 * that differs from `in`, an unknown format, an RGB format with NULL `color` or mtrx 2
 * (unspecified: the caller has to choose), identity without 4:4:4; -ENOTSUP for matrices 8 and
 * 10-14; -ENOMEM, -EIO. */
int mi_display_picture(MiCtx *ctx, const MiPicture *in, const MiDisplayImage *out,
                       const MiColorInfo *color, const MiFilmGrainData *fg, void *stream);

/* ---- device tensor output (librav1d_amd.so) ---------------------------------------------- */

/* A shown picture as the tensor an ML consumer on the device reads: cropped, resized, normalised
 * R'G'B', 3 channels (R, G, B) of w x h elements, in one pass over the decoded planes.
 *
 * The result is finish(resize(crop(P))), P the w x h picture MI_OUT_RGB_PLANAR gives for the same
 * `in`, `color` and `fg` (the same chroma upsampler over the whole picture, the same matrix, the
 * same colour rules, film grain through the same scratch picture), M = 2^bpc - 1.
 *
 * crop: crop_w x crop_h luma pixels of P at (crop_x, crop_y), inside the picture and at least
 *   1 x 1; crop_w == 0 and crop_h == 0 take the whole picture (crop_x, crop_y are not read then).
 *   The crop never changes a sample's value: odd origins are fine in 4:2:0.
 * resize: separable, the horizontal pass first, its result an integer in [0, M] the vertical pass
 *   runs over. Per axis (n_in the crop extent, n_out the output extent, S = 18), in exact integers:
 *     Rr = 2 max(n_in, n_out); for output o, C = (2o+1) n_in; for every integer i
 *     wt_i = Rr - |C - (2i+1) n_out|; the taps are the i with wt_i > 0 (a triangle filter on
 *     half-pixel centres, widened by the downscale ratio; plain bilinear when n_in <= n_out);
 *     W = sum wt_i, k_i = (wt_i 2^S + W/2) / W (floor); 2^S - sum k_i is added to the first tap
 *     with the largest wt_i; tap i reads crop sample clamp(i, 0, n_in - 1);
 *     out[o] = (sum k_i x_i + 2^(S-1)) >> S.
 *   n_in == n_out is the identity. A downscale above 64:1 on either axis (n_in > 64 n_out) is
 *   -EINVAL.
 * finish, v the integer result:
 *   MI_T_U8: v at 8 bpc, else min(255, (v + 2^(bpc-9)) >> (bpc-8)); scale and bias are not read;
 *   float dtypes: f = fl32(fl32(float(v) * scale[c]) + bias[c]), two separately rounded float32
 *   operations; MI_T_F32 stores f, MI_T_F16 / MI_T_BF16 store f rounded to nearest-even.
 * destination: element (c, y, x) is at data + c stride[0] + y stride[1] + x stride[2]; only the
 *   3 w h elements are written. Column stride == element size (CHW) and channel stride == element
 *   size with a column stride of 3 elements (HWC) are the fast orders, so a slice of an NCHW or
 *   channels-last batch is one of them; any other strides are stored element by element. */
enum { MI_T_U8 = 0, MI_T_F16 = 1, MI_T_BF16 = 2, MI_T_F32 = 3 };
typedef struct MiTensorImage {
    void *data; ptrdiff_t stride[3];     /* bytes between channels, rows, columns */
    int32_t w, h, dtype;                 /* output size; 3 channels, R, G, B */
    int32_t crop_x, crop_y, crop_w, crop_h;  /* luma pixels of `in`; crop_w == 0 and crop_h == 0: the whole picture */
    float scale[3], bias[3];             /* float dtypes: out = fl(fl(float(v) * scale[c]) + bias[c]) */
} MiTensorImage;

/* Enqueue the tensor output of `in` on `stream` (never synchronises); the context owns the
 * scratch between the two passes (allocated on first use, replaced only when a call needs more).
 * Every check precedes any device work: -EINVAL for a null or malformed argument, w or h outside
 * 1..65536, an unknown dtype, a stride that is not a positive multiple of the element size, a
 * `data` not aligned to it, a crop outside the picture or of zero extent, a downscale above 64:1,
 * a non-finite scale or bias (float dtypes), NULL `color`, mtrx 2 or reserved, a bad range,
 * identity without 4:4:4; -ENOTSUP for matrices 8 and 10-14; -ENOMEM and -EIO as above. */
int mi_display_tensor(MiCtx *ctx, const MiPicture *in, const MiTensorImage *out,
                      const MiColorInfo *color, const MiFilmGrainData *fg, void *stream);

/* ---- colour-volume stage: tone mapping and gamut conversion (librav1d_amd.so) ------------ */

/* An optional stage after the matrix, in the same pass: source-coded R'G'B' at the source depth
 * (the integers the matrix gives, identity and 4:0:0 included, clipped to [0, Ms]) to
 * destination-coded R'G'B' at dst_bpc. The source is described by color->pri and color->trc:
 *   pri 1, 5, 6, 7, 9, 12 (H.273 chromaticities, D65 white (0.3127, 0.3290)); 2 (unspecified: the
 *     caller has to choose, as for mtrx 2) and reserved values are -EINVAL, every other defined
 *     value (4, 8, 10, 11, 22) -ENOTSUP;
 *   trc 1, 6, 14, 15 (the BT.709 curve), 13 (sRGB), 16 (PQ, ST 2084); 2 and reserved values are
 *     -EINVAL, every other defined value (4, 5, 7 - 12, 17, 18) -ENOTSUP. 18 (HLG, ARIB STD-B67)
 *     is a source on a context that has opted in (mi_ctx_enable_hlg, "HLG sources" below) and
 *     -ENOTSUP everywhere else.
 * Ms = 2^src_bpc - 1, Md = 2^dst_bpc - 1. Three tables, built on the host in double precision and
 * rounded once:
 *   lut_in[v], v = 0 .. Ms, x = v / Ms: linear light in [0, 1] as float32.
 *     BT.709 curve: x / 4.5 for x < 0.081, else ((x + 0.099) / 1.099)^(1 / 0.45);
 *     sRGB: x / 12.92 for x <= 0.04045, else ((x + 0.055) / 1.055)^2.4;
 *     PQ: m1 = 2610/16384, m2 = 2523/32, c1 = 3424/4096, c2 = 2413/128, c3 = 2392/128,
 *       N(L) = ((c1 + c2 Y^m1) / (1 + c3 Y^m1))^m2 with Y = L / 10000 (the inverse EOTF of L nits),
 *       EOTF(E) = 10000 (max(E^(1/m2) - c1, 0) / (c2 - c3 E^(1/m2)))^(1/m1) nits; the BT.2390 EETF
 *       with black level 0, per channel on the R'G'B' signal: E1 = min(x / N(src_peak), 1),
 *       maxLum = min(N(dst_peak) / N(src_peak), 1), KS = 1.5 maxLum - 0.5; E2 = E1 for E1 < KS (and
 *       always when KS = 1), else with T = (E1 - KS) / (1 - KS)
 *       E2 = (2T^3 - 3T^2 + 1) KS + (T^3 - 2T^2 + T)(1 - KS) + (-2T^3 + 3T^2) maxLum;
 *       lut_in = min(EOTF(E2 N(src_peak)) / dst_peak, 1).
 *     lut_in[0] is exactly 0, and every later entry is the largest value of the formula over the
 *     codes 1 .. v (the table never decreases: the two segments of the BT.709 curve, with the
 *     constants as the standard rounds them, meet 5.5e-5 apart at x = 0.081, more than a 12-bit
 *     code's step); a value that would round to a subnormal float32 is 0.
 *   m[9]: row-major float32 of inv(RGB->XYZ of dst_pri) (RGB->XYZ of color->pri); the exact
 *     identity when the two are the same value.
 *   lut_out[i], i = 0 .. 65535: floor(OETF(i / 65535) Md + 0.5) as uint16, L = i / 65535.
 *     BT.709: 4.5 L for L < 0.018, else 1.099 L^0.45 - 0.099;
 *     sRGB: 12.92 L for L <= 0.0031308, else 1.055 L^(1/2.4) - 0.055.
 * Per pixel on the device, every float32 operation rounded separately (no fused multiply-add):
 *   r = lut_in[R'], g = lut_in[G'], b = lut_in[B']; for each row k of m:
 *   t = fl(fl(fl(m[k][0] r) + fl(m[k][1] g)) + fl(m[k][2] b)); t = min(max(t, 0), 1);
 *   out_k = lut_out[(int)fl(fl(t * 65535) + 0.5)]   (the conversion truncates). */
typedef struct MiToneMap {
    int32_t dst_pri;    /* Dav1dColorPrimaries of the output: 1 (BT.709), 9 (BT.2020), 12 (P3-D65) */
    int32_t dst_trc;    /* output OETF: 1 (BT.709) or 13 (sRGB) */
    int32_t dst_bpc;    /* output depth: 8, 10 or 12, independent of the source depth */
    float src_peak;     /* PQ sources: mastering peak Lw, nits (HLG sources: not read) */
    float dst_peak;     /* PQ sources: target peak Lmax, nits; linear light is normalised by it
                           (HLG sources: the nominal peak of the display the OOTF renders for) */
} MiToneMap;

/* Host only, no device and no context: the tables the device stage uses for a source of
 * `src_bpc` bits (8, 10, 12) described by color->pri and color->trc. lut_in receives
 * 1 << src_bpc floats, m 9, lut_out 65536 entries. -EINVAL for a NULL argument, a dst_pri,
 * dst_trc or dst_bpc outside the lists above, a src_bpc other than 8, 10, 12, pri or trc 2 or
 * reserved, and for PQ sources a peak that is not finite or lies outside [1, 10000] (other sources
 * do not read the peaks); -ENOTSUP for the other defined pri and trc values. */
int mi_tonemap_tables(const MiToneMap *tm, const MiColorInfo *color, int src_bpc,
                      float *lut_in, float m[9], uint16_t *lut_out);

/* mi_display_picture with the colour-volume stage: the RGB formats only (MI_OUT_SEMIPLANAR is
 * -ENOTSUP); out->bpc must equal tm->dst_bpc and need not equal in->bpc; the sample type follows
 * out->bpc (u8 at 8, else u16 LSB-aligned) and alpha is 2^dst_bpc - 1. The checks of
 * mi_display_picture (its colour-matrix rules included) and of mi_tonemap_tables apply, all before
 * any device work, the NULL `ctx` last. The context owns the device tables: they are rebuilt and
 * uploaded (on `stream`, without synchronising it) only when *tm, color->pri, color->trc or
 * in->bpc differ from the call before, and then only the tables that read what changed (a change of
 * the peaks alone rebuilds lut_in, not the 65536 entries of lut_out); calls on one context use one
 * stream, which orders a table change behind the kernels still reading the old tables. */
int mi_display_picture_tm(MiCtx *ctx, const MiPicture *in, const MiDisplayImage *out,
                          const MiColorInfo *color, const MiToneMap *tm,
                          const MiFilmGrainData *fg, void *stream);

/* mi_display_tensor with the colour-volume stage: the picture P of its definition is the
 * tone-mapped picture (MI_OUT_RGB_PLANAR of mi_display_picture_tm) and M is 2^dst_bpc - 1 (so
 * MI_T_U8 shifts by dst_bpc - 8); crop, resize and finish are otherwise as written there. */
int mi_display_tensor_tm(MiCtx *ctx, const MiPicture *in, const MiTensorImage *out,
                         const MiColorInfo *color, const MiToneMap *tm,
                         const MiFilmGrainData *fg, void *stream);

/* ---- HLG sources (librav1d_amd.so) -------------------------------------------------------- */

/* color->trc == 18 (HLG, BT.2100) as a source of the colour-volume stage, with any color->pri the
 * stage converts (the pri rules are unchanged). A context accepts it only after
 * mi_ctx_enable_hlg(ctx, 1): the flag is off in a new context, may be switched at any time between
 * calls, and a context with it off (and a NULL `ctx`) answers trc 18 with -ENOTSUP exactly as
 * before, so a caller that takes that answer as "convert it yourself" keeps getting it. Reading the
 * flag of a non-NULL `ctx` is part of the checks: they still all precede device work, and the NULL
 * `ctx` is still reported last. With the flag on, mi_display_picture_tm, mi_display_tensor_tm,
 * mi_display_tensor_rs, mi_display_yuv_tm and mi_display_scaled_tm accept trc 18; they are defined
 * through the picture P of mi_display_picture_tm as for every other source. -EINVAL for NULL `ctx`,
 * else 0.
 *
 * The destination is as above (dst_pri, dst_trc, dst_bpc). tm->dst_peak is the nominal peak Lw of
 * the display the picture is rendered for, finite and in [1, 10000], else -EINVAL. tm->src_peak is
 * not read (any value, NaN included): HLG is scene-referred, and a dimmer display is served by the
 * signal's own OOTF at that display's peak, so there is no EETF and no black lift (beta = 0).
 *
 * Tables, built on the host in double precision and rounded once:
 *   lut_in[v], v = 0 .. Ms, x = v / Ms: the scene-linear signal, the HLG inverse OETF
 *     E = x^2 / 3 for x <= 1/2, else min((exp((x - c) / a) + b) / 12, 1), a = 0.17883277,
 *     b = 1 - 4a, c = 0.5 - a ln(4a), under the rules of lut_in above (entry 0 exactly 0, the
 *     running maximum, a subnormal float32 becomes 0). It depends on the source depth alone.
 *   yw[3]: the float32 of the Y row of RGB->XYZ of color->pri (BT.2020: 0.2627, 0.6780, 0.0593;
 *     BT.2100 defines HLG on BT.2020, a stream with other primaries gets their own row).
 *   lut_gain[1538]: the OOTF gain Y^(gamma - 1), gamma = 1.2 * 1.111^log2(Lw / 1000) (BT.2100-2
 *     note 5, the extended range; 1.2 at 1000 nits). With U0 = 103 << 23 (the float32 bits of
 *     2^-24) and U1 = 127 << 23 (of 1.0), y_k is the float32 of bit pattern min(U0 + (k << 17), U1)
 *     and lut_gain[k] = float32(y_k^(gamma - 1)), k = 0 .. 1537: 64 nodes per octave over 24
 *     octaves, entries 1536 and 1537 both exactly 1.
 *   m[9] and lut_out are as above.
 * Per pixel on the device, every float32 operation rounded separately (no fused multiply-add):
 *   r = lut_in[R'], g = lut_in[G'], b = lut_in[B'];
 *   Y = fl(fl(fl(yw[0] r) + fl(yw[1] g)) + fl(yw[2] b));
 *   u = the bits of Y as an unsigned integer clamped to [U0, U1], d = u - U0, k = d >> 17,
 *   f = float(d & 0x1FFFF) * 2^-17 (both exact);
 *   gain = fl(lut_gain[k] + fl(f * fl(lut_gain[k + 1] - lut_gain[k])));
 *   r = fl(r * gain), g = fl(g * gain), b = fl(b * gain);
 *   then the rows of m, the clamp to [0, 1] (which also takes a channel that a gamma below 1 pushes
 *   above 1) and lut_out as above. Node and fraction are integer operations on the bits of Y: the
 *   device evaluates no transcendental, and the gain is linear in Y between nodes (within 2.8e-5
 *   relative of Y^(gamma - 1) at dst_peak 1, below 1e-5 from dst_peak 50; half a 12-bit code is
 *   1.2e-4). */
int mi_ctx_enable_hlg(MiCtx *ctx, int on);

/* Host only, no device and no context: mi_tonemap_tables for an HLG source, with the two tables it
 * adds (yw 3 floats, lut_gain 1538). The argument rules of mi_tonemap_tables apply; -EINVAL also
 * for a NULL yw or lut_gain, for a color->trc other than 18 and for a dst_peak that is not finite
 * or lies outside [1, 10000]. (mi_tonemap_tables itself has no context and keeps answering trc 18
 * with -ENOTSUP.) */
int mi_tonemap_tables_hlg(const MiToneMap *tm, const MiColorInfo *color, int src_bpc,
                          float *lut_in, float m[9], uint16_t *lut_out, float yw[3],
                          float *lut_gain /* 1538 */);

/* ---- scaled semi-planar output (librav1d_amd.so) ------------------------------------------ */

/* A shown picture as cropped, resized semi-planar YUV at a chosen depth, for an encoder on the
 * device (a transcode ladder: one call writes up to 8 rungs). The output keeps the source's chroma
 * subsampling and the storage of MI_OUT_SEMIPLANAR: data[0] = Y, data[1] = interleaved UV (NV12 /
 * NV16 / NV24; 4:0:0 writes Y only and does not read data[1]), u8 at 8 bpc, else u16 MSB-aligned
 * (v << (16 - bpc)). Only the w x h luma samples and the cw x ch UV pairs are written.
 *
 * sh, sv = the layout's subsampling shifts. The luma crop is crop_w x crop_h at (crop_x, crop_y),
 * crop_w == 0 and crop_h == 0 the whole picture (crop_x, crop_y are not read then); the chroma crop
 * is at (crop_x >> sh, crop_y >> sv) with extent ((crop_w + sh) >> sh, (crop_h + sv) >> sv), and the
 * chroma output extent is cw x ch = ((w + sh) >> sh, (h + sv) >> sv). So that the two crops cover
 * the same area, crop_x must be even with sh and crop_y with sv, and crop_w (crop_h) must be even
 * with sh (sv) unless the crop reaches the picture's right (bottom) edge.
 *
 * resize: every plane on its own, separable, the horizontal pass first, its result an integer in
 *   [0, Ms] (Ms = 2^in->bpc - 1) the vertical pass runs over; n_in the plane's crop extent, n_out
 *   its output extent on the axis, S = 18.
 *   Luma, and chroma on an axis that is not subsampled or whose samples are centred (every axis
 *   of 4:4:4, the vertical axis of 4:2:2, the vertical axis of 4:2:0 with chr 0 or 1): the formula
 *   of mi_display_tensor, Rr = 2 max(n_in, n_out), C = (2o+1) n_in, wt_i = Rr - |C - (2i+1) n_out|.
 *   Chroma on a co-sited axis (the horizontal axis of 4:2:0 and 4:2:2, the vertical axis of 4:2:0
 *   with chr == 2: the sitings the upsampler of the RGB formats assumes), where a chroma sample
 *   sits on the even luma sample, a quarter of a chroma sample left of (above) its centre:
 *   Rr = 4 max(n_in, n_out), C = (4o+1) n_in, wt_i = Rr - |C - (4i+1) n_out|.
 *   Both: the taps are the i with wt_i > 0; W = sum wt_i, k_i = (wt_i 2^S + W/2) / W (floor);
 *   2^S - sum k_i is added to the first tap with the largest wt_i; tap i reads crop sample
 *   clamp(i, 0, n_in - 1); out[o] = (sum k_i x_i + 2^(S-1)) >> S. n_in == n_out is the identity
 *   with either formula. A downscale above 64:1 on any plane axis (n_in > 64 n_out) is -EINVAL.
 * depth: v the vertical pass's integer at the source depth s, d = bpc of the rung, Md = 2^d - 1:
 *   d == s: v; d < s: min(Md, (v + 2^(s-d-1)) >> (s-d)); d > s: v << (d-s); then the store above.
 * color may be NULL; only color->chr is read (NULL: 0), and it is the siting of the output too.
 * With `fg`, film grain is applied once (mi_film_grain_frame, mtrx_identity = color &&
 * color->mtrx == 0) into the context's scratch picture and every rung reads that. Each rung is
 * defined from the (grained) source picture alone, never from another rung: a call with n_outs
 * rungs equals n_outs calls with one rung, bit for bit. 1:1 at the source depth without a crop is
 * MI_OUT_SEMIPLANAR of mi_display_picture. */
typedef struct MiScaledImage {
    void *data[2]; ptrdiff_t stride[2];   /* Y plane; interleaved UV plane (unused for 4:0:0) */
    int32_t w, h;                         /* output luma size */
    int32_t bpc;                          /* output depth 8, 10 or 12; need not equal in->bpc */
    int32_t crop_x, crop_y, crop_w, crop_h;  /* luma pixels of `in`; crop_w == crop_h == 0: whole picture */
} MiScaledImage;

/* Enqueue the n_outs (1..8) scaled outputs of `in` on `stream` (never synchronises); the context
 * owns the scratch (tap tables and the horizontal pass's result; allocated on first use, replaced
 * only when a call needs more; a call with the geometry of the one before reuses the tables).
 * Every check precedes any device work, the NULL `ctx` last: -EINVAL for NULL `in` / `outs`, a
 * malformed `in`, n_outs outside 1..8; per rung a NULL data[0], a NULL data[1] with a chroma
 * layout, w or h outside 1..65536, a bpc other than 8 / 10 / 12, a stride smaller than the row it
 * holds or not a multiple of the sample size, a pointer not aligned to the sample size, a crop
 * outside the picture or with one extent zero, an odd crop origin or extent as described above, a
 * downscale above 64:1 on any plane axis; color->chr outside 0..2. -ENOMEM and -EIO as above. */
int mi_display_scaled(MiCtx *ctx, const MiPicture *in, const MiScaledImage *outs, int n_outs,
                      const MiColorInfo *color, const MiFilmGrainData *fg, void *stream);

/* ---- resampling filters of the tensor and scaled outputs (librav1d_amd.so) ---------------- */

/* The filter of the resize of mi_display_tensor and mi_display_scaled: the triangle written there,
 * or a Mitchell-Netravali cubic (B, C) of radius 2, widened by the downscale ratio like the
 * triangle: (0, 0.5) is Catmull-Rom (Keys a = -0.5: PIL, torch with antialiasing), (0, 0.75) Keys
 * a = -0.75 (OpenCV, torch without antialiasing), (0, 0.6) swscale's default bicubic, (1/3, 1/3)
 * Mitchell. One filter applies to every rung and every plane of a call.
 *
 * MI_RS_CUBIC replaces the resize step of those definitions; crop, sitings, finish, depth and
 * stores stay. Per axis (n_in the crop extent, n_out the output extent, S = 18, P the phase: 2 on a
 * centred axis, 4 on a co-sited one, chosen as written at mi_display_scaled):
 *   n_in == n_out is the identity for every filter: start = o, one tap of 2^S (so B > 0 does not
 *   blur an axis that is not resized). Otherwise, in exact integers, Rr = P max(n_in, n_out),
 *   C = (P o + 1) n_in, d_i = |C - (P i + 1) n_out|; the taps are every i with d_i < 2 Rr (at most
 *   4 ceil(max(n_in, n_out) / n_out) + 1 of them); tap i reads crop sample clamp(i, 0, n_in - 1).
 *   Weights, in float64, every operation rounded on its own in the order written (no fused
 *   multiply-add), b and c the float32 members widened to double: t = d_i / Rr,
 *     w_i = ((p3 t + p2) t + p1) t + p0, with
 *     d_i < Rr:  p3 = 12 - 9 b - 6 c, p2 = -18 + 12 b + 6 c, p1 = 0, p0 = 6 - 2 b;
 *     otherwise: p3 = -b - 6 c, p2 = 6 b + 30 c, p1 = -12 b - 48 c, p0 = 8 b + 24 c
 *   (each coefficient evaluated left to right: (12 - 9 b) - 6 c, ((-18) + 12 b) + 6 c, (-b) - 6 c, ...;
 *   six times the usual kernel: the normalisation removes the factor).
 *   W = the sum of the w_i in ascending i; k_i = floor(w_i / W * 2^S + 0.5) (the quotient first);
 *   2^S - sum k_i is added to the first tap with the largest w_i. A weight that is zero inside the
 *   support stays a tap; slots j >= count hold zero.
 *   Each pass: out[o] = clamp((sum k_i x_i + 2^(S-1)) >> S, 0, M), an arithmetic shift of the
 *   signed sum, M = 2^depth - 1 of the samples the pass runs over (Ms for the scaled planes, the
 *   tone-mapped depth for a tensor with `tm`). The horizontal pass's clamped integer is what the
 *   vertical pass reads. sum |k_i| <= 1.54 * 2^S for every (b, c) in [0, 1]^2 and every size the
 *   64:1 limit admits, so 32-bit sums hold at 12 bits. */
enum { MI_RS_TRIANGLE = 0, MI_RS_CUBIC = 1 };
typedef struct MiResample { int32_t filter; float b, c; } MiResample;   /* b, c: Mitchell-Netravali, read for MI_RS_CUBIC only */

/* mi_display_tensor (tm NULL: no colour-volume stage) or mi_display_tensor_tm with the filter
 * `rs`. rs == NULL or MI_RS_TRIANGLE is exactly that call: the same kernels, the same output bit
 * for bit. Their checks apply; in addition -EINVAL for a filter outside the list and, for
 * MI_RS_CUBIC, a b or c that is not finite or lies outside [0, 1]. Every check precedes any device
 * work, the NULL `ctx` last. The 64:1 limit stays. The context's tap tables are reused only by a
 * call with the same geometry and the same filter, b and c. */
int mi_display_tensor_rs(MiCtx *ctx, const MiPicture *in, const MiTensorImage *out, const MiColorInfo *color,
                         const MiToneMap *tm, const MiResample *rs, const MiFilmGrainData *fg, void *stream);
/* mi_display_scaled with the filter `rs`, by the same rules. */
int mi_display_scaled_rs(MiCtx *ctx, const MiPicture *in, const MiScaledImage *outs, int n_outs,
                         const MiColorInfo *color, const MiResample *rs, const MiFilmGrainData *fg, void *stream);

/* Host only, no device and no context: the sizes the device passes use for an axis n_in -> n_out
 * under `rs` (NULL: the triangle). *cap: the slots per output of its tap table; *seg_outputs: the
 * output columns one workgroup of the horizontal pass takes, sized so that the source columns their
 * taps reach, with the 15 the 8-column runs of the tile spend, fit 2048. -EINVAL for a NULL `cap`
 * or `seg_outputs`, a bad `rs`, n_in or n_out outside 1..65536, n_in > 64 n_out. */
int mi_resample_plan(const MiResample *rs, int n_in, int n_out, int *cap, int *seg_outputs);
/* Host only: the tap table of the axis, from the source the device's table kernel runs: output o
 * reads crop sample clamp(start[o] + j, 0, n_in - 1) with weight k[j * n_out + o], j < count[o];
 * slots count[o] <= j < cap hold zero. phase: 2 centred, 4 co-sited. -EINVAL as mi_resample_plan,
 * for a NULL table, a phase other than 2 and 4, and a `cap` below mi_resample_plan's. */
int mi_resample_taps(const MiResample *rs, int n_in, int n_out, int phase, int cap,
                     int32_t *start, int32_t *count, int32_t *k /* [cap][n_out] */);

/* ---- tone-mapped YUV output (librav1d_amd.so) ---------------------------------------------- */

/* The colour-volume stage with a Y'CbCr result, for an encoder on the device: an HDR10 source to
 * SDR semi-planar YUV, 1:1 (mi_display_yuv_tm) or as the rungs of a ladder (mi_display_scaled_tm).
 * Both are defined through the picture Q:
 *
 * P is the w x h R'G'B' picture mi_display_picture_tm gives as MI_OUT_RGB_PLANAR for the same
 * `in`, `color`, `tm` and `fg` (the upsampler, the matrix of color->mtrx, identity and 4:0:0
 * included, the stage; film grain applied once, to the source, before all of it).
 * d = tm->dst_bpc, Md = 2^d - 1, H = 2^(d-1), S = 14. The target is MiYuvTarget: mtrx one of 1, 4,
 * 5, 6, 7, 9 with the Kr, Kb of the inverse direction above; range 0 (limited) or 1 (full). Q has
 * the source's layout (sh, sv the subsampling shifts), depth d, and chroma size cw x ch =
 * ((w + sh) >> sh, (h + sv) >> sv). A source with color->mtrx == 0 (GBR, 4:4:4) is a valid source:
 * Q carries the target's matrix.
 *
 * Forward matrix, at full resolution on the integers of P. Kg = 1 - Kr - Kb; limited: Yo =
 * 16 << (d-8), sy = (219 << (d-8)) / Md, sc = (224 << (d-8)) / Md; full: Yo = 0, sy = sc = 1. The
 * coefficients are computed on the host in double precision and rounded once (round(x) =
 * floor(x + 0.5)):
 *   yr = round(2^S Kr sy), yb = round(2^S Kb sy), yg = round(2^S sy) - yr - yb;
 *   ur = -round(2^S sc Kr / (2 (1-Kb))), ug = -round(2^S sc Kg / (2 (1-Kb))), ub = -(ur + ug);
 *   vg = -round(2^S sc Kg / (2 (1-Kr))), vb = -round(2^S sc Kb / (2 (1-Kr))), vr = -(vg + vb);
 * so grey maps to chroma H exactly and white to the top of the luma range.
 *   Y  = clip(((yr R + yg G + yb B + 2^(S-1)) >> S) + Yo, 0, Md)
 *   U4 = clip(((ur R + ug G + ub B + 2^(S-1)) >> S) + H, 0, Md)
 *   V4 = clip(((vr R + vg G + vb B + 2^(S-1)) >> S) + H, 0, Md)
 * (an arithmetic shift of a signed 32-bit sum, which fits: three coefficients of at most 2^14
 * times 4095).
 *
 * Chroma decimation of U4 and V4 (w x h each) to cw x ch: one 2-D integer filter per output sample
 * (i, j), rounded once, indices clamped, so no pass order is implied.
 *   horizontal, 4:2:0 and 4:2:2 (co-sited, the siting the upsampler and mi_display_scaled assume):
 *     weights (1, 2, 1) on columns max(2i-1, 0), 2i, min(2i+1, w-1);
 *   vertical, 4:2:0, chr == 2 (co-located): (1, 2, 1) on rows max(2j-1, 0), 2j, min(2j+1, h-1);
 *   vertical, 4:2:0, chr 0 or 1 (centred): (1, 1) on rows 2j, min(2j+1, h-1);
 *   an axis that is not subsampled: weight 1 on its own sample.
 *   C[j][i] = (sum wx wy C4[row][column] + W/2) >> log2(W), W = sum wx wy (2, 4, 8 or 16).
 * 4:4:4: U = U4, V = V4. 4:0:0: Q has Y only (R = G = B comes out of the matrix, and the stage
 * still runs on it). */
typedef struct MiYuvTarget { int32_t mtrx, range; } MiYuvTarget;

/* Enqueue Q on `stream` (never synchronises) in the storage of MI_OUT_SEMIPLANAR: out->format must
 * be MI_OUT_SEMIPLANAR and out->bpc == tm->dst_bpc; data[0] = Y, data[1] = interleaved UV at the
 * source's subsampling (not read for 4:0:0), u8 at 8 bits, else u16 MSB-aligned. Only the w x h
 * luma samples and the cw x ch UV pairs are written, straight from the kernel that computes them.
 * The checks of mi_display_picture_tm apply (its colour-matrix rules for the source, the rules of
 * the stage: -ENOTSUP for the pri and trc values listed there), all before any device work, the NULL
 * `ctx` last; in addition -EINVAL for NULL `tm` or `target`, a target->mtrx outside the list (0, 2,
 * 8, 10 - 14 and reserved values alike: the caller chooses the output, nothing is unsupported on
 * the source's behalf), a target->range outside 0 / 1, an out->format other than
 * MI_OUT_SEMIPLANAR, out->bpc != tm->dst_bpc, NULL data[1] with a chroma layout. */
int mi_display_yuv_tm(MiCtx *ctx, const MiPicture *in, const MiDisplayImage *out,
                      const MiColorInfo *color, const MiToneMap *tm, const MiYuvTarget *target,
                      const MiFilmGrainData *fg, void *stream);

/* mi_display_scaled_rs(ctx, Q, outs, n_outs, color, rs, NULL, stream), bit for bit: Q a planar
 * picture of depth d in a scratch the context owns (allocated on first use, replaced only when a
 * call needs more, shared with no other scratch), written by one kernel in front of the scaled
 * passes on the same stream. Ms of the scaled definition is Md and a rung's bpc converts from d;
 * `color` as passed (the scaled passes read its chr, the siting of Q and of the rungs). The checks
 * are those of mi_display_scaled_rs and of mi_display_yuv_tm's source, tone map and target, all
 * before any device work, the NULL `ctx` last. */
int mi_display_scaled_tm(MiCtx *ctx, const MiPicture *in, const MiScaledImage *outs, int n_outs,
                         const MiColorInfo *color, const MiToneMap *tm, const MiYuvTarget *target,
                         const MiResample *rs, const MiFilmGrainData *fg, void *stream);

/* ---- light level of a picture (librav1d_amd.so) ------------------------------------------- */

/* What src_peak to give the colour-volume stage for a stream that carries no metadata, or whose
 * container is wider than its content: measured from the decoded planes on the device.
 *
 * Let P be the planar R'G'B' picture mi_display_picture writes for `in` and `color` with
 * MI_OUT_RGB_PLANAR, bpc = in->bpc and no film grain (the chroma upsampler and the 14-bit matrix
 * stated there). Then
 *   hist[c] = the number of pixels of P with max(R, G, B) == c, c = 0 .. 2^bpc - 1.
 * `hist` is device memory of 1 << bpc uint32_t. The entry zeroes it on `stream` and then counts,
 * never synchronising; the counts are integers, so the result does not depend on the order of
 * the additions. Film grain is deliberately not applied: it is noise the tone curve should not
 * follow, and the measurement is cheaper without it. The whole picture is measured (no crop, no
 * active-area detection).
 * Every check precedes any device work: -EINVAL for a NULL or malformed `in`, NULL `hist`,
 * w * h >= 2^32, and the colour rules of mi_display_picture for an RGB format (NULL `color`, mtrx 2
 * or reserved, a bad range, identity without 4:4:4; -ENOTSUP for matrices 8 and 10-14), the NULL
 * `ctx` last; -EIO. */
int mi_picture_light_level(MiCtx *ctx, const MiPicture *in, const MiColorInfo *color, uint32_t *hist, void *stream);
/* Diagnostic (tools/light_bench.py): the same result through the counting `variant` of
 * csrc/light.hip (0 one LDS atomic per pixel, 1 equal neighbours of a lane combined, 2 a uniform
 * wave combined as well: the entry above); -EINVAL for any other. */
int mi_picture_light_level_variant(MiCtx *ctx, const MiPicture *in, const MiColorInfo *color, uint32_t *hist,
                                   int variant, void *stream);

/* Host only, no device and no context: the statistics of a histogram of `bpc` bits (8, 10, 12; host
 * memory of 1 << bpc counts) whose codes are read as full-range PQ (ST 2084: the caller uses it for
 * trc 16 only). nits(c) = EOTF(c / (2^bpc - 1)) with the EOTF of the colour-volume stage above;
 * N = sum hist[c].
 *   max_code: the highest c with hist[c] != 0; max_nits = nits(max_code).
 *   pct_code: the lowest c with hist[0] + .. + hist[c] >= ceil(percentile / 100 * N), the product in
 *     double; pct_nits = nits(pct_code).
 *   avg_nits: sum hist[c] nits(c) / N, summed in double in increasing c: the picture's frame-average
 *     light level in the CTA-861.3 sense, over the whole picture.
 * -EINVAL for a NULL argument, a bpc outside the list, a percentile outside (0, 100] and N == 0. */
typedef struct MiLightLevel { int32_t max_code, pct_code; double max_nits, pct_nits, avg_nits; } MiLightLevel;
int mi_light_level_stats(const uint32_t *hist, int bpc, double percentile, MiLightLevel *out);

#ifdef __cplusplus
}
#endif
#endif /* MI_AV1OUT_H */
