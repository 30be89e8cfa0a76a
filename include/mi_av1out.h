/*
 * mi_av1out.h — the output side of the decode path: displayed pictures from the device to the
 * host (film grain fused with the copy) and the reference's output muxers.
 *
 * Two libraries implement it:
 *   - librav1d_amd.so (gfx950): mi_host_picture_alloc / _free, mi_output_picture, and the
 *     output that stays on the device, mi_display_picture and mi_display_tensor;
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
 * transfer-function or primaries conversion: the output is R'G'B' in the stream's primaries. */
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

#ifdef __cplusplus
}
#endif
#endif /* MI_AV1OUT_H */
