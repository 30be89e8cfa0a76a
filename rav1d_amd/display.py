"""Device display output (include/mi_av1out.h, mi_display_picture): a shown picture as a tight
torch tensor on the device, semi-planar YUV (NV12 / P010 and their 4:2:2 / 4:4:4 kin) or R'G'B'
(planar, or packed with alpha), with film grain applied. torch allocates; the conversion is the
gfx950 kernel of csrc/display.hip. display_tensor (mi_display_tensor, csrc/tensor.hip) writes the
cropped, resized, normalised R'G'B' tensor an ML consumer reads. With a ToneMap both go through the
colour-volume stage (mi_display_picture_tm / mi_display_tensor_tm: inverse transfer and, for PQ, the
BT.2390 tone curve, primaries conversion, the destination's OETF at a chosen depth) in the same pass.
display_scaled (mi_display_scaled, csrc/scaled.hip) writes cropped, resized semi-planar YUV at a
chosen depth, several sizes per call: the rungs of a transcode ladder. Both resize with the
triangle filter, or with resample=Resample(...) (mi_display_tensor_rs / mi_display_scaled_rs) with a
Mitchell-Netravali cubic: Catmull-Rom, Mitchell, Keys a = -0.75 or any (B, C) in [0, 1]^2.
display_yuv (mi_display_yuv_tm, csrc/yuv_tm.hip) and display_scaled with a ToneMap
(mi_display_scaled_tm) write the tone-mapped picture as semi-planar YUV in a YuvTarget's matrix and
range: an HDR10 source as the SDR picture, or the SDR ladder, an encoder takes."""
import ctypes

import numpy as np
import torch

from . import MiFilmGrainData, MiPicture, check, lib
from .av1dec import MiColorInfo
from .frame import _stream_ptr, film_grain_data

OUT_SEMIPLANAR, OUT_RGB_PLANAR, OUT_RGBA_PACKED = 0, 1, 2
FORMATS = {"nv12": OUT_SEMIPLANAR, "rgb": OUT_RGB_PLANAR, "rgba": OUT_RGBA_PACKED}

# Dav1dMatrixCoefficients of the matrices mi_display_picture converts
MC_IDENTITY, MC_BT709, MC_UNKNOWN, MC_FCC, MC_BT470BG, MC_BT601, MC_SMPTE240, MC_BT2020_NCL = 0, 1, 2, 4, 5, 6, 7, 9


class MiDisplayImage(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p * 3), ("stride", ctypes.c_ssize_t * 3),
                ("w", ctypes.c_int32), ("h", ctypes.c_int32), ("format", ctypes.c_int32), ("bpc", ctypes.c_int32)]


class DisplayImage:
    """The destination of display_picture for a w x h picture of `bpc` bits and pixel `layout`
    (0 I400 .. 3 I444). Samples are uint8 at 8 bpc, else 16-bit words held in int16 storage
    (view them as uint16 on the host: numpy()). format "nv12" (or 0): `y` (h, w) and `uv`
    (ch, cw, 2) at the layout's own subsampling (None for 4:0:0), 10 / 12-bit samples MSB-aligned;
    "rgb" (1): `rgb` (3, h, w); "rgba" (2): `rgba` (h, w, 4), alpha 2^bpc - 1; RGB samples are
    full range at the source bit depth, LSB-aligned. out_bpc: the depth of the samples when it
    differs from the picture's (a tone-mapped RGB destination: ToneMap.dst_bpc); `bpc` is then
    that depth."""

    def __init__(self, w, h, bpc, layout, format, device="cuda", out_bpc=None):
        bpc = bpc if out_bpc is None else int(out_bpc)
        self.w, self.h, self.bpc, self.layout = w, h, bpc, layout
        self.format = FORMATS[format] if isinstance(format, str) else int(format)
        if self.format not in FORMATS.values():
            raise ValueError(f"format {format!r}")
        dt = torch.uint8 if bpc == 8 else torch.int16
        ss_hor, ss_ver = int(layout in (1, 2)), int(layout == 1)
        self.cw, self.ch = (w + ss_hor) >> ss_hor, (h + ss_ver) >> ss_ver
        self.y = self.uv = self.rgb = self.rgba = None
        if self.format == OUT_SEMIPLANAR:
            self.y = torch.zeros((h, w), dtype=dt, device=device)
            if layout:
                self.uv = torch.zeros((self.ch, self.cw, 2), dtype=dt, device=device)
        elif self.format == OUT_RGB_PLANAR:
            self.rgb = torch.zeros((3, h, w), dtype=dt, device=device)
        else:
            self.rgba = torch.zeros((h, w, 4), dtype=dt, device=device)

    def tensors(self):
        return [t for t in (self.y, self.uv, self.rgb, self.rgba) if t is not None]

    def image(self):
        """The MiDisplayImage over the tensors."""
        im = MiDisplayImage()
        im.w, im.h, im.format, im.bpc = self.w, self.h, self.format, self.bpc
        pxb = 1 if self.bpc == 8 else 2
        if self.format == OUT_SEMIPLANAR:
            im.data[0], im.stride[0] = self.y.data_ptr(), self.w * pxb
            if self.uv is not None:
                im.data[1], im.stride[1] = self.uv.data_ptr(), 2 * self.cw * pxb
        elif self.format == OUT_RGB_PLANAR:
            for p in range(3):
                im.data[p], im.stride[p] = self.rgb[p].data_ptr(), self.w * pxb
        else:
            im.data[0], im.stride[0] = self.rgba.data_ptr(), 4 * self.w * pxb
        return im

    def numpy(self):
        """Host copies of the tensors as unsigned samples, in tensors() order."""
        out = []
        for t in self.tensors():
            a = t.cpu().numpy()
            out.append(a.view("<u2") if self.bpc > 8 else a)
        return out


class MiToneMap(ctypes.Structure):
    _fields_ = [("dst_pri", ctypes.c_int32), ("dst_trc", ctypes.c_int32), ("dst_bpc", ctypes.c_int32),
                ("src_peak", ctypes.c_float), ("dst_peak", ctypes.c_float)]


def ToneMap(dst_pri=1, dst_trc=13, dst_bpc=8, src_peak=1000.0, dst_peak=100.0):
    """A MiToneMap: the output's primaries (1 BT.709, 9 BT.2020, 12 P3-D65), OETF (1 BT.709,
    13 sRGB) and depth (8, 10, 12), and for PQ sources the mastering and the target peak in nits.
    For HLG sources (enable_hlg) dst_peak is the nominal peak of the display the picture is rendered
    for and src_peak is not read. The defaults take HDR10 to 8-bit sRGB at 100 nits."""
    return MiToneMap(int(dst_pri), int(dst_trc), int(dst_bpc), float(src_peak), float(dst_peak))


def tonemap_tables(tm, color, src_bpc):
    """mi_tonemap_tables (host only): (lut_in float32 [1 << src_bpc], m float32 [3, 3],
    lut_out uint16 [65536]), the tables the device stage uses for a source of `src_bpc` bits
    described by color.pri and color.trc. Raises MiError on a negative return."""
    lut_in = np.empty(1 << src_bpc if src_bpc in (8, 10, 12) else 1, dtype=np.float32)
    m = np.empty(9, dtype=np.float32)
    lut_out = np.empty(65536, dtype=np.uint16)
    check(lib().mi_tonemap_tables(ctypes.byref(tm) if tm is not None else None,
                                  ctypes.byref(color) if color is not None else None, int(src_bpc),
                                  lut_in.ctypes.data_as(ctypes.c_void_p), m.ctypes.data_as(ctypes.c_void_p),
                                  lut_out.ctypes.data_as(ctypes.c_void_p)), "mi_tonemap_tables")
    return lut_in, m.reshape(3, 3), lut_out


GAIN_NODES = 1538   # entries of lut_gain


def enable_hlg(ctx, on=True):
    """mi_ctx_enable_hlg: let `ctx` take HLG sources (color.trc 18) in display_picture,
    display_tensor, display_yuv and display_scaled with a ToneMap, whose dst_peak is then the
    nominal peak of the display the picture is rendered for (src_peak is not read). Off in a new
    context; a context with it off answers trc 18 with ENOTSUP. Raises MiError on a negative
    return."""
    check(lib().mi_ctx_enable_hlg(ctx.h if ctx is not None else None, 1 if on else 0), "mi_ctx_enable_hlg")


def tonemap_tables_hlg(tm, color, src_bpc):
    """mi_tonemap_tables_hlg (host only): (lut_in float32 [1 << src_bpc], m float32 [3, 3],
    lut_out uint16 [65536], yw float32 [3], lut_gain float32 [1538]), the tables the device stage
    uses for an HLG source (color.trc 18) of `src_bpc` bits with the primaries color.pri, rendered
    for a display of tm.dst_peak nits. Raises MiError on a negative return."""
    lut_in = np.empty(1 << src_bpc if src_bpc in (8, 10, 12) else 1, dtype=np.float32)
    m = np.empty(9, dtype=np.float32)
    lut_out = np.empty(65536, dtype=np.uint16)
    yw = np.empty(3, dtype=np.float32)
    lut_gain = np.empty(GAIN_NODES, dtype=np.float32)
    check(lib().mi_tonemap_tables_hlg(ctypes.byref(tm) if tm is not None else None,
                                      ctypes.byref(color) if color is not None else None, int(src_bpc),
                                      *(a.ctypes.data_as(ctypes.c_void_p) for a in (lut_in, m, lut_out, yw, lut_gain))),
          "mi_tonemap_tables_hlg")
    return lut_in, m.reshape(3, 3), lut_out, yw, lut_gain


def _source_args(frame, color, fg):
    """What every display call passes for its source: (the MiPicture of `frame`, a device Frame or a
    MiPicture; the pointer to `color` or None; the pointer to the MiFilmGrainData of `fg`, itself
    or a make_fg_params dict, or None)."""
    src = frame if isinstance(frame, MiPicture) else frame.picture()
    if fg is not None and not isinstance(fg, MiFilmGrainData):
        fg = film_grain_data(fg)
    return src, ctypes.byref(color) if color is not None else None, ctypes.byref(fg) if fg is not None else None


def display_picture(ctx, frame, image, color=None, fg=None, stream=None, tonemap=None):
    """Enqueue mi_display_picture: `frame` (a device Frame or a MiPicture) into `image` (a
    DisplayImage or a MiDisplayImage), with film grain when `fg` (a MiFilmGrainData or a
    make_fg_params dict). color: a MiColorInfo, needed by the RGB formats (its mtrx picks the
    matrix, range the scaling, chr the 4:2:0 chroma siting). tonemap: a MiToneMap (ToneMap()):
    the call is mi_display_picture_tm, color.pri and color.trc describe the source, and `image`
    holds samples of tonemap.dst_bpc bits (DisplayImage(..., out_bpc=)). Raises MiError on a
    negative return."""
    src, cp, fp = _source_args(frame, color, fg)
    im = image if isinstance(image, MiDisplayImage) else image.image()
    if tonemap is not None:
        check(lib().mi_display_picture_tm(ctx.h, ctypes.byref(src), ctypes.byref(im), cp, ctypes.byref(tonemap), fp,
                                          _stream_ptr(stream)), "mi_display_picture_tm")
        return
    check(lib().mi_display_picture(ctx.h, ctypes.byref(src), ctypes.byref(im), cp, fp, _stream_ptr(stream)),
          "mi_display_picture")


RS_TRIANGLE, RS_CUBIC = 0, 1


class MiResample(ctypes.Structure):
    _fields_ = [("filter", ctypes.c_int32), ("b", ctypes.c_float), ("c", ctypes.c_float)]


# named filters: (MI_RS_*, B, C)
RESAMPLE_PRESETS = {"triangle": (RS_TRIANGLE, 0.0, 0.0), "catmull_rom": (RS_CUBIC, 0.0, 0.5),
                    "mitchell": (RS_CUBIC, 1.0 / 3.0, 1.0 / 3.0), "cubic_075": (RS_CUBIC, 0.0, 0.75)}


def Resample(filter="cubic", b=0.0, c=0.5):
    """A MiResample: the filter of display_tensor's and display_scaled's resize. "cubic" takes the
    Mitchell-Netravali (b, c), each in [0, 1] (the default is Catmull-Rom); the presets fix them:
    "catmull_rom" (0, 0.5: Keys a = -0.5, what PIL and torch with antialiasing use), "mitchell"
    (1/3, 1/3), "cubic_075" (0, 0.75: Keys a = -0.75, OpenCV and torch without antialiasing) and
    "triangle", the filter of the calls without a MiResample."""
    if filter == "cubic":
        return MiResample(RS_CUBIC, float(b), float(c))
    if filter not in RESAMPLE_PRESETS:
        raise ValueError(f"filter {filter!r}: want 'cubic' or one of {sorted(RESAMPLE_PRESETS)}")
    return MiResample(*RESAMPLE_PRESETS[filter])


def resample_plan(rs, n_in, n_out):
    """mi_resample_plan (host only): (cap, seg_outputs) of the axis n_in -> n_out under `rs` (a
    MiResample, or None for the triangle): the slots per output of its tap table, and the output
    columns one workgroup of the horizontal pass takes. Raises MiError on a negative return."""
    cap, seg = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().mi_resample_plan(ctypes.byref(rs) if rs is not None else None, int(n_in), int(n_out),
                                 ctypes.byref(cap), ctypes.byref(seg)), "mi_resample_plan")
    return cap.value, seg.value


def resample_taps(rs, n_in, n_out, phase=2):
    """mi_resample_taps (host only): (start int32 [n_out], count int32 [n_out], k int32
    [cap, n_out]), the tap table the device builds for the axis n_in -> n_out under `rs` (None: the
    triangle) with phase 2 (centred) or 4 (co-sited): output o reads sample
    clamp(start[o] + j, 0, n_in - 1) with weight k[j, o]. Raises MiError on a negative return."""
    cap, _ = resample_plan(rs, n_in, n_out)
    start = np.empty(n_out, dtype=np.int32)
    count = np.empty(n_out, dtype=np.int32)
    k = np.empty((cap, n_out), dtype=np.int32)
    check(lib().mi_resample_taps(ctypes.byref(rs) if rs is not None else None, int(n_in), int(n_out), int(phase), cap,
                                 start.ctypes.data_as(ctypes.c_void_p), count.ctypes.data_as(ctypes.c_void_p),
                                 k.ctypes.data_as(ctypes.c_void_p)), "mi_resample_taps")
    return start, count, k


T_U8, T_F16, T_BF16, T_F32 = 0, 1, 2, 3
_TENSOR_DTYPES = {torch.uint8: T_U8, torch.float16: T_F16, torch.bfloat16: T_BF16, torch.float32: T_F32}


class MiTensorImage(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("stride", ctypes.c_ssize_t * 3),
                ("w", ctypes.c_int32), ("h", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("crop_x", ctypes.c_int32), ("crop_y", ctypes.c_int32), ("crop_w", ctypes.c_int32),
                ("crop_h", ctypes.c_int32), ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3)]


def tensor_image(out, bpc, crop=None, mean=None, std=None, channels_last=False):
    """The MiTensorImage over `out`, a (3, H, W) tensor in any strides (or (H, W, 3) with
    channels_last) of dtype uint8, float16, bfloat16 or float32, for a frame of `bpc` bits:
    scale[c] = float32(1 / (M std[c])), bias[c] = float32(-mean[c] / std[c]), M = 2^bpc - 1,
    computed in Python floats and rounded once. crop: (x, y, w, h) in luma pixels, or None."""
    if out.dim() != 3 or out.shape[2 if channels_last else 0] != 3:
        raise ValueError(f"out of shape {tuple(out.shape)}: want {'(H, W, 3)' if channels_last else '(3, H, W)'}")
    if out.dtype not in _TENSOR_DTYPES:
        raise ValueError(f"out of dtype {out.dtype}")
    if channels_last:
        out = out.permute(2, 0, 1)
    im = MiTensorImage()
    es = out.element_size()
    im.data, im.dtype = out.data_ptr(), _TENSOR_DTYPES[out.dtype]
    im.h, im.w = out.shape[1], out.shape[2]
    for i in range(3):
        # (a dimension of size 1 may carry any stride; none of its steps is ever taken)
        im.stride[i] = out.stride(i) * es if out.shape[i] > 1 and out.stride(i) > 0 else es
    if crop is not None:
        im.crop_x, im.crop_y, im.crop_w, im.crop_h = (int(v) for v in crop)
    mean = (0.0, 0.0, 0.0) if mean is None else tuple(float(v) for v in mean)
    std = (1.0, 1.0, 1.0) if std is None else tuple(float(v) for v in std)
    m = float((1 << bpc) - 1)
    for c in range(3):
        im.scale[c] = 1.0 / (m * std[c])
        im.bias[c] = -mean[c] / std[c]
    return im


def display_tensor(ctx, frame, out, color, fg=None, crop=None, mean=None, std=None, stream=None, channels_last=False,
                   tonemap=None, resample=None):
    """Enqueue mi_display_tensor: `frame` (a device Frame or a MiPicture) cropped to `crop`
    ((x, y, w, h) in luma pixels; None: the whole picture), resized to the size of `out` and
    normalised, as R'G'B' into `out`: a device tensor of shape (3, H, W) in any strides (batch[n] of
    an NCHW or a channels-last batch), or (H, W, 3) with channels_last; dtype and strides are the
    tensor's. Float dtypes receive (v / M - mean[c]) / std[c] (defaults 0 and 1: [0, 1]), uint8
    the sample at 8 bits. color: a MiColorInfo, as for display_picture's RGB formats; fg: film
    grain. `out` may also be a ready MiTensorImage. tonemap: a MiToneMap (ToneMap()): the call is
    mi_display_tensor_tm, the resized picture is the tone-mapped one and M is 2^dst_bpc - 1.
    resample: a MiResample (Resample()): the call is mi_display_tensor_rs and the resize uses that
    filter; None calls the entries without one (the triangle). Raises MiError on a negative return."""
    src, cp, fp = _source_args(frame, color, fg)
    bpc = src.bpc if tonemap is None else tonemap.dst_bpc
    im = out if isinstance(out, MiTensorImage) else tensor_image(out, bpc, crop, mean, std, channels_last)
    if resample is not None:
        check(lib().mi_display_tensor_rs(ctx.h, ctypes.byref(src), ctypes.byref(im), cp,
                                         ctypes.byref(tonemap) if tonemap is not None else None, ctypes.byref(resample),
                                         fp, _stream_ptr(stream)), "mi_display_tensor_rs")
        return
    if tonemap is not None:
        check(lib().mi_display_tensor_tm(ctx.h, ctypes.byref(src), ctypes.byref(im), cp, ctypes.byref(tonemap), fp,
                                         _stream_ptr(stream)), "mi_display_tensor_tm")
        return
    check(lib().mi_display_tensor(ctx.h, ctypes.byref(src), ctypes.byref(im), cp, fp, _stream_ptr(stream)),
          "mi_display_tensor")


class MiScaledImage(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p * 2), ("stride", ctypes.c_ssize_t * 2),
                ("w", ctypes.c_int32), ("h", ctypes.c_int32), ("bpc", ctypes.c_int32),
                ("crop_x", ctypes.c_int32), ("crop_y", ctypes.c_int32), ("crop_w", ctypes.c_int32),
                ("crop_h", ctypes.c_int32)]


def even_crop(crop, w, h, layout):
    """`crop` ((x, y, cw, ch) in luma pixels of a w x h picture) moved onto the chroma grid of
    `layout`, as mi_display_scaled asks: an odd origin on a subsampled axis goes one luma sample
    left (up) and the extent grows by it, and an odd extent that does not reach the picture's edge
    grows by one sample (it always fits: the edge it would pass is the odd one it may reach)."""
    x, y, cw, ch = (int(v) for v in crop)
    if layout in (1, 2):
        cw, x = cw + (x & 1), x & ~1
        if cw & 1 and x + cw != w:
            cw += 1
    if layout == 1:
        ch, y = ch + (y & 1), y & ~1
        if ch & 1 and y + ch != h:
            ch += 1
    return x, y, cw, ch


class ScaledImage:
    """One rung of display_scaled: a w x h semi-planar destination of `bpc` bits for a picture of
    pixel `layout` (0 I400 .. 3 I444): `y` (h, w) and `uv` (ch, cw, 2) at the layout's own
    subsampling (None for 4:0:0), uint8 at 8 bpc, else 16-bit words MSB-aligned held in int16
    storage (view them as uint16 on the host: numpy()). crop: (x, y, w, h) in luma pixels of the
    source, or None for the whole picture."""

    def __init__(self, w, h, bpc, layout, crop=None, device="cuda"):
        self.w, self.h, self.bpc, self.layout = int(w), int(h), int(bpc), layout
        self.crop = None if crop is None else tuple(int(v) for v in crop)
        dt = torch.uint8 if self.bpc == 8 else torch.int16
        ss_hor, ss_ver = int(layout in (1, 2)), int(layout == 1)
        self.cw, self.ch = (self.w + ss_hor) >> ss_hor, (self.h + ss_ver) >> ss_ver
        self.y = torch.zeros((self.h, self.w), dtype=dt, device=device)
        self.uv = torch.zeros((self.ch, self.cw, 2), dtype=dt, device=device) if layout else None

    def tensors(self):
        """(Y (h, w), UV (ch, cw, 2) or None)."""
        return self.y, self.uv

    def image(self):
        """The MiScaledImage over the tensors."""
        im = MiScaledImage()
        im.w, im.h, im.bpc = self.w, self.h, self.bpc
        pxb = 1 if self.bpc == 8 else 2
        im.data[0], im.stride[0] = self.y.data_ptr(), self.w * pxb
        if self.uv is not None:
            im.data[1], im.stride[1] = self.uv.data_ptr(), 2 * self.cw * pxb
        if self.crop is not None:
            im.crop_x, im.crop_y, im.crop_w, im.crop_h = self.crop
        return im

    def numpy(self):
        """Host copies of the tensors as unsigned samples: [Y] or [Y, UV]."""
        out = []
        for t in self.tensors():
            if t is not None:
                a = t.cpu().numpy()
                out.append(a.view("<u2") if self.bpc > 8 else a)
        return out


class MiYuvTarget(ctypes.Structure):
    _fields_ = [("mtrx", ctypes.c_int32), ("range", ctypes.c_int32)]


def YuvTarget(mtrx=1, range=0):
    """A MiYuvTarget: the Y'CbCr a tone-mapped YUV output is written in, the matrix (1 BT.709, 4, 5,
    6 BT.601, 7, 9 BT.2020 NCL) and the range (0 limited, 1 full). The default is what an SDR
    encoder expects: BT.709, limited."""
    return MiYuvTarget(int(mtrx), int(range))


def output_colour(tonemap, target, chr=0):
    """The MiColorInfo an encoder should tag the output of display_yuv / display_scaled(tonemap=)
    with: the tone map's primaries and transfer, the target's matrix and range, the source's chroma
    siting `chr` (the outputs keep it)."""
    target = YuvTarget() if target is None else target
    return MiColorInfo(tonemap.dst_pri, tonemap.dst_trc, target.mtrx, target.range, int(chr))


def display_yuv(ctx, frame, image, color, tonemap, target=None, fg=None, stream=None):
    """Enqueue mi_display_yuv_tm: `frame` (a device Frame or a MiPicture) through the colour-volume
    stage `tonemap` (a MiToneMap; color.pri, color.trc and color.mtrx describe the source) and back
    to Y'CbCr in `target` (a MiYuvTarget; None: YuvTarget()), semi-planar at the frame's own
    subsampling and tonemap.dst_bpc bits, into `image`: a DisplayImage(..., "nv12",
    out_bpc=tonemap.dst_bpc) or a MiDisplayImage. fg: film grain, applied to the source. Raises
    MiError on a negative return."""
    src, cp, fp = _source_args(frame, color, fg)
    im = image if isinstance(image, MiDisplayImage) else image.image()
    target = YuvTarget() if target is None else target
    check(lib().mi_display_yuv_tm(ctx.h, ctypes.byref(src), ctypes.byref(im), cp,
                                  ctypes.byref(tonemap) if tonemap is not None else None, ctypes.byref(target), fp,
                                  _stream_ptr(stream)), "mi_display_yuv_tm")


def display_scaled(ctx, frame, images, color=None, fg=None, stream=None, resample=None, tonemap=None, target=None):
    """Enqueue mi_display_scaled: `frame` (a device Frame or a MiPicture) cropped, resized and
    converted to each rung's depth into `images`, 1 to 8 ScaledImage or MiScaledImage (or one of
    them on its own), semi-planar at the frame's own subsampling, in one call: film grain (`fg`: a
    MiFilmGrainData or a make_fg_params dict) is applied once and every rung reads the grained
    picture. color: a MiColorInfo or None; only its chr is read (the 4:2:0 chroma siting, of the
    source and of the output). resample: a MiResample (Resample()): the call is
    mi_display_scaled_rs and every plane of every rung is resized with that filter; None calls
    mi_display_scaled (the triangle). tonemap: a MiToneMap (ToneMap()): the call is
    mi_display_scaled_tm, the rungs are resized from the tone-mapped picture in the Y'CbCr of
    `target` (a MiYuvTarget; None: YuvTarget()), color.pri, color.trc and color.mtrx describe the
    source, and a rung's depth converts from tonemap.dst_bpc (output_colour gives the tags of the
    result). Without tonemap, `target` must be None. Raises MiError on a negative return."""
    src, cp, fp = _source_args(frame, color, fg)
    if isinstance(images, (ScaledImage, MiScaledImage)):
        images = [images]
    ims = (MiScaledImage * max(len(images), 1))()
    for i, image in enumerate(images):
        ims[i] = image if isinstance(image, MiScaledImage) else image.image()
    if tonemap is not None:
        target = YuvTarget() if target is None else target
        check(lib().mi_display_scaled_tm(ctx.h, ctypes.byref(src), ims, len(images), cp, ctypes.byref(tonemap),
                                         ctypes.byref(target), ctypes.byref(resample) if resample is not None else None,
                                         fp, _stream_ptr(stream)), "mi_display_scaled_tm")
        return
    if target is not None:
        raise ValueError("target needs a tonemap: a matrix or range conversion alone is not an output")
    if resample is not None:
        check(lib().mi_display_scaled_rs(ctx.h, ctypes.byref(src), ims, len(images), cp, ctypes.byref(resample), fp,
                                         _stream_ptr(stream)), "mi_display_scaled_rs")
        return
    check(lib().mi_display_scaled(ctx.h, ctypes.byref(src), ims, len(images), cp, fp, _stream_ptr(stream)),
          "mi_display_scaled")


class MiLightLevel(ctypes.Structure):
    _fields_ = [("max_code", ctypes.c_int32), ("pct_code", ctypes.c_int32),
                ("max_nits", ctypes.c_double), ("pct_nits", ctypes.c_double), ("avg_nits", ctypes.c_double)]


_light = None


def _light_lib():
    """lib() with the signatures of the light-level entries set (a library without them raises
    AttributeError here: nothing stands in for a missing entry)."""
    global _light
    if _light is None:
        L, vp = lib(), ctypes.c_void_p
        for name, args in (("mi_picture_light_level", [vp, ctypes.POINTER(MiPicture), vp, vp, vp]),
                           ("mi_picture_light_level_variant", [vp, ctypes.POINTER(MiPicture), vp, vp, ctypes.c_int, vp]),
                           ("mi_light_level_stats", [vp, ctypes.c_int, ctypes.c_double, vp])):
            f = getattr(L, name)
            f.restype, f.argtypes = ctypes.c_int, args
        _light = L
    return _light


def light_level(ctx, frame, color, stream=None, variant=None):
    """Enqueue mi_picture_light_level: the histogram of max(R', G', B') over the planar R'G'B'
    picture display_picture(..., "rgb") would write for `frame` (a device Frame or a MiPicture)
    and `color`, without film grain. Returns a fresh torch.int32 device tensor of 1 << bpc bins
    (the bits are those of the uint32 counts), filled by work enqueued on `stream`. variant: the
    counting variant of mi_picture_light_level_variant (a diagnostic; None: the entry itself).
    Raises MiError on a negative return."""
    src = frame if isinstance(frame, MiPicture) else frame.picture()
    n = 1 << src.bpc if src.bpc in (8, 10, 12) else 1
    hist = torch.empty(n, dtype=torch.int32, device="cuda")
    cp = ctypes.byref(color) if color is not None else None
    if variant is None:
        check(_light_lib().mi_picture_light_level(ctx.h, ctypes.byref(src), cp, ctypes.c_void_p(hist.data_ptr()),
                                           _stream_ptr(stream)), "mi_picture_light_level")
    else:
        check(_light_lib().mi_picture_light_level_variant(ctx.h, ctypes.byref(src), cp, ctypes.c_void_p(hist.data_ptr()),
                                                   int(variant), _stream_ptr(stream)), "mi_picture_light_level_variant")
    return hist


def light_stats(hist, bpc, percentile=99.99):
    """mi_light_level_stats (host only): the MiLightLevel of a histogram of `bpc` bits read as
    full-range PQ codes: max_code / max_nits, pct_code / pct_nits (the lowest code whose
    cumulative count reaches ceil(percentile / 100 * N)) and avg_nits. hist: light_level's tensor
    (copied to the host, which synchronises) or any array of 1 << bpc counts. Raises MiError on a
    negative return (an empty histogram, a percentile outside (0, 100])."""
    if isinstance(hist, torch.Tensor):
        hist = hist.cpu().numpy()
    h = np.ascontiguousarray(np.asarray(hist).view(np.uint32) if np.asarray(hist).dtype == np.int32
                             else np.asarray(hist, dtype=np.uint32))
    if bpc in (8, 10, 12) and h.size != 1 << bpc:
        raise ValueError(f"hist of {h.size} bins for {bpc} bits")
    out = MiLightLevel()
    check(_light_lib().mi_light_level_stats(h.ctypes.data_as(ctypes.c_void_p), int(bpc), ctypes.c_double(percentile),
                                     ctypes.byref(out)), "mi_light_level_stats")
    return out


__all__ = ["DisplayImage", "MiDisplayImage", "MiColorInfo", "display_picture", "FORMATS",
           "MiScaledImage", "ScaledImage", "display_scaled", "even_crop",
           "OUT_SEMIPLANAR", "OUT_RGB_PLANAR", "OUT_RGBA_PACKED",
           "MiTensorImage", "tensor_image", "display_tensor", "T_U8", "T_F16", "T_BF16", "T_F32",
           "MiToneMap", "ToneMap", "tonemap_tables", "enable_hlg", "tonemap_tables_hlg", "MiYuvTarget", "YuvTarget", "display_yuv", "output_colour",
           "MiLightLevel", "light_level", "light_stats",
           "MiResample", "Resample", "RESAMPLE_PRESETS", "RS_TRIANGLE", "RS_CUBIC", "resample_plan", "resample_taps"]
