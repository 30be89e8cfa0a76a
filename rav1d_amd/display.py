"""Device display output (include/mi_av1out.h, mi_display_picture): a shown picture as a tight
torch tensor on the device, semi-planar YUV (NV12 / P010 and their 4:2:2 / 4:4:4 kin) or R'G'B'
(planar, or packed with alpha), with film grain applied. torch allocates; the conversion is the
gfx950 kernel of csrc/display.hip."""
import ctypes

import torch

from . import MiFilmGrainData, MiPicture, check, lib
from .av1dec import MiColorInfo

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
    full range at the source bit depth, LSB-aligned."""

    def __init__(self, w, h, bpc, layout, format, device="cuda"):
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


def display_picture(ctx, frame, image, color=None, fg=None, stream=None):
    """Enqueue mi_display_picture: `frame` (a device Frame or a MiPicture) into `image` (a
    DisplayImage or a MiDisplayImage), with film grain when `fg` (a MiFilmGrainData or a
    make_fg_params dict). color: a MiColorInfo, needed by the RGB formats (its mtrx picks the
    matrix, range the scaling, chr the 4:2:0 chroma siting). Raises MiError on a negative return."""
    from .frame import _stream_ptr, film_grain_data
    src = frame if isinstance(frame, MiPicture) else frame.picture()
    im = image if isinstance(image, MiDisplayImage) else image.image()
    if fg is not None and not isinstance(fg, MiFilmGrainData):
        fg = film_grain_data(fg)
    check(lib().mi_display_picture(ctx.h, ctypes.byref(src), ctypes.byref(im),
                                   ctypes.byref(color) if color is not None else None,
                                   ctypes.byref(fg) if fg is not None else None, _stream_ptr(stream)),
          "mi_display_picture")


__all__ = ["DisplayImage", "MiDisplayImage", "MiColorInfo", "display_picture", "FORMATS",
           "OUT_SEMIPLANAR", "OUT_RGB_PLANAR", "OUT_RGBA_PACKED"]
