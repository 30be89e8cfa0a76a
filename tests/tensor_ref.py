"""Reference model of the tensor output (include/mi_av1out.h, mi_display_tensor), written from the
arithmetic the header states: the integer taps of the triangle filter, the separable resize
(horizontal pass first), the finish of the four dtypes, and the whole call on top of
tests/display_ref.py's integer R'G'B' picture. The taps, the pass over one axis and the float64
triangle filter that bounds it are tests/resize_ref.py's, in the centred siting."""
import numpy as np

from tests import display_ref as R
from tests.resize_ref import S, resize_axis, triangle_float, weights  # noqa: F401 (the tests call them as T.*)

U8, F16, BF16, F32 = 0, 1, 2, 3


def resize(x, out_w, out_h):
    """(..., h, w) -> (..., out_h, out_w): the horizontal pass, then the vertical pass over its integers."""
    return resize_axis(resize_axis(x, out_w, -1), out_h, -2)


def bfloat16_bits(f):
    """float32 array -> the bfloat16 bit patterns (uint16), round to nearest-even."""
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def finish(v, bpc, dtype, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """(3, h, w) integers -> the stored elements: uint8, float16, bfloat16 as its uint16 bit
    patterns, or float32. scale and bias are rounded to float32 here."""
    v = np.asarray(v, dtype=np.int64)
    if dtype == U8:
        return (v if bpc == 8 else np.minimum(255, (v + (1 << (bpc - 9))) >> (bpc - 8))).astype(np.uint8)
    s = np.asarray(scale, dtype=np.float32).reshape(3, 1, 1)
    b = np.asarray(bias, dtype=np.float32).reshape(3, 1, 1)
    f = v.astype(np.float32) * s       # float32 product, rounded
    f = (f + b).astype(np.float32)     # float32 sum, rounded
    assert f.dtype == np.float32
    if dtype == F32:
        return f
    if dtype == F16:
        return f.astype(np.float16)
    return bfloat16_bits(f)


def scale_bias(bpc, mean=None, std=None):
    """display_tensor's scale and bias: Python floats, rounded once to float32."""
    mean = (0.0, 0.0, 0.0) if mean is None else mean
    std = (1.0, 1.0, 1.0) if std is None else std
    m = float((1 << bpc) - 1)
    return ([np.float32(1.0 / (m * float(s))) for s in std], [np.float32(-float(a) / float(s)) for a, s in zip(mean, std)])


def tensor(planes, bpc, layout, color, crop, size, dtype, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """The whole call. color: (mtrx, full range, chr); crop: (x, y, w, h) or None; size: (w, h).
    Returns the (3, h, w) stored elements (finish)."""
    mtrx, full, chr = color
    rgb = R.to_rgb(planes, bpc, layout, mtrx, full, chr)
    if crop is not None:
        x, y, w, h = crop
        rgb = rgb[:, y:y + h, x:x + w]
    return finish(resize(rgb, size[0], size[1]), bpc, dtype, scale, bias)

