"""CPU, no device: mi_display_picture checks its arguments on the host before any device work,
as the per-call entries do (tests/test_abi.py). No context can exist without a GPU, so the
context is NULL: a call whose other arguments pass is -EINVAL for that alone."""
import ctypes
import errno

import pytest

from rav1d_amd import MiPicture, lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import OUT_RGB_PLANAR, OUT_RGBA_PACKED, OUT_SEMIPLANAR, MiDisplayImage

BUF = (ctypes.c_uint8 * (1 << 16))()
P = ctypes.addressof(BUF)


def picture(w=32, h=16, bpc=8, layout=1):
    pic = MiPicture()
    for p in range(3):
        pic.data[p] = P + 4096 * p
    pic.stride[0], pic.stride[1] = 128 * (1 if bpc == 8 else 2), 128 * (1 if bpc == 8 else 2)
    pic.w, pic.h, pic.bpc, pic.layout = w, h, bpc, layout
    return pic


def image(fmt, w=32, h=16, bpc=8, planes=3, stride=None):
    im = MiDisplayImage()
    for p in range(planes):
        im.data[p] = P + 16384 + 8192 * p
        im.stride[p] = stride if stride is not None else 4 * w * (1 if bpc == 8 else 2)
    im.w, im.h, im.format, im.bpc = w, h, fmt, bpc
    return im


def call(pic, im, color=None):
    return lib().mi_display_picture(None, ctypes.byref(pic) if pic is not None else None,
                                    ctypes.byref(im) if im is not None else None,
                                    ctypes.byref(color) if color is not None else None, None, None)


BT709 = MiColorInfo(1, 1, 1, 0, 0)


def test_einval():
    E = -errno.EINVAL
    assert call(None, image(OUT_SEMIPLANAR)) == E
    assert call(picture(), None) == E
    # size or bpc mismatch
    assert call(picture(), image(OUT_SEMIPLANAR, w=31)) == E
    assert call(picture(), image(OUT_SEMIPLANAR, h=17)) == E
    assert call(picture(), image(OUT_RGB_PLANAR, bpc=10), BT709) == E
    # identity needs 4:4:4
    for layout in (0, 1, 2):
        assert call(picture(layout=layout), image(OUT_RGB_PLANAR), MiColorInfo(1, 13, 0, 1, 0)) == E
    # an RGB format without a colour description, or with an unspecified matrix: the caller chooses
    for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED):
        assert call(picture(), image(fmt), None) == E
        assert call(picture(), image(fmt), MiColorInfo(2, 2, 2, 0, 0)) == E
    assert call(picture(), image(OUT_RGB_PLANAR), MiColorInfo(1, 1, 1, 2, 0)) == E      # range
    assert call(picture(), image(OUT_RGB_PLANAR), MiColorInfo(1, 1, 3, 0, 0)) == E      # reserved matrix
    assert call(picture(), image(OUT_RGB_PLANAR), MiColorInfo(1, 1, 15, 0, 0)) == E
    # format
    assert call(picture(), image(3), BT709) == E
    assert call(picture(), image(-1), BT709) == E
    # null planes: Y; UV of a picture with chroma; G / B
    assert call(picture(), image(OUT_SEMIPLANAR, planes=0)) == E
    assert call(picture(), image(OUT_SEMIPLANAR, planes=1)) == E
    assert call(picture(), image(OUT_RGB_PLANAR, planes=2), BT709) == E
    assert call(picture(), image(OUT_RGBA_PACKED, planes=0), BT709) == E
    src = picture()
    src.data[2] = None
    assert call(src, image(OUT_SEMIPLANAR)) == E
    # a stride shorter than a row; 16-bit samples off their alignment
    assert call(picture(), image(OUT_SEMIPLANAR, stride=31)) == E
    assert call(picture(), image(OUT_RGBA_PACKED, stride=127), BT709) == E
    assert call(picture(bpc=10), image(OUT_SEMIPLANAR, bpc=10, stride=129)) == E
    # source: bit depth, layout, size
    assert call(picture(bpc=9), image(OUT_SEMIPLANAR, bpc=9)) == E
    assert call(picture(layout=4), image(OUT_SEMIPLANAR)) == E
    assert call(picture(w=0), image(OUT_SEMIPLANAR, w=0)) == E


def test_enotsup():
    for mtrx in (8, 10, 11, 12, 13, 14):
        for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED):
            assert call(picture(), image(fmt), MiColorInfo(1, 1, mtrx, 0, 0)) == -errno.ENOTSUP


@pytest.mark.parametrize("mtrx", [1, 4, 5, 6, 7, 9])
def test_valid_arguments_without_a_context(mtrx):
    """Everything but the context passes: -EINVAL for the NULL context, nothing was launched."""
    for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED):
        assert call(picture(), image(fmt), MiColorInfo(1, 1, mtrx, 1, 2)) == -errno.EINVAL
    assert call(picture(layout=3), image(OUT_RGB_PLANAR), MiColorInfo(1, 13, 0, 1, 0)) == -errno.EINVAL
    assert call(picture(), image(OUT_SEMIPLANAR)) == -errno.EINVAL
    assert call(picture(layout=0), image(OUT_SEMIPLANAR, planes=1)) == -errno.EINVAL
