"""CPU, no device: mi_display_tensor checks its arguments on the host before any device work, with
the NULL context checked last (as mi_display_picture, tests/test_display_args.py): a call whose
other arguments pass is -EINVAL for that alone."""
import ctypes
import errno
import math

import pytest

from rav1d_amd import MiPicture, lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import T_BF16, T_F16, T_F32, T_U8, MiTensorImage

BUF = (ctypes.c_uint8 * (1 << 16))()
P = (ctypes.addressof(BUF) + 63) & ~63
E = -errno.EINVAL
ES = {T_U8: 1, T_F16: 2, T_BF16: 2, T_F32: 4}
# An unsupported matrix: the colour rules are checked after every other argument, so -EINVAL with
# it comes from the argument a test names, and -ENOTSUP shows that every other argument passed.
UNSUP = MiColorInfo(1, 1, 8, 0, 0)


def picture(w=32, h=16, bpc=8, layout=1, stride=None):
    pic = MiPicture()
    for p in range(3):
        pic.data[p] = P + 4096 * p
    pxb = 1 if bpc == 8 else 2
    pic.stride[0] = pic.stride[1] = stride if stride is not None else max(128, w) * pxb
    pic.w, pic.h, pic.bpc, pic.layout = w, h, bpc, layout
    return pic


def image(w=8, h=4, dtype=T_F16, crop=None, strides=None, offset=0, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0),
          data=True):
    im = MiTensorImage()
    es = ES.get(dtype, 1)
    im.data = P + 16384 + offset if data else None
    for i, s in enumerate(strides if strides is not None else (w * h * es, w * es, es)):
        im.stride[i] = s
    im.w, im.h, im.dtype = w, h, dtype
    if crop is not None:
        im.crop_x, im.crop_y, im.crop_w, im.crop_h = crop
    for c in range(3):
        im.scale[c], im.bias[c] = scale[c], bias[c]
    return im


def call(pic, im, color=UNSUP):
    return lib().mi_display_tensor(None, ctypes.byref(pic) if pic is not None else None,
                                   ctypes.byref(im) if im is not None else None,
                                   ctypes.byref(color) if color is not None else None, None, None)


def test_null_arguments():
    assert call(None, image()) == E
    assert call(picture(), None) == E
    assert call(picture(), image(data=False)) == E
    assert call(picture(), image(), None) == E
    src = picture()
    src.data[0] = None
    assert call(src, image()) == E
    src = picture()
    src.data[2] = None
    assert call(src, image()) == E


def test_source():
    assert call(picture(bpc=9), image()) == E
    assert call(picture(layout=4), image()) == E
    assert call(picture(w=0), image()) == E
    assert call(picture(stride=31), image()) == E


def test_crop():
    for crop in ((0, 0, 33, 16), (0, 0, 32, 17), (1, 0, 32, 16), (0, 1, 32, 16), (-1, 0, 8, 8), (0, -1, 8, 8),
                 (32, 0, 1, 1), (0, 16, 1, 1), (0, 0, 0, 5), (0, 0, 5, 0), (3, 3, -2, 4), (3, 3, 4, -2)):
        assert call(picture(), image(crop=crop)) == E, crop


def test_output_size_and_downscale_limit():
    assert call(picture(), image(w=0)) == E
    assert call(picture(), image(h=0)) == E
    assert call(picture(), image(w=-1)) == E
    assert call(picture(), image(w=65537, strides=(2, 2, 2))) == E
    assert call(picture(), image(h=65537, strides=(2, 2, 2))) == E
    # above 64:1 on either axis: 521 -> 8, 16 -> 0.24
    assert call(picture(w=521), image(w=8)) == E
    assert call(picture(w=600, h=521, layout=3, stride=600), image(w=16, h=8)) == E
    assert call(picture(w=521), image(w=8, crop=(0, 0, 513, 16))) == E


def test_dtype():
    for dtype in (-1, 4, 255):
        assert call(picture(), image(dtype=dtype)) == E


@pytest.mark.parametrize("dtype", [T_F16, T_BF16, T_F32])
def test_strides_and_alignment(dtype):
    es = ES[dtype]
    good = (8 * 4 * es, 8 * es, es)
    for i in range(3):
        for bad in (0, -good[i], good[i] + 1, good[i] + es - 1):
            s = list(good)
            s[i] = bad
            assert call(picture(), image(dtype=dtype, strides=tuple(s))) == E, (i, bad)
    for offset in range(1, es):
        assert call(picture(), image(dtype=dtype, offset=offset)) == E
    assert call(picture(), image(dtype=T_U8, strides=(0, 8, 1))) == E
    assert call(picture(), image(dtype=T_U8, strides=(32, -8, 1))) == E


def test_non_finite_scale_and_bias():
    for bad in (math.inf, -math.inf, math.nan):
        for c in range(3):
            v = [1.0, 1.0, 1.0]
            v[c] = bad
            assert call(picture(), image(scale=tuple(v))) == E
            assert call(picture(), image(bias=tuple(v))) == E


def test_colour_errors():
    assert call(picture(), image(), None) == E
    assert call(picture(), image(), MiColorInfo(2, 2, 2, 0, 0)) == E
    assert call(picture(), image(), MiColorInfo(1, 1, 1, 2, 0)) == E       # range
    assert call(picture(), image(), MiColorInfo(1, 1, 1, -1, 0)) == E
    assert call(picture(), image(), MiColorInfo(1, 1, 3, 0, 0)) == E       # reserved matrix
    assert call(picture(), image(), MiColorInfo(1, 1, 15, 0, 0)) == E
    for layout in (0, 1, 2):                                             # identity needs 4:4:4
        assert call(picture(layout=layout), image(), MiColorInfo(1, 13, 0, 1, 0)) == E


def test_enotsup():
    for mtrx in (8, 10, 11, 12, 13, 14):
        assert call(picture(), image(), MiColorInfo(1, 1, mtrx, 0, 0)) == -errno.ENOTSUP


@pytest.mark.parametrize("mtrx", [1, 4, 5, 6, 7, 9])
def test_valid_arguments_without_a_context(mtrx):
    """Everything but the context passes: -EINVAL for the NULL context, nothing was launched.
    (The calls of the tests above differ from one of these in the one thing they name.)"""
    color = MiColorInfo(1, 1, mtrx, 1, 2)

    def passes(pic, im, color=color):
        assert call(pic, im, UNSUP) == -errno.ENOTSUP
        return call(pic, im, color)

    for dtype in (T_U8, T_F16, T_BF16, T_F32):
        es = ES[dtype]
        assert passes(picture(), image(dtype=dtype), color) == E
        assert passes(picture(), image(dtype=dtype, strides=(es, 8 * 3 * es, 3 * es)), color) == E       # HWC
        assert passes(picture(), image(dtype=dtype, strides=(8 * es, 8 * 3 * es + 4 * es, 2 * es)), color) == E
    assert passes(picture(layout=3), image(), MiColorInfo(1, 13, 0, 1, 0)) == E
    assert passes(picture(), image(crop=(3, 5, 21, 11)), color) == E
    assert passes(picture(), image(crop=(31, 15, 1, 1)), color) == E
    assert passes(picture(), image(w=65536, h=1, dtype=T_U8, strides=(1, 1, 1)), color) == E
    # the 64:1 extreme passes: 512 -> 8
    assert passes(picture(w=512), image(w=8), color) == E
    assert passes(picture(w=521), image(w=8, crop=(9, 0, 512, 16)), color) == E
    # a non-finite scale is not read for uint8
    assert passes(picture(), image(dtype=T_U8, strides=(32, 8, 1), scale=(math.nan, 1.0, 1.0)), color) == E
