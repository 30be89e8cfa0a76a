"""CPU, no device: mi_display_picture_tm, mi_display_tensor_tm and mi_tonemap_tables check their
arguments on the host before any device work, the NULL context last (as tests/test_display_args.py
and tests/test_tensor_args.py): a call whose other arguments pass is -EINVAL for the context alone,
so every refusal below is isolated by changing one thing in a call that is otherwise accepted, and
an -ENOTSUP can only come from the rule under test."""
import ctypes
import errno
import math

import pytest

from rav1d_amd import lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (OUT_RGB_PLANAR, OUT_RGBA_PACKED, OUT_SEMIPLANAR, T_F16, T_U8, MiTensorImage, ToneMap)
from tests.test_display_args import P, image, picture

E, NS = -errno.EINVAL, -errno.ENOTSUP
HDR10 = MiColorInfo(9, 16, 9, 0, 0)
SDR = MiColorInfo(1, 1, 1, 0, 0)


def call_pic(pic, im, color, tm):
    return lib().mi_display_picture_tm(None, ctypes.byref(pic) if pic is not None else None,
                                       ctypes.byref(im) if im is not None else None,
                                       ctypes.byref(color) if color is not None else None,
                                       ctypes.byref(tm) if tm is not None else None, None, None)


def tensor(dtype=T_F16, w=8, h=8):
    im = MiTensorImage()
    es = 1 if dtype == T_U8 else 2
    im.data, im.w, im.h, im.dtype = P + 32768, w, h, dtype
    im.stride[0], im.stride[1], im.stride[2] = w * h * es, w * es, es
    for c in range(3):
        im.scale[c], im.bias[c] = 1.0, 0.0
    return im


def call_tensor(pic, im, color, tm):
    return lib().mi_display_tensor_tm(None, ctypes.byref(pic), ctypes.byref(im),
                                      ctypes.byref(color) if color is not None else None,
                                      ctypes.byref(tm) if tm is not None else None, None, None)


BUFS = ((ctypes.c_float * 4096)(), (ctypes.c_float * 9)(), (ctypes.c_uint16 * 65536)())


def call_tables(tm, color, src_bpc=10, bufs=BUFS):
    return lib().mi_tonemap_tables(ctypes.byref(tm) if tm is not None else None,
                                   ctypes.byref(color) if color is not None else None, src_bpc, *bufs)


def every_entry(color, tm, src_bpc=10):
    """The three entries' answers for one (color, tm), everything else accepted."""
    pic = picture(bpc=src_bpc)
    dst = tm.dst_bpc if tm is not None and tm.dst_bpc in (8, 10, 12) else 8
    return (call_pic(pic, image(OUT_RGB_PLANAR, bpc=dst), color, tm), call_tensor(pic, tensor(), color, tm),
            call_tables(tm, color, src_bpc))


def test_accepted_without_a_context():
    """Everything but the context passes: -EINVAL for the NULL context from the two device entries,
    0 from the host-only one."""
    for color in (HDR10, SDR, MiColorInfo(5, 6, 6, 1, 2), MiColorInfo(6, 14, 6, 0, 0), MiColorInfo(7, 15, 7, 0, 0),
                  MiColorInfo(12, 13, 1, 1, 0)):
        for tm in (ToneMap(), ToneMap(9, 1, 10), ToneMap(12, 13, 12, 4000.0, 1000.0)):
            for src_bpc in (8, 10, 12):
                assert every_entry(color, tm, src_bpc) == (E, E, 0)
    # out->bpc follows dst_bpc, not the source: every pair
    for src_bpc in (8, 10, 12):
        for dst_bpc in (8, 10, 12):
            for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED):
                assert call_pic(picture(bpc=src_bpc), image(fmt, bpc=dst_bpc), HDR10, ToneMap(dst_bpc=dst_bpc)) == E
    assert call_tensor(picture(bpc=10), tensor(T_U8), HDR10, ToneMap(dst_bpc=12)) == E


def test_null_tonemap():
    assert every_entry(HDR10, None) == (E, E, E)


def test_null_color():
    assert every_entry(None, ToneMap()) == (E, E, E)


@pytest.mark.parametrize("pri", [2, 0, 3, 13, 21, 23, -1])
def test_unspecified_or_reserved_primaries(pri):
    assert every_entry(MiColorInfo(pri, 16, 9, 0, 0), ToneMap()) == (E, E, E)


@pytest.mark.parametrize("pri", [4, 8, 10, 11, 22])
def test_other_defined_primaries(pri):
    assert every_entry(MiColorInfo(pri, 16, 9, 0, 0), ToneMap()) == (NS, NS, NS)


@pytest.mark.parametrize("trc", [2, 0, 3, 19, -1])
def test_unspecified_or_reserved_transfer(trc):
    assert every_entry(MiColorInfo(9, trc, 9, 0, 0), ToneMap()) == (E, E, E)


@pytest.mark.parametrize("trc", [18, 8, 4, 5, 7, 9, 10, 11, 12, 17])
def test_other_defined_transfers(trc):
    """HLG (18), linear (8), the gammas, 240M, the logs, IEC 61966-2-4, BT.1361, ST 428."""
    assert every_entry(MiColorInfo(9, trc, 9, 0, 0), ToneMap()) == (NS, NS, NS)


@pytest.mark.parametrize("field,value", [("dst_pri", 2), ("dst_pri", 5), ("dst_pri", 6), ("dst_pri", 0), ("dst_trc", 16),
                                         ("dst_trc", 2), ("dst_trc", 14), ("dst_bpc", 9), ("dst_bpc", 16), ("dst_bpc", 0)])
def test_destination_outside_the_lists(field, value):
    tm = ToneMap()
    setattr(tm, field, value)
    assert every_entry(HDR10, tm) == (E, E, E)
    assert every_entry(SDR, tm) == (E, E, E)


BAD_PEAKS = [0.0, 0.5, -100.0, 10000.5, 1e9, math.inf, -math.inf, math.nan]


@pytest.mark.parametrize("peak", BAD_PEAKS)
def test_peaks_of_pq_sources(peak):
    assert every_entry(HDR10, ToneMap(src_peak=peak)) == (E, E, E)
    assert every_entry(HDR10, ToneMap(dst_peak=peak)) == (E, E, E)


def test_peak_limits_are_inclusive():
    assert every_entry(HDR10, ToneMap(src_peak=1.0, dst_peak=1.0)) == (E, E, 0)
    assert every_entry(HDR10, ToneMap(src_peak=10000.0, dst_peak=10000.0)) == (E, E, 0)


@pytest.mark.parametrize("peak", BAD_PEAKS)
def test_peaks_are_not_read_for_sdr_sources(peak):
    for trc in (1, 6, 13, 14, 15):
        color = MiColorInfo(1, trc, 1, 0, 0)
        assert every_entry(color, ToneMap(src_peak=peak, dst_peak=peak)) == (E, E, 0)


def test_sdr_tables_do_not_depend_on_the_peaks():
    a = [(ctypes.c_float * 1024)(), (ctypes.c_float * 9)(), (ctypes.c_uint16 * 65536)()]
    b = [(ctypes.c_float * 1024)(), (ctypes.c_float * 9)(), (ctypes.c_uint16 * 65536)()]
    assert call_tables(ToneMap(), SDR, 10, a) == 0
    assert call_tables(ToneMap(src_peak=math.nan, dst_peak=-1.0), SDR, 10, b) == 0
    assert all(bytes(x) == bytes(y) for x, y in zip(a, b))


def test_semiplanar_is_not_supported():
    assert call_pic(picture(), image(OUT_SEMIPLANAR), HDR10, ToneMap()) == NS
    assert call_pic(picture(bpc=10), image(OUT_SEMIPLANAR, bpc=10), None, ToneMap(dst_bpc=10)) == NS


def test_output_depth_must_be_dst_bpc():
    for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED):
        assert call_pic(picture(bpc=10), image(fmt, bpc=10), HDR10, ToneMap(dst_bpc=8)) == E
        assert call_pic(picture(bpc=10), image(fmt, bpc=8), HDR10, ToneMap(dst_bpc=10)) == E
        assert call_pic(picture(bpc=8), image(fmt, bpc=12), SDR, ToneMap(dst_bpc=8)) == E
        assert call_pic(picture(bpc=8), image(fmt, bpc=9), SDR, ToneMap(dst_bpc=8)) == E


def test_tables_arguments():
    tm = ToneMap()
    for bpc in (9, 0, 16, -8):
        assert call_tables(tm, HDR10, bpc) == E
    for i in range(3):
        bufs = list(BUFS)
        bufs[i] = None
        assert call_tables(tm, HDR10, 10, bufs) == E


def test_rules_of_the_plain_entries_still_apply():
    """The colour-matrix rules of display_color, the size and the destination checks."""
    tm = ToneMap()
    for color, want in ((MiColorInfo(9, 16, 2, 0, 0), E), (MiColorInfo(9, 16, 9, 2, 0), E), (MiColorInfo(9, 16, 3, 0, 0), E),
                        (MiColorInfo(9, 16, 0, 1, 0), E),      # identity needs 4:4:4
                        (MiColorInfo(9, 16, 8, 0, 0), NS), (MiColorInfo(9, 16, 14, 0, 0), NS)):
        assert call_pic(picture(), image(OUT_RGB_PLANAR), color, tm) == want
        assert call_tensor(picture(), tensor(), color, tm) == want
    assert call_pic(None, image(OUT_RGB_PLANAR), HDR10, tm) == E
    assert call_pic(picture(), None, HDR10, tm) == E
    assert call_pic(picture(), image(OUT_RGB_PLANAR, w=31), HDR10, tm) == E
    assert call_pic(picture(), image(3), HDR10, tm) == E
    assert call_pic(picture(), image(OUT_RGB_PLANAR, planes=2), HDR10, tm) == E
    assert call_pic(picture(bpc=9), image(OUT_RGB_PLANAR), HDR10, tm) == E
    # the row size and the alignment follow the destination's sample type, not the source's
    assert call_pic(picture(bpc=8), image(OUT_RGBA_PACKED, bpc=10, stride=4 * 32 * 2 - 2), SDR, ToneMap(dst_bpc=10)) == E
    assert call_pic(picture(bpc=8), image(OUT_RGBA_PACKED, bpc=10, stride=4 * 32 * 2 + 1), SDR, ToneMap(dst_bpc=10)) == E
    assert call_pic(picture(bpc=10), image(OUT_RGBA_PACKED, bpc=8, stride=4 * 32 - 1), HDR10, ToneMap(dst_bpc=8)) == E
    bad = tensor()
    bad.crop_w, bad.crop_h = 64, 8
    assert call_tensor(picture(), bad, HDR10, tm) == E
