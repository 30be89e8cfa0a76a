"""CPU, no device: the host side of HLG sources (include/mi_av1out.h, "HLG sources"):
mi_ctx_enable_hlg and mi_tonemap_tables_hlg check their arguments, the device entries and
mi_tonemap_tables keep answering -ENOTSUP for trc 18 without a context that has opted in, and the
tables of mi_tonemap_tables_hlg are tests/hlg_ref.py's bit for bit (the model evaluates the same
formulas in double precision, entry by entry, and rounds once as the library does)."""
import ctypes
import errno
import math

import numpy as np
import pytest

from rav1d_amd import MiError, lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (OUT_RGB_PLANAR, OUT_RGBA_PACKED, Resample, ToneMap, YuvTarget, enable_hlg,
                               tonemap_tables_hlg)
from tests import hlg_ref as H
from tests.test_display_args import image, picture
from tests.test_tonemap_args import BAD_PEAKS, call_pic, call_tables, call_tensor, tensor
from tests.test_yuv_tm_args import both

E, NS = -errno.EINVAL, -errno.ENOTSUP
HLG = MiColorInfo(9, 18, 9, 0, 0)
PEAKS = [50.0, 100.0, 203.0, 1000.0, 4000.0, 10000.0]


def bufs(src_bpc=10):
    return [(ctypes.c_float * (1 << src_bpc))(), (ctypes.c_float * 9)(), (ctypes.c_uint16 * 65536)(),
            (ctypes.c_float * 3)(), (ctypes.c_float * 1538)()]


BUFS = bufs(12)


def call_hlg(tm, color, src_bpc=10, out=BUFS):
    return lib().mi_tonemap_tables_hlg(ctypes.byref(tm) if tm is not None else None,
                                       ctypes.byref(color) if color is not None else None, src_bpc, *out)


def call_tensor_rs(pic, im, color, tm, rs):
    return lib().mi_display_tensor_rs(None, ctypes.byref(pic), ctypes.byref(im), ctypes.byref(color), ctypes.byref(tm),
                                      ctypes.byref(rs), None, None)


def test_enable_needs_a_context():
    assert lib().mi_ctx_enable_hlg(None, 1) == E
    assert lib().mi_ctx_enable_hlg(None, 0) == E
    with pytest.raises(MiError):
        enable_hlg(None)


def test_every_device_entry_refuses_hlg_without_a_context():
    """Calls that are -EINVAL for the NULL context alone with a PQ source are -ENOTSUP with trc 18:
    the answer of a library from before HLG."""
    pq = MiColorInfo(9, 16, 9, 0, 0)
    for src_bpc in (8, 10, 12):
        for tm in (ToneMap(), ToneMap(9, 1, 10, math.nan, 1000.0), ToneMap(12, 13, 12, 4000.0, 203.0)):
            pic = picture(bpc=src_bpc)
            for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED):
                assert call_pic(pic, image(fmt, bpc=tm.dst_bpc), HLG, tm) == NS
            assert call_tensor(pic, tensor(), HLG, tm) == NS
            assert call_tensor_rs(pic, tensor(), HLG, tm, Resample("catmull_rom")) == NS
            assert both(HLG, tm, YuvTarget(), src_bpc) == (NS, NS)
            assert call_tables(tm, HLG, src_bpc) == NS
    # (the same calls with a PQ source: everything but the context passes)
    tm = ToneMap()
    assert call_pic(picture(), image(OUT_RGB_PLANAR), pq, tm) == E
    assert call_tensor(picture(), tensor(), pq, tm) == E
    assert call_tensor_rs(picture(), tensor(), pq, tm, Resample("catmull_rom")) == E
    assert both(pq, tm, YuvTarget()) == (E, E)
    assert call_tables(tm, pq) == 0
    # a malformed description is still reported as such
    assert call_pic(picture(), image(OUT_RGB_PLANAR), MiColorInfo(2, 18, 9, 0, 0), tm) == E
    assert call_pic(picture(), image(OUT_RGB_PLANAR), MiColorInfo(4, 18, 9, 0, 0), tm) == NS


def test_tables_accepted():
    for pri in (1, 5, 6, 7, 9, 12):
        for src_bpc in (8, 10, 12):
            for tm in (ToneMap(), ToneMap(9, 1, 10, 0.0, 1.0), ToneMap(12, 13, 12, -1.0, 10000.0)):
                assert call_hlg(tm, MiColorInfo(pri, 18, 9, 0, 0), src_bpc) == 0


def test_tables_null_arguments():
    assert call_hlg(None, HLG) == E
    assert call_hlg(ToneMap(), None) == E
    for i in range(5):
        out = list(BUFS)
        out[i] = None
        assert call_hlg(ToneMap(), HLG, 10, out) == E, i


@pytest.mark.parametrize("src_bpc", [9, 0, 16, -8, 11])
def test_tables_source_depth(src_bpc):
    assert call_hlg(ToneMap(), HLG, src_bpc) == E


@pytest.mark.parametrize("trc", [16, 1, 13, 14, 2, 0, 17, 8, 19, -1])
def test_tables_are_for_hlg_alone(trc):
    assert call_hlg(ToneMap(), MiColorInfo(9, trc, 9, 0, 0)) == E


@pytest.mark.parametrize("pri", [2, 0, 3, 13, 21, 23, -1])
def test_tables_unspecified_or_reserved_primaries(pri):
    assert call_hlg(ToneMap(), MiColorInfo(pri, 18, 9, 0, 0)) == E


@pytest.mark.parametrize("pri", [4, 8, 10, 11, 22])
def test_tables_other_defined_primaries(pri):
    assert call_hlg(ToneMap(), MiColorInfo(pri, 18, 9, 0, 0)) == NS


@pytest.mark.parametrize("field,value", [("dst_pri", 2), ("dst_pri", 5), ("dst_pri", 6), ("dst_pri", 0), ("dst_trc", 16),
                                         ("dst_trc", 18), ("dst_trc", 2), ("dst_trc", 14), ("dst_bpc", 9), ("dst_bpc", 16),
                                         ("dst_bpc", 0)])
def test_tables_destination_outside_the_lists(field, value):
    tm = ToneMap()
    setattr(tm, field, value)
    assert call_hlg(tm, HLG) == E


@pytest.mark.parametrize("peak", BAD_PEAKS)
def test_tables_dst_peak(peak):
    assert call_hlg(ToneMap(dst_peak=peak), HLG) == E


def test_tables_dst_peak_limits_are_inclusive():
    assert call_hlg(ToneMap(dst_peak=1.0), HLG) == 0
    assert call_hlg(ToneMap(dst_peak=10000.0), HLG) == 0


@pytest.mark.parametrize("peak", BAD_PEAKS + [1000.0])
def test_tables_do_not_read_src_peak(peak):
    a, b = bufs(), bufs()
    assert call_hlg(ToneMap(src_peak=1000.0, dst_peak=203.0), HLG, 10, a) == 0
    assert call_hlg(ToneMap(src_peak=peak, dst_peak=203.0), HLG, 10, b) == 0
    assert all(bytes(x) == bytes(y) for x, y in zip(a, b))


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


_model_in = {}


@pytest.mark.parametrize("pri", [1, 5, 6, 7, 9, 12])
@pytest.mark.parametrize("src_bpc", [8, 10, 12])
def test_tables_equal_the_model(src_bpc, pri):
    """Every (source depth, pri) under every destination and peak: lut_in reads the depth alone, yw
    the primaries, m the two primaries, lut_out (dst_trc, dst_bpc), lut_gain the peak."""
    color = MiColorInfo(pri, 18, 9, 0, 0)
    if src_bpc not in _model_in:
        _model_in[src_bpc] = H.table_in(src_bpc)
    n = 0
    for dst_pri in (1, 9, 12):
        for dst_trc in (1, 13):
            for dst_bpc in (8, 10, 12):
                peak = PEAKS[n % len(PEAKS)]
                n += 1
                lut_in, m, lut_out, yw, lut_gain = tonemap_tables_hlg(ToneMap(dst_pri, dst_trc, dst_bpc, math.nan, peak), color, src_bpc)
                _, w_m, w_out, w_yw, w_gain = H.tables(pri, 8, dst_pri, dst_trc, dst_bpc, peak)
                what = (src_bpc, pri, dst_pri, dst_trc, dst_bpc, peak)
                assert same_bits(lut_in, _model_in[src_bpc]), what
                assert same_bits(m, w_m), what
                assert same_bits(lut_out, w_out), what
                assert same_bits(yw, w_yw), what
                assert same_bits(lut_gain, w_gain), what
                assert lut_in[0] == 0.0 and lut_in[-1] == 1.0 and np.all(np.diff(lut_in) >= 0)
                assert lut_gain[1536] == 1.0 and lut_gain[1537] == 1.0
                if pri == dst_pri:
                    assert np.array_equal(m, np.eye(3, dtype=np.float32))


@pytest.mark.parametrize("dst_peak", PEAKS + [1.0, 301.0])
def test_gain_table_equals_the_model_at_every_peak(dst_peak):
    lut_gain = tonemap_tables_hlg(ToneMap(dst_peak=dst_peak), HLG, 8)[4]
    assert same_bits(lut_gain, H.table_gain(dst_peak))
    # gamma crosses 1 near 301 nits: the gain falls with Y below it and rises above it
    assert (lut_gain[0] > 1.0) == (H.gamma(dst_peak) < 1.0)
