"""CPU, no device: mi_display_yuv_tm and mi_display_scaled_tm check their arguments on the host
before any device work, the NULL context last (as tests/test_tonemap_args.py and
tests/test_scaled_args.py): a call whose other arguments pass is -EINVAL for the context alone, so
every refusal below differs from an accepted call in one thing, and an -ENOTSUP can only come from
the rule under test."""
import ctypes
import errno
import math

import pytest

from rav1d_amd import lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import OUT_RGB_PLANAR, OUT_RGBA_PACKED, OUT_SEMIPLANAR, MiResample, Resample, ToneMap, YuvTarget
from tests import test_scaled_args as SA
from tests.test_display_args import image, picture

E, NS = -errno.EINVAL, -errno.ENOTSUP
HDR10 = MiColorInfo(9, 16, 9, 0, 0)
SDR = MiColorInfo(1, 1, 1, 0, 0)


def ref(x):
    return ctypes.byref(x) if x is not None else None


def call_yuv(pic, im, color, tm, target):
    return lib().mi_display_yuv_tm(None, ref(pic), ref(im), ref(color), ref(tm), ref(target), None, None)


def call_scaled(case, color, tm, target, rs=None):
    """mi_display_scaled_tm on a case of tests/test_scaled_args.py with `color` in place of its own
    (the case's chr kept)."""
    pic = SA.picture(case)
    (p, outs, n, col, fg, st), _keep = SA.arguments(case, pic, SA.P + 98304, SA.P + 98304 + 8192)
    if col is None:
        color = None
    elif color is not None:
        color = MiColorInfo(color.pri, color.trc, color.mtrx, color.range, dict(SA.BASE, **case)["chr"])
    return lib().mi_display_scaled_tm(None, p, outs, n, ref(color), ref(tm), ref(target), ref(rs), fg, st)


def both(color, tm, target, src_bpc=10, layout=1):
    """The two entries' answers for one (color, tm, target), everything else accepted."""
    dst = tm.dst_bpc if tm is not None and tm.dst_bpc in (8, 10, 12) else 8
    return (call_yuv(picture(bpc=src_bpc, layout=layout), image(OUT_SEMIPLANAR, bpc=dst), color, tm, target),
            call_scaled(dict(bpc=src_bpc, layout=layout), color, tm, target))


def test_accepted_without_a_context():
    for color in (HDR10, SDR, MiColorInfo(5, 6, 6, 1, 2), MiColorInfo(12, 13, 1, 1, 0)):
        for tm in (ToneMap(), ToneMap(9, 1, 10), ToneMap(12, 13, 12, 4000.0, 1000.0)):
            for src_bpc in (8, 10, 12):
                for target in (YuvTarget(), YuvTarget(9, 1), YuvTarget(6, 0)):
                    assert both(color, tm, target, src_bpc) == (E, E)
    for mtrx in (1, 4, 5, 6, 7, 9):
        for rng in (0, 1):
            assert both(HDR10, ToneMap(), YuvTarget(mtrx, rng)) == (E, E)
    # every layout; a GBR source (4:4:4) is a source like any other
    for layout in range(4):
        assert both(HDR10, ToneMap(), YuvTarget(), layout=layout) == (E, E)
    assert both(MiColorInfo(9, 16, 0, 1, 0), ToneMap(), YuvTarget(), layout=3) == (E, E)
    # 4:0:0 does not read data[1]
    assert call_yuv(picture(layout=0), image(OUT_SEMIPLANAR, planes=1), SDR, ToneMap(), YuvTarget()) == E
    # a rung's depth is free; the filter is mi_display_scaled_rs's
    for obpc in (8, 10, 12):
        assert call_scaled(dict(bpc=10, obpc=obpc), HDR10, ToneMap(dst_bpc=10), YuvTarget()) == E
    assert call_scaled({}, SDR, ToneMap(), YuvTarget(), Resample("mitchell")) == E


@pytest.mark.parametrize("case", [c for _, c in SA.PASSING if c.get("null") != "color"],
                         ids=[n for n, c in SA.PASSING if c.get("null") != "color"])
def test_scaled_cases_that_pass(case):
    assert call_scaled(case, SDR, ToneMap(), YuvTarget()) == E


@pytest.mark.parametrize("case", [c for _, c in SA.REJECTED], ids=[n for n, _ in SA.REJECTED])
def test_scaled_rules_still_apply(case):
    assert call_scaled(case, SDR, ToneMap(), YuvTarget()) == E


def test_null_tonemap_or_target():
    assert both(HDR10, None, YuvTarget()) == (E, E)
    assert both(HDR10, ToneMap(), None) == (E, E)
    # (a trc the stage does not support: still the NULL argument's -EINVAL)
    assert both(MiColorInfo(9, 18, 9, 0, 0), None, YuvTarget()) == (E, E)


def test_null_color():
    assert both(None, ToneMap(), YuvTarget()) == (E, E)
    assert call_scaled(dict(null="color"), SDR, ToneMap(), YuvTarget()) == E


@pytest.mark.parametrize("mtrx", [0, 2, 8, 10, 15, 3, 11, 12, 13, 14, -1, 255])
def test_target_matrix_outside_the_list(mtrx):
    """Identity, unspecified, the defined matrices without Kr / Kb and reserved values alike."""
    assert both(HDR10, ToneMap(), YuvTarget(mtrx, 0)) == (E, E)
    assert both(SDR, ToneMap(), YuvTarget(mtrx, 1), layout=3) == (E, E)


@pytest.mark.parametrize("rng", [2, -1, 3])
def test_target_range(rng):
    assert both(HDR10, ToneMap(), YuvTarget(1, rng)) == (E, E)


@pytest.mark.parametrize("trc", [18, 8, 4, 17])
def test_unsupported_source_transfer(trc):
    """HLG among them: defined, not converted."""
    assert both(MiColorInfo(9, trc, 9, 0, 0), ToneMap(), YuvTarget()) == (NS, NS)


@pytest.mark.parametrize("pri", [4, 8, 22])
def test_unsupported_source_primaries(pri):
    assert both(MiColorInfo(pri, 16, 9, 0, 0), ToneMap(), YuvTarget()) == (NS, NS)


@pytest.mark.parametrize("color", [MiColorInfo(2, 16, 9, 0, 0), MiColorInfo(0, 16, 9, 0, 0), MiColorInfo(9, 2, 9, 0, 0),
                                   MiColorInfo(9, 19, 9, 0, 0)], ids=["pri2", "pri0", "trc2", "trc19"])
def test_unspecified_or_reserved_source(color):
    assert both(color, ToneMap(), YuvTarget()) == (E, E)


@pytest.mark.parametrize("peak", [0.0, 0.5, 10000.5, math.inf, math.nan])
def test_bad_pq_peak(peak):
    assert both(HDR10, ToneMap(src_peak=peak), YuvTarget()) == (E, E)
    assert both(HDR10, ToneMap(dst_peak=peak), YuvTarget()) == (E, E)
    assert both(SDR, ToneMap(src_peak=peak, dst_peak=peak), YuvTarget()) == (E, E)      # not read: the context alone


@pytest.mark.parametrize("field,value", [("dst_pri", 2), ("dst_pri", 5), ("dst_trc", 16), ("dst_trc", 2), ("dst_bpc", 9),
                                         ("dst_bpc", 16), ("dst_bpc", 0)])
def test_destination_outside_the_lists(field, value):
    tm = ToneMap()
    setattr(tm, field, value)
    assert both(HDR10, tm, YuvTarget()) == (E, E)


def test_source_matrix_rules():
    """display_color's: the source's matrix is the one the picture is decoded with."""
    for color, want in ((MiColorInfo(9, 16, 2, 0, 0), E), (MiColorInfo(9, 16, 9, 2, 0), E), (MiColorInfo(9, 16, 3, 0, 0), E),
                        (MiColorInfo(9, 16, 0, 1, 0), E),      # identity needs 4:4:4
                        (MiColorInfo(9, 16, 8, 0, 0), NS), (MiColorInfo(9, 16, 14, 0, 0), NS)):
        assert both(color, ToneMap(), YuvTarget()) == (want, want)


def test_yuv_format_and_depth():
    tm, t = ToneMap(), YuvTarget()
    for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED, 3, -1):
        assert call_yuv(picture(bpc=10), image(fmt), HDR10, tm, t) == E
    # out->bpc must be dst_bpc
    assert call_yuv(picture(bpc=10), image(OUT_SEMIPLANAR, bpc=10), HDR10, ToneMap(dst_bpc=8), t) == E
    assert call_yuv(picture(bpc=10), image(OUT_SEMIPLANAR, bpc=8), HDR10, ToneMap(dst_bpc=10), t) == E
    assert call_yuv(picture(bpc=8), image(OUT_SEMIPLANAR, bpc=12), SDR, ToneMap(dst_bpc=8), t) == E
    assert call_yuv(picture(bpc=8), image(OUT_SEMIPLANAR, bpc=9), SDR, ToneMap(dst_bpc=8), t) == E
    for src_bpc in (8, 10, 12):
        for dst_bpc in (8, 10, 12):
            assert call_yuv(picture(bpc=src_bpc), image(OUT_SEMIPLANAR, bpc=dst_bpc), HDR10, ToneMap(dst_bpc=dst_bpc), t) == E


def test_yuv_destination_and_source():
    tm, t = ToneMap(), YuvTarget()
    assert call_yuv(None, image(OUT_SEMIPLANAR), HDR10, tm, t) == E
    assert call_yuv(picture(), None, HDR10, tm, t) == E
    assert call_yuv(picture(), image(OUT_SEMIPLANAR, w=31), HDR10, tm, t) == E
    assert call_yuv(picture(), image(OUT_SEMIPLANAR, h=17), HDR10, tm, t) == E
    assert call_yuv(picture(bpc=9), image(OUT_SEMIPLANAR), HDR10, tm, t) == E
    assert call_yuv(picture(), image(OUT_SEMIPLANAR, planes=0), HDR10, tm, t) == E
    for layout in (1, 2, 3):      # NULL data[1] with a chroma layout
        assert call_yuv(picture(layout=layout), image(OUT_SEMIPLANAR, planes=1), HDR10, tm, t) == E
    # rows of the destination's sample type: 32 Y samples, 16 UV pairs
    assert call_yuv(picture(bpc=10), image(OUT_SEMIPLANAR, stride=31), HDR10, tm, t) == E
    assert call_yuv(picture(bpc=8), image(OUT_SEMIPLANAR, bpc=10, stride=62), SDR, ToneMap(dst_bpc=10), t) == E
    assert call_yuv(picture(bpc=8), image(OUT_SEMIPLANAR, bpc=10, stride=65), SDR, ToneMap(dst_bpc=10), t) == E
    assert call_yuv(picture(layout=3), image(OUT_SEMIPLANAR, stride=63), HDR10, tm, t) == E      # 4:4:4: 32 pairs
    assert call_yuv(picture(layout=3), image(OUT_SEMIPLANAR, stride=64), HDR10, tm, t) == E      # (passes: the context)
    src = picture()
    src.stride[0] = 31
    assert call_yuv(src, image(OUT_SEMIPLANAR), HDR10, tm, t) == E


def test_scaled_filter_rules():
    assert call_scaled({}, SDR, ToneMap(), YuvTarget(), MiResample(2, 0.0, 0.5)) == E
    assert call_scaled({}, SDR, ToneMap(), YuvTarget(), MiResample(1, 1.5, 0.5)) == E


def test_existing_entries_keep_their_answers():
    """Semi-planar on mi_display_picture_tm stays -ENOTSUP."""
    from tests.test_tonemap_args import call_pic
    assert call_pic(picture(), image(OUT_SEMIPLANAR), HDR10, ToneMap()) == NS
