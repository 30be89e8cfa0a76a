"""CPU, no device: the argument checks of the resampling entries (include/mi_av1out.h):
mi_display_tensor_rs and mi_display_scaled_rs check the filter on the host before any device work,
with the NULL context checked last, and the checks of the entries without a filter reach them
unchanged (the cases of tests/test_tensor_args.py and tests/test_scaled_args.py); mi_resample_plan
and mi_resample_taps are host-only. tests/test_resample_gpu.py runs the filters of BAD and GOOD
again with a live context, where GOOD returns 0."""
import ctypes
import errno
import math

import numpy as np
import pytest

from rav1d_amd import lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import RS_CUBIC, RS_TRIANGLE, MiResample, MiToneMap, Resample, resample_plan
from tests import test_scaled_args as SA
from tests import test_tensor_args as TA

E = -errno.EINVAL
ENOTSUP = -errno.ENOTSUP

BAD = [("filter 2", MiResample(2, 0.0, 0.5)), ("filter -1", MiResample(-1, 0.0, 0.5)),
       ("b nan", MiResample(RS_CUBIC, math.nan, 0.5)), ("c nan", MiResample(RS_CUBIC, 0.0, math.nan)),
       ("b inf", MiResample(RS_CUBIC, math.inf, 0.5)), ("c inf", MiResample(RS_CUBIC, 0.0, math.inf)),
       ("c -inf", MiResample(RS_CUBIC, 0.0, -math.inf)),
       ("b -0.01", MiResample(RS_CUBIC, -0.01, 0.5)), ("c -0.01", MiResample(RS_CUBIC, 0.0, -0.01)),
       ("b 1.01", MiResample(RS_CUBIC, 1.01, 0.5)), ("c 1.01", MiResample(RS_CUBIC, 0.0, 1.01))]
GOOD = [("NULL", None), ("triangle", Resample("triangle")), ("triangle, b and c not read", MiResample(RS_TRIANGLE, math.nan, 7.0)),
        ("catmull_rom", Resample("catmull_rom")), ("mitchell", Resample("mitchell")), ("cubic_075", Resample("cubic_075")),
        ("(0, 0)", Resample("cubic", 0.0, 0.0)), ("(1, 1)", Resample("cubic", 1.0, 1.0))]


def ref(x):
    return ctypes.byref(x) if x is not None else None


def tensor_rs(pic, im, color=TA.UNSUP, tm=None, rs=None):
    return lib().mi_display_tensor_rs(None, ref(pic), ref(im), ref(color), ref(tm), ref(rs), None, None)


def scaled_rs(case, rs):
    pic = SA.picture(case)
    args, _keep = SA.arguments(case, pic, SA.P + 98304, SA.P + 98304 + 8192)
    return lib().mi_display_scaled_rs(None, *args[:4], ref(rs), *args[4:])


@pytest.mark.parametrize("rs", [r for _, r in BAD], ids=[n for n, _ in BAD])
def test_bad_filter(rs):
    """With the unsupported matrix a call whose other arguments pass is -ENOTSUP, so -EINVAL is the
    filter's; mi_display_scaled_rs has no such rule and is -EINVAL either way (the GPU test tells
    the two apart with a live context)."""
    assert tensor_rs(TA.picture(), TA.image(), rs=rs) == E
    assert scaled_rs({}, rs) == E
    cap, seg = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib().mi_resample_plan(ref(rs), 17, 5, ctypes.byref(cap), ctypes.byref(seg)) == E
    assert (cap.value, seg.value) == (-1, -1)
    buf = (ctypes.c_int32 * 64)()
    assert lib().mi_resample_taps(ref(rs), 4, 2, 2, 9, buf, buf, buf) == E


@pytest.mark.parametrize("rs", [r for _, r in GOOD], ids=[n for n, _ in GOOD])
def test_good_filter(rs):
    assert tensor_rs(TA.picture(), TA.image(), rs=rs) == ENOTSUP      # everything else passed
    assert tensor_rs(TA.picture(), TA.image(), MiColorInfo(1, 1, 1, 1, 0), rs=rs) == E   # the NULL context alone
    assert scaled_rs({}, rs) == E
    assert resample_plan(rs, 17, 5)[0] == (17 if rs is not None and rs.filter == RS_CUBIC else 9)


def test_tensor_checks_reach_the_new_entry(monkeypatch):
    """tests/test_tensor_args.py's cases through mi_display_tensor_rs, with no filter and with
    Mitchell: its `call` is swapped for the new entry and its tests run as they are."""
    for rs in (None, Resample("mitchell")):
        monkeypatch.setattr(TA, "call", lambda pic, im, color=TA.UNSUP, rs=rs: tensor_rs(pic, im, color, None, rs))
        TA.test_null_arguments()
        TA.test_source()
        TA.test_crop()
        TA.test_output_size_and_downscale_limit()
        TA.test_dtype()
        for dtype in (TA.T_F16, TA.T_BF16, TA.T_F32):
            TA.test_strides_and_alignment(dtype)
        TA.test_non_finite_scale_and_bias()
        TA.test_colour_errors()
        TA.test_enotsup()


def test_tone_checks_reach_the_new_entry():
    """tm non-NULL is mi_display_tensor_tm: its rules apply (dst_bpc 9, then a source trc that is
    unspecified); a passing tone map leaves the NULL context."""
    full = MiColorInfo(9, 16, 9, 0, 0)
    rs = Resample("catmull_rom")
    assert tensor_rs(TA.picture(bpc=10), TA.image(), full, MiToneMap(1, 13, 9, 1000.0, 100.0), rs) == E
    assert tensor_rs(TA.picture(bpc=10), TA.image(), MiColorInfo(9, 2, 9, 0, 0), MiToneMap(1, 13, 8, 1000.0, 100.0), rs) == E
    assert tensor_rs(TA.picture(bpc=10), TA.image(), MiColorInfo(9, 18, 9, 0, 0), MiToneMap(1, 13, 8, 1000.0, 100.0), rs) == ENOTSUP
    assert tensor_rs(TA.picture(bpc=10), TA.image(), full, MiToneMap(1, 13, 8, 1000.0, 100.0), rs) == E
    assert tensor_rs(TA.picture(bpc=10), TA.image(), full, MiToneMap(1, 13, 8, 1000.0, 100.0), MiResample(3, 0, 0)) == E


@pytest.mark.parametrize("case", [c for _, c in SA.REJECTED], ids=[n for n, _ in SA.REJECTED])
def test_scaled_rejected_cases_reach_the_new_entry(case):
    for rs in (None, Resample("mitchell")):
        assert scaled_rs(case, rs) == E


def test_scaled_passing_cases_but_for_the_context():
    for name, case in SA.PASSING:
        for rs in (None, Resample("catmull_rom")):
            assert scaled_rs(case, rs) == E, name


def test_host_only_calls():
    L = lib()
    rs = Resample("catmull_rom")
    cap, seg = ctypes.c_int(0), ctypes.c_int(0)
    assert L.mi_resample_plan(ref(rs), 17, 5, None, ctypes.byref(seg)) == E
    assert L.mi_resample_plan(ref(rs), 17, 5, ctypes.byref(cap), None) == E
    for n_in, n_out in ((0, 5), (17, 0), (-1, 5), (65537, 1100), (5, 65537), (321, 5), (641, 10)):
        assert L.mi_resample_plan(ref(rs), n_in, n_out, ctypes.byref(cap), ctypes.byref(seg)) == E, (n_in, n_out)
    assert L.mi_resample_plan(ref(rs), 320, 5, ctypes.byref(cap), ctypes.byref(seg)) == 0     # 64:1 exactly
    assert cap.value == 257
    assert L.mi_resample_plan(ref(rs), 17, 5, ctypes.byref(cap), ctypes.byref(seg)) == 0
    assert cap.value == 17 and seg.value >= 1
    n = cap.value
    start, count = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 5)()
    k = (ctypes.c_int32 * ((n + 3) * 5))(*([77] * ((n + 3) * 5)))
    assert L.mi_resample_taps(ref(rs), 17, 5, 2, n, None, count, k) == E
    assert L.mi_resample_taps(ref(rs), 17, 5, 2, n, start, None, k) == E
    assert L.mi_resample_taps(ref(rs), 17, 5, 2, n, start, count, None) == E
    for phase in (0, 1, 3, 8):
        assert L.mi_resample_taps(ref(rs), 17, 5, phase, n, start, count, k) == E
    assert L.mi_resample_taps(ref(rs), 17, 5, 2, n - 1, start, count, k) == E        # cap too small
    assert L.mi_resample_taps(None, 17, 5, 2, 8, start, count, k) == E               # the triangle needs 9
    assert L.mi_resample_taps(ref(rs), 641, 10, 2, 300, start, count, k) == E
    assert all(v == 77 for v in k)                                                   # nothing was written
    # a larger cap: the slots past the plan's are zero, and nothing past cap * n_out is written
    assert L.mi_resample_taps(ref(rs), 17, 5, 2, n + 2, start, count, k) == 0
    a = np.array(k[:]).reshape(n + 3, 5)
    assert np.all(a[:n + 2].sum(axis=0) == 1 << 18) and not np.any(a[n:n + 2]) and np.all(a[n + 2] == 77)
