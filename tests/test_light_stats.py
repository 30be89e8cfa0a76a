"""CPU, no device: mi_light_level_stats against a numpy restatement of include/mi_av1out.h, the
PeakTracker and the metadata selection of rav1d_amd.stream, and the host-side rejections of
mi_picture_light_level (the context is NULL, as in tests/test_display_args.py: a call whose other
arguments pass is -EINVAL for that alone)."""
import ctypes
import errno
import math

import numpy as np
import pytest

from rav1d_amd import MiError, MiPicture
from rav1d_amd.av1dec import MiColorInfo, MiContentLight, MiDecEvent, MiMasteringDisplay
from rav1d_amd.display import ToneMap, _light_lib, light_stats
from rav1d_amd.stream import PeakTracker, decode_to_ladder, decode_to_tensors, metadata_peak

M1, M2, C1, C2, C3 = 2610 / 16384, 2523 / 32, 3424 / 4096, 2413 / 128, 2392 / 128


def pq_eotf(e):
    p = e ** (1 / M2)
    return 10000.0 * (max(p - C1, 0.0) / (C2 - C3 * p)) ** (1 / M1)


def model(hist, bpc, percentile):
    """(max_code, pct_code, max_nits, pct_nits, avg_nits) as the header states them."""
    hist = np.asarray(hist, dtype=np.uint64)
    n = int(hist.sum())
    top = (1 << bpc) - 1
    want = math.ceil(percentile / 100 * n)
    cum = np.cumsum(hist)
    max_code = int(np.nonzero(hist)[0][-1])
    pct_code = int(np.nonzero(cum >= want)[0][0])
    s = 0.0
    for c in range(top + 1):
        s += float(hist[c]) * pq_eotf(c / top)
    return max_code, pct_code, pq_eotf(max_code / top), pq_eotf(pct_code / top), s / n


def check(hist, bpc, percentile):
    got = light_stats(np.asarray(hist, dtype=np.uint32), bpc, percentile)
    mc, pc, mn, pn, avg = model(hist, bpc, percentile)
    assert (got.max_code, got.pct_code) == (mc, pc)
    for a, b in ((got.max_nits, mn), (got.pct_nits, pn), (got.avg_nits, avg)):
        assert a == pytest.approx(b, rel=1e-12, abs=1e-300)
    return got


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_one_bin(bpc):
    n = 1 << bpc
    h = np.zeros(n, dtype=np.uint32)
    h[0] = 12345
    got = check(h, bpc, 99.99)
    assert (got.max_code, got.pct_code) == (0, 0) and got.max_nits == 0.0 and got.avg_nits == 0.0
    h[:] = 0
    h[n - 1] = 7
    got = check(h, bpc, 50.0)
    assert (got.max_code, got.pct_code) == (n - 1, n - 1)
    for v in (got.max_nits, got.pct_nits, got.avg_nits):
        assert v == pytest.approx(10000.0, rel=1e-9)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_percentile_boundary(bpc):
    """Two bins of 9000 and 1000 pixels: ceil(p / 100 N) on the cumulative step, and one count
    either side of it."""
    n = 1 << bpc
    lo, hi = n // 5, n - 3
    h = np.zeros(n, dtype=np.uint32)
    h[lo], h[hi] = 9000, 1000
    assert check(h, bpc, 90.0).pct_code == lo            # the 9000th pixel: the last of the low bin
    assert check(h, bpc, 89.99).pct_code == lo           # the 8999th
    assert check(h, bpc, 90.01).pct_code == hi           # the 9001st
    assert check(h, bpc, 100.0).pct_code == hi
    assert check(h, bpc, 1e-9).pct_code == lo            # ceil: the first pixel
    got = check(h, bpc, 99.99)
    assert got.max_code == hi and got.avg_nits == pytest.approx(0.9 * pq_eotf(lo / (n - 1)) + 0.1 * got.max_nits, rel=1e-12)


def test_random_histograms():
    rng = np.random.default_rng(5)
    for bpc in (8, 10, 12):
        h = rng.integers(0, 1 << 20, 1 << bpc).astype(np.uint32)
        h[rng.integers(0, 1 << bpc, (1 << bpc) // 2)] = 0
        for p in (0.01, 50.0, 99.99, 100.0):
            check(h, bpc, p)
    # counts beyond 2^31 are unsigned, and their sum passes 2^32
    h = np.zeros(256, dtype=np.uint32)
    h[10], h[200] = 0xffffffff, 0xfffffff0
    assert check(h, 8, 50.0).pct_code == 10 and check(h, 8, 50.1).pct_code == 200
    # the bits of light_level's int32 tensor are those counts
    assert light_stats(h.view(np.int32), 8, 50.1).pct_code == 200


def test_einval():
    h = np.zeros(1024, dtype=np.uint32)
    with pytest.raises(MiError):
        light_stats(h, 10, 99.99)                        # empty
    h[3] = 1
    for p in (0.0, -1.0, 100.0001, float("nan")):
        with pytest.raises(MiError):
            light_stats(h, 10, p)
    L = _light_lib()
    out = (ctypes.c_double * 8)()
    hp = h.ctypes.data_as(ctypes.c_void_p)
    assert L.mi_light_level_stats(hp, 10, 99.99, out) == 0
    assert L.mi_light_level_stats(None, 10, 99.99, out) == -errno.EINVAL
    assert L.mi_light_level_stats(hp, 10, 99.99, None) == -errno.EINVAL
    for bpc in (0, 9, 16):
        assert L.mi_light_level_stats(hp, bpc, 99.99, out) == -errno.EINVAL


# ---- PeakTracker ----

def test_tracker_attack_and_release():
    t = PeakTracker(100.0)
    assert t.update(250.0) == 300.0                       # the first measurement, raised to the quantum
    assert t.update(1000.0) == 1000.0                     # rising input passes at once
    assert t.update(4000.0) == 4000.0
    s, outs = 4000.0, []
    for _ in range(40):                                   # falling input decays by sixteenths
        s = s + (200.0 - s) / 16
        outs.append(t.update(200.0))
        assert t.s == s and outs[-1] == math.ceil(s / 100) * 100
    assert outs == sorted(outs, reverse=True) and outs[0] == 3800.0 and outs[-1] < 600.0
    assert t.update(700.0) == 700.0                       # and a rise is taken at once again


def test_tracker_quantum_and_clamp():
    rng = np.random.default_rng(9)
    for dst in (100.0, 203.0, 1.0, 600.0):
        t = PeakTracker(dst)
        lo = max(100.0, dst)
        for m in list(rng.uniform(0, 12000, 200)) + [0.0, 1e-3, 10000.0, 20000.0]:
            v = t.update(m)
            assert lo <= v <= 10000.0
            assert v % 100 == 0 or v == lo
    assert PeakTracker(100.0).update(0.0) == 100.0
    assert PeakTracker(100.0).update(50000.0) == 10000.0
    assert PeakTracker(203.0).update(150.0) == 203.0


def test_tracker_constant_input():
    for m in (99.0, 100.0, 100.5, 987.6, 10000.0):
        t = PeakTracker(100.0)
        assert len({t.update(m) for _ in range(50)}) == 1    # no table rebuild within a scene


# ---- the "metadata" order ----

def event(mdcv=None, cll=None):
    ev = MiDecEvent()
    if mdcv is not None:
        ev.mastering_display = MiMasteringDisplay(present=1, max_luminance=mdcv)
    if cll is not None:
        ev.content_light = MiContentLight(present=1, max_cll=cll, max_fall=1)
    return ev


def test_metadata_order():
    tm = ToneMap(src_peak=1234.0)
    assert metadata_peak(event(mdcv=4000 << 8, cll=900), tm) == 4000.0
    assert metadata_peak(event(mdcv=(1000 << 8) + 128, cll=900), tm) == 1000.5      # 24.8 fixed point
    assert metadata_peak(event(mdcv=0, cll=900), tm) == 900.0                        # a zero is no value
    assert metadata_peak(event(cll=900), tm) == 900.0
    assert metadata_peak(event(mdcv=0, cll=0), tm) == 1234.0
    assert metadata_peak(event(), tm) == 1234.0
    ev = event(cll=900)
    ev.content_light.present = 0
    assert metadata_peak(ev, tm) == 1234.0
    assert tm.src_peak == 1234.0


def test_peak_argument_is_checked_before_decoding():
    for kw in ({"peak": "metadata"}, {"peak": "measured"}, {"peak": "bogus", "tonemap": ToneMap()}):
        with pytest.raises(ValueError):
            next(decode_to_ladder(None, b"", [(8, 8)], **kw))
        with pytest.raises(ValueError):
            next(decode_to_tensors(None, b"", format="rgb", **kw))


# ---- mi_picture_light_level without a context ----

BUF = (ctypes.c_uint8 * (1 << 16))()
P = ctypes.addressof(BUF)
HIST = ctypes.c_void_p(P + 32768)
BT709 = MiColorInfo(1, 1, 1, 0, 0)


def picture(w=32, h=16, bpc=8, layout=1):
    pic = MiPicture()
    for p in range(3):
        pic.data[p] = P + 4096 * p
    pic.stride[0], pic.stride[1] = 128 * (1 if bpc == 8 else 2), 128 * (1 if bpc == 8 else 2)
    pic.w, pic.h, pic.bpc, pic.layout = w, h, bpc, layout
    return pic


def call(pic, color=BT709, hist=HIST, variant=None):
    pp = ctypes.byref(pic) if pic is not None else None
    cp = ctypes.byref(color) if color is not None else None
    if variant is not None:
        return _light_lib().mi_picture_light_level_variant(None, pp, cp, hist, variant, None)
    return _light_lib().mi_picture_light_level(None, pp, cp, hist, None)


def test_light_level_rejections():
    E = -errno.EINVAL
    assert call(picture()) == E                                   # only the context is missing
    assert call(None) == E
    assert call(picture(), hist=None) == E
    assert call(picture(), color=None) == E
    assert call(picture(), MiColorInfo(2, 2, 2, 0, 0)) == E       # unspecified: the caller chooses
    assert call(picture(), MiColorInfo(1, 1, 1, 2, 0)) == E       # range
    assert call(picture(), MiColorInfo(1, 1, 3, 0, 0)) == E       # reserved matrix
    for layout in (0, 1, 2):
        assert call(picture(layout=layout), MiColorInfo(1, 13, 0, 1, 0)) == E   # identity needs 4:4:4
    for m in (8, 10, 11, 12, 13, 14):
        assert call(picture(), MiColorInfo(1, 1, m, 0, 0)) == -errno.ENOTSUP
    for bad in (dict(w=0), dict(h=0), dict(w=65537), dict(bpc=9), dict(layout=4), dict(w=200)):
        assert call(picture(**bad)) == E                          # (w 200: the stride holds 128)
    big = picture(w=65536, h=65536)                               # w h = 2^32: a bin could not hold it
    big.stride[0] = big.stride[1] = 65536
    assert call(big) == E
    big.h = 65535
    big.data[0] = None
    assert call(big) == E
    for v in (-1, 3):
        assert call(picture(), variant=v) == E
