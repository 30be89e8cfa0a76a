"""GPU: mi_picture_light_level (include/mi_av1out.h, csrc/light.hip): the histogram of
max(R', G', B') of the planar R'G'B' picture, bit for bit np.bincount over tests/display_ref.py's
integer model. `hist` lies inside a larger buffer whose guard words must stay untouched, and the
counts always sum to w h."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import check
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import _light_lib, light_level, light_stats
from tests import display_ref as R
from tests.test_display_gpu import make_planes
from tests.test_lr_gpu import to_frame

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0x5A5A5A5A
# (mtrx, full range, chr): matrices 1, 6 and 9, both ranges, every chroma siting
COMBOS = [(1, 0, 0), (1, 1, 2), (6, 0, 1), (6, 1, 0), (9, 0, 2), (9, 1, 1)]


def want_hist(planes, bpc, layout, mtrx, full, chr):
    rgb = R.to_rgb(planes, bpc, layout, mtrx, full, chr)
    return np.bincount(rgb.max(axis=0).ravel(), minlength=1 << bpc)


class Hist:
    """1 << bpc counts with GUARD words of FILL on either side, prefilled with FILL too (the
    entry zeroes what it owns)."""

    def __init__(self, bpc):
        self.n = 1 << bpc
        self.buf = torch.full((self.n + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")

    def run(self, gpu, src, color, variant=None):
        pic = src.picture()
        p = ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)
        if variant is None:
            check(_light_lib().mi_picture_light_level(gpu.h, ctypes.byref(pic), ctypes.byref(color), p, None), "light")
        else:
            check(_light_lib().mi_picture_light_level_variant(gpu.h, ctypes.byref(pic), ctypes.byref(color), p, variant, None),
                  "light variant")
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy().view(np.uint32)
        assert np.all(host[:GUARD] == FILL) and np.all(host[GUARD + self.n:] == FILL), "guard words"
        return host[GUARD:GUARD + self.n].astype(np.int64)


def check_case(gpu, planes, w, h, bpc, layout, combos, variants=(None,)):
    src = to_frame(planes, w, h, bpc, layout)
    hist = Hist(bpc)
    for mtrx, full, chr in combos:
        want = want_hist(planes, bpc, layout, mtrx, full, chr)
        for v in variants:
            got = hist.run(gpu, src, MiColorInfo(1, 16, mtrx, full, chr), v)
            assert got.sum() == w * h, (mtrx, full, chr, v)
            assert np.array_equal(got, want), (mtrx, full, chr, v)


def combos_for(layout, k):
    """Two of COMBOS per case, rotating, and the identity on 4:4:4."""
    c = [COMBOS[k % 6], COMBOS[(k + 3) % 6]]
    return c + ([(0, 1, 0)] if layout == 3 else [])


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_small_sizes(gpu, layout, bpc):
    rng = np.random.default_rng(100 * layout + bpc)
    for k, (w, h) in enumerate([(1, 1), (2, 2), (17, 9), (24, 19)]):
        for kind in ("random", "blocks"):
            check_case(gpu, make_planes(rng, w, h, bpc, layout, kind), w, h, bpc, layout, combos_for(layout, k + bpc))


@pytest.mark.parametrize("layout", [1, 3])
@pytest.mark.parametrize("bpc", [8, 10])
def test_every_combination(gpu, bpc, layout):
    """Every siting, both ranges, matrices 1, 6, 9 (and the identity), in all three counting variants."""
    rng = np.random.default_rng(7 * layout + bpc)
    w, h = 40, 22
    combos = COMBOS + ([(0, 1, 0), (0, 0, 2)] if layout == 3 else [])
    check_case(gpu, make_planes(rng, w, h, bpc, layout, "random"), w, h, bpc, layout, combos, (None, 0, 1, 2))


# 521 x 5; the workgroup's 512 columns from either side; pictures with more tiles of 4 row units than
# the kernel launches workgroups (1024, split between the columns of workgroups), so that each walks
# two tiles, the last one ragged: 4100 and 8201 rows under one column of workgroups, 1400 under three
@pytest.mark.parametrize("size, layout, bpc", [((521, 5), 1, 10), ((511, 6), 2, 8), ((512, 7), 1, 12), ((513, 4), 3, 10),
                                               ((1025, 3), 1, 8), ((8, 4100), 3, 8), ((1030, 1400), 3, 10),
                                               ((14, 8201), 1, 10)])
def test_workgroup_edges(gpu, size, layout, bpc):
    w, h = size
    rng = np.random.default_rng(w + h)
    check_case(gpu, make_planes(rng, w, h, bpc, layout, "random"), w, h, bpc, layout, combos_for(layout, w)[:2])


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("layout", [0, 1, 3])
def test_flat_and_checkerboard(gpu, layout, bpc):
    """A constant picture (one bin holds w h: every lane of every wave adds to it) at code 0, at
    mid and at the top, and a two-value checkerboard (no two neighbours equal)."""
    m, w, h = (1 << bpc) - 1, 530, 37
    cw, ch = R.chroma_size(w, h, layout)
    dt = np.uint8 if bpc == 8 else np.uint16
    for k, v in enumerate((0, 1 << (bpc - 1), m)):
        planes = [np.full((h, w), v, dt)] + ([np.full((ch, cw), 1 << (bpc - 1), dt)] * 2 if layout else [])
        src = to_frame(planes, w, h, bpc, layout)
        for mtrx, full, chr in ((1, 1, 0), (9, 0, 2)):
            for variant in (None, 0, 1):
                got = Hist(bpc).run(gpu, src, MiColorInfo(9, 16, mtrx, full, chr), variant)
                assert np.array_equal(got, want_hist(planes, bpc, layout, mtrx, full, chr))
                assert np.count_nonzero(got) == 1 and got.max() == w * h
    yy, xx = np.mgrid[0:h, 0:w]
    board = np.where((xx + yy) & 1, m - 3, 5).astype(dt)
    planes = [board] + ([np.full((ch, cw), 1 << (bpc - 1), dt)] * 2 if layout else [])
    check_case(gpu, planes, w, h, bpc, layout, [(1, 1, 0), (6, 0, 1)], (None, 0, 1))


def test_every_bin(gpu):
    """64 x 64 at 8 bits, the luma walking through every code: every bin is flushed."""
    planes = [(np.arange(64 * 64) % 256).astype(np.uint8).reshape(64, 64)]
    src = to_frame(planes, 64, 64, 8, 0)
    got = Hist(8).run(gpu, src, MiColorInfo(1, 16, 1, 1, 0))
    assert np.all(got == 16) and np.array_equal(got, want_hist(planes, 8, 0, 1, 1, 0))


def test_calls_do_not_accumulate(gpu):
    """Two calls in a row on one hist; then 12 bits followed by 8 bits on one context."""
    rng = np.random.default_rng(3)
    w, h = 70, 30
    a = make_planes(rng, w, h, 12, 1, "random")
    b = make_planes(rng, w, h, 12, 1, "blocks")
    color = MiColorInfo(9, 16, 9, 0, 0)
    hist = Hist(12)
    assert np.array_equal(hist.run(gpu, to_frame(a, w, h, 12, 1), color), want_hist(a, 12, 1, 9, 0, 0))
    assert np.array_equal(hist.run(gpu, to_frame(b, w, h, 12, 1), color), want_hist(b, 12, 1, 9, 0, 0))
    c = make_planes(rng, w, h, 8, 1, "random")
    assert np.array_equal(Hist(8).run(gpu, to_frame(c, w, h, 8, 1), color), want_hist(c, 8, 1, 9, 0, 0))


def test_python_entry(gpu):
    """light_level returns the counts as an int32 tensor; light_stats reads it."""
    rng = np.random.default_rng(11)
    w, h = 33, 21
    planes = make_planes(rng, w, h, 10, 1, "random")
    color = MiColorInfo(9, 16, 9, 0, 0)
    t = light_level(gpu, to_frame(planes, w, h, 10, 1), color)
    assert t.dtype == torch.int32 and t.shape == (1024,) and t.is_cuda
    want = want_hist(planes, 10, 1, 9, 0, 0)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want)
    s = light_stats(t, 10, 100.0)
    assert s.max_code == s.pct_code == int(np.nonzero(want)[0][-1])
