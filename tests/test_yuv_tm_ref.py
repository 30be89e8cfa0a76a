"""CPU: the model of the tone-mapped YUV outputs (tests/yuv_tm_ref.py) has the properties the
header's definition of the picture Q promises: the forward matrix's anchors and its distance from
the float64 equations, and a decimation whose taps carry the siting display_ref's upsampler
assumes."""
import numpy as np
import pytest

from tests import display_ref as R
from tests import yuv_tm_ref as Q

CASES = [(m, r, d) for m in Q.TARGET_MATRICES for r in (0, 1) for d in (8, 10, 12)]
IDS = [f"mtrx{m}-range{r}-{d}bit" for m, r, d in CASES]
# (layout, chr): every subsampling, every siting of 4:2:0
SITINGS = [(1, 0), (1, 1), (1, 2), (2, 0), (3, 0)]


def span(rng, d):
    """(top of the luma range, lowest and highest nominal chroma code) of a range at depth d."""
    if rng:
        return (1 << d) - 1, 0, (1 << d) - 1
    return 235 << (d - 8), 16 << (d - 8), 240 << (d - 8)


@pytest.mark.parametrize("mtrx,rng,d", CASES, ids=IDS)
def test_anchors(mtrx, rng, d):
    md, half = (1 << d) - 1, 1 << (d - 1)
    (yr, yg, yb), ku, kv, yo = Q.coefficients(mtrx, rng, d)
    _, sy, _ = Q.scaling(rng, d)
    assert yr + yg + yb == int(np.floor(sy * (1 << Q.S) + 0.5))
    assert sum(ku) == 0 and sum(kv) == 0
    grey = np.arange(md + 1)
    y, u, v = Q.forward(np.stack([grey, grey, grey]), mtrx, rng, d)
    assert np.all(u == half) and np.all(v == half)
    assert y[0] == yo == (0 if rng else 16 << (d - 8))
    assert y[md] == span(rng, d)[0]
    assert np.all(np.diff(y) >= 0)


@pytest.mark.parametrize("mtrx,rng,d", CASES, ids=IDS)
def test_cube_corners_stay_within_a_code_of_the_nominal_range(mtrx, rng, d):
    md = (1 << d) - 1
    corners = np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)]).T * md
    y, u, v = Q.forward_sums(corners, mtrx, rng, d)
    top, lo, hi = span(rng, d)
    assert y.min() >= (0 if rng else 16 << (d - 8)) - 1 and y.max() <= top + 1
    for c in (u, v):
        # (full range: +0.5 of the span is code 2^(d-1) + Md / 2, half a code above Md)
        assert c.min() >= lo - 1 and c.max() <= hi + 1


@pytest.mark.parametrize("mtrx,rng,d", CASES, ids=IDS)
def test_integer_matrix_is_within_a_code_of_float64(mtrx, rng, d):
    """Each coefficient is off by at most (0.5 + 1 + 0.5) / 2^14 (its own rounding; for the one
    completed from the others their two roundings and that of the row's sum), times at most 4095
    that is 0.5 of a code over a row, and the final rounding adds its own."""
    rng_ = np.random.default_rng(mtrx * 100 + rng * 10 + d)
    rgb = rng_.integers(0, 1 << d, (3, 4096))
    rgb[:, :8] = np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)]).T * ((1 << d) - 1)
    for a, b in zip(Q.forward(rgb, mtrx, rng, d), Q.forward_float(rgb, mtrx, rng, d)):
        assert np.abs(a - b).max() <= 1


@pytest.mark.parametrize("layout,chr", SITINGS, ids=[f"layout{a}-chr{b}" for a, b in SITINGS])
def test_decimate_of_a_constant_is_the_constant(layout, chr):
    for h, w in ((1, 1), (1, 2), (2, 1), (7, 9), (9, 17), (4, 6)):
        for value in (0, 1, 513, 4095):
            out = Q.decimate(np.full((h, w), value), layout, chr)
            cw, ch = R.chroma_size(w, h, layout)
            assert out.shape == (ch, cw) and np.all(out == value)


@pytest.mark.parametrize("layout,chr", SITINGS, ids=[f"layout{a}-chr{b}" for a, b in SITINGS])
def test_decimate_clamps_its_indices(layout, chr):
    """1 x 1 and 1 x n planes: every tap beyond the plane reads the edge sample; checked against the
    sums written out by hand."""
    assert Q.decimate(np.array([[77]]), layout, chr).tolist() == [[77]]
    row = np.array([[10, 20, 40, 80, 160]])
    got = Q.decimate(row, layout, chr)
    if layout == 3:
        assert np.array_equal(got, row)
    else:
        # every row tap of 4:2:0 clamps to the one row, so both layouts give the horizontal filter
        want = [(10 + 2 * 10 + 20 + 2) >> 2, (20 + 2 * 40 + 80 + 2) >> 2, (80 + 2 * 160 + 160 + 2) >> 2]
        assert got.tolist() == [want]
    col = row.T
    got = Q.decimate(col, layout, chr)
    if layout != 1:
        assert np.array_equal(got, col)
    elif chr == 2:
        assert got[:, 0].tolist() == [(10 + 2 * 10 + 20 + 2) >> 2, (20 + 2 * 40 + 80 + 2) >> 2, (80 + 2 * 160 + 160 + 2) >> 2]
    else:
        assert got[:, 0].tolist() == [(10 + 20 + 1) >> 1, (40 + 80 + 1) >> 1, 160]


@pytest.mark.parametrize("layout,chr", SITINGS, ids=[f"layout{a}-chr{b}" for a, b in SITINGS])
def test_decimate_then_upsample_keeps_a_ramp(layout, chr):
    """A linear ramp in x and y, decimated and put back by display_ref's upsampler, is the ramp
    again in the interior to within a code: the taps sit where the upsampler assumes the samples."""
    h, w = 24, 32
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = 100 + 12 * xx + 20 * yy
    back = R.upsample(Q.decimate(ramp, layout, chr), layout, chr, w, h)
    assert back.shape == ramp.shape
    assert np.abs(back - ramp)[2:-2, 2:-2].max() <= 1
