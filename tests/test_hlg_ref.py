"""CPU, no device: tests/hlg_ref.py, the model of HLG sources in the colour-volume stage
(include/mi_av1out.h, "HLG sources"), against float64 and the anchors of BT.2100 / BT.2408: the
inverse OETF at its joint and its end, the system gamma, reference white, the luminance row, the
gain table against Y^(gamma - 1), and the float32 stage over the tables against the conversion in
float64.

The bounds are derived, not measured: 1e-4 relative for the gain is below half a 12-bit code step
(1 / 8190 = 1.2e-4), so the table cannot move a destination code by itself; 1 code end to end is
the bound tests/test_tonemap_tables.py holds the PQ stage to (output rounding 0.5, the 16-bit index
at most 0.40, the gain 0.41 of a 12-bit code at 1e-4, never all at their worst in one sample: the
gain's worst is at dst_peak 1, outside these cases)."""
import math

import numpy as np
import pytest

from tests import hlg_ref as H

PEAKS = [50.0, 100.0, 203.0, 1000.0, 4000.0, 10000.0]


def test_inverse_oetf_is_continuous_at_one_half():
    lo, hi = H.inv_oetf_branches(0.5)
    assert lo == 1.0 / 12.0
    assert abs(hi - 1.0 / 12.0) <= 1e-9          # (a, b, c as the standard rounds them)
    assert H.inv_oetf(0.5) == lo
    below, above = H.inv_oetf(0.5 - 1e-9), H.inv_oetf(0.5 + 1e-9)
    assert below < lo < above and above - below < 1e-8


def test_inverse_oetf_reaches_exactly_one():
    _, hi = H.inv_oetf_branches(1.0)
    assert 1.0 < hi < 1.0 + 1e-7, "the formula alone overshoots: the min is needed"
    assert H.inv_oetf(1.0) == 1.0
    assert H.inv_oetf(0.0) == 0.0
    x = np.linspace(0.0, 1.0, 4097)
    e = H.inv_oetf_f64(x)
    assert np.all(np.diff(e) > 0) and e[0] == 0.0 and e[-1] == 1.0
    # (the array form and the scalar form evaluate exp in different libraries: a few ulps of float64)
    assert np.all(np.abs(e - np.array([H.inv_oetf(float(v)) for v in x])) <= 4 * np.spacing(e))


def test_system_gamma():
    assert H.gamma(1000.0) == 1.2
    for lw in (400.0, 600.0, 1000.0, 1500.0, 2000.0):
        assert abs(H.gamma(lw) - (1.2 + 0.42 * math.log10(lw / 1000.0))) <= 0.03, lw
    assert H.gamma(100.0) < 1.0 < H.gamma(400.0)
    assert abs(H.gamma(100.0) - 0.846) < 1e-3


def test_reference_white():
    """A grey signal of 0.75 on a 1000-nit display: BT.2408's HDR reference white, 203 nits."""
    e = H.inv_oetf(0.75)
    nits = 1000.0 * e * math.pow(e, H.gamma(1000.0) - 1.0)      # grey: Y = E
    assert abs(nits - 203.0) <= 2.03, nits


def test_luminance_row_of_bt2020():
    yw = H.luminance_row(9)
    assert yw.dtype == np.float32
    assert np.all(np.abs(yw.astype(np.float64) - np.array([0.2627, 0.6780, 0.0593])) <= 1e-4)
    for pri in (1, 5, 6, 7, 9, 12):
        assert abs(float(H.luminance_row(pri).astype(np.float64).sum()) - 1.0) <= 2.0 ** -22, pri


def test_nodes():
    y = H.nodes()
    assert y.shape == (H.NODES,) and y[0] == np.float32(2.0 ** -24) and y[1536] == 1.0 and y[1537] == 1.0
    assert np.all(np.diff(y[:1537]) > 0)
    assert np.array_equal(y[0:1537:64], np.float32(2.0) ** np.arange(-24, 1, dtype=np.float32))      # 64 per octave


@pytest.mark.parametrize("dst_peak", PEAKS)
def test_gain_table_against_float64(dst_peak):
    lut = H.table_gain(dst_peak)
    assert lut.dtype == np.float32 and lut.shape == (H.NODES,)
    assert lut[1536] == 1.0 and lut[1537] == 1.0
    rng = np.random.default_rng(int(dst_peak))
    y = np.exp2(rng.uniform(-24.0, 0.0, 200000)).astype(np.float32)
    y = np.concatenate([y, H.nodes(), np.float32([2.0 ** -24, 1.0])])
    want = np.power(y.astype(np.float64), H.gamma(dst_peak) - 1.0)
    err = np.abs(H.gain(y, lut).astype(np.float64) / want - 1.0)
    print("dst_peak", dst_peak, "worst relative error of the gain", float(err.max()))
    assert err.max() <= 1e-4


def test_gain_indexes_inside_the_table_at_the_ends():
    lut = H.table_gain(100.0)
    ends = np.float32([0.0, 1e-30, 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 1.0000119, 1.5])
    g = H.gain(ends, lut)      # (asserts the index range itself)
    assert g[0] == lut[0] and g[1] == lut[0] and g[2] == lut[0]
    assert np.all(g[3:] == 1.0)


@pytest.mark.parametrize("dst_peak", [100.0, 1000.0])
@pytest.mark.parametrize("dst_bpc", [8, 10, 12])
@pytest.mark.parametrize("src_bpc", [8, 10, 12])
def test_float32_stage_against_float64(src_bpc, dst_bpc, dst_peak):
    """BT.2020 -> BT.709 / sRGB, and BT.2020 kept (identity m) under the BT.709 OETF."""
    rng = np.random.default_rng(src_bpc * 100 + dst_bpc + int(dst_peak))
    ms = (1 << src_bpc) - 1
    rgb = rng.integers(0, ms + 1, (3, 64, 64))
    rgb[:, 0, :8] = np.array([0, ms, ms // 2, 1, ms - 1, 0, ms, 0])     # the extremes, and
    rgb[1, 0, 5:8] = ms                                                  # saturated pairs
    rgb[2, 0, 7] = ms
    for dst_pri, dst_trc in ((1, 13), (9, 1)):
        got = H.apply(rgb, *H.tables(9, src_bpc, dst_pri, dst_trc, dst_bpc, dst_peak))
        want = H.apply_f64(rgb, src_bpc, 9, dst_pri, dst_trc, dst_bpc, dst_peak)
        assert got.min() >= 0 and got.max() <= (1 << dst_bpc) - 1
        diff = np.abs(got - want)
        print(src_bpc, dst_bpc, dst_peak, dst_pri, "codes that differ", int((diff > 0).sum()), "worst", int(diff.max()))
        assert diff.max() <= 1
