"""CPU, no device: mi_tonemap_tables (include/mi_av1out.h), the tables of the colour-volume stage,
against tests/tonemap_ref.py's independent float64 evaluation, their structure, the PQ tone curve's
end points, and the float32 stage over those tables against the conversion in float64.

The margins are derived, not measured: a double-precision evaluation is orders below a float32 ulp
(or an output code), so the library and the model can differ only where the one final rounding
falls on a boundary: 1 float32 ulp for lut_in, 2^-23 absolute for m (entries below 2: the ulp
there), 1 code for lut_out."""
import numpy as np
import pytest

from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import ToneMap, tonemap_tables
from tests import tonemap_ref as T

FLT_MIN = float(np.finfo(np.float32).tiny)
# (pri, trc) of the source: every accepted value of either appears
SOURCES = [(9, 16), (9, 14), (1, 1), (5, 6), (6, 6), (7, 13), (12, 13), (9, 15), (1, 16)]
# (dst_pri, dst_trc, dst_bpc): every accepted value of each appears
DESTS = [(1, 13, 8), (1, 1, 10), (9, 13, 12), (12, 1, 8), (9, 1, 12), (12, 13, 10)]


def tables(pri, trc, src_bpc, dst_pri=1, dst_trc=13, dst_bpc=8, src_peak=1000.0, dst_peak=100.0):
    return tonemap_tables(ToneMap(dst_pri, dst_trc, dst_bpc, src_peak, dst_peak), MiColorInfo(pri, trc, 1, 0, 0), src_bpc)


def ulp32(v):
    """The float32 ulp at the magnitude of float64 values v."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def assert_lut_in(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    # (the subnormal flush is not in play: no entry of these tables is that small)
    assert np.all((want == 0) | (want >= FLT_MIN))
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= ulp32(want)), float((err / ulp32(want)).max())


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: f"pri{s[0]}trc{s[1]}")
def test_tables_match_float64(src):
    pri, trc = src
    for src_bpc in (8, 10, 12):
        for dst_pri, dst_trc, dst_bpc in DESTS:
            for peaks in ((1000.0, 100.0), (4000.0, 203.0)) if trc == 16 else ((1000.0, 100.0),):
                lut_in, m, lut_out = tables(pri, trc, src_bpc, dst_pri, dst_trc, dst_bpc, *peaks)
                w_in, w_m, w_out = T.tables_f64(pri, trc, src_bpc, dst_pri, dst_trc, dst_bpc, *peaks)
                what = (pri, trc, src_bpc, dst_pri, dst_trc, dst_bpc, peaks)
                assert_lut_in(lut_in, w_in)
                assert m.dtype == np.float32 and np.all(np.abs(m.astype(np.float64) - w_m) <= 2.0 ** -23), what
                assert lut_out.dtype == np.uint16 and lut_out.shape == (65536,)
                assert np.all(np.abs(lut_out.astype(np.int64) - np.floor(w_out + 0.5).astype(np.int64)) <= 1), what


@pytest.mark.parametrize("src", SOURCES, ids=lambda s: f"pri{s[0]}trc{s[1]}")
def test_structure(src):
    pri, trc = src
    for src_bpc in (8, 10, 12):
        for dst_pri, dst_trc, dst_bpc in DESTS:
            lut_in, m, lut_out = tables(pri, trc, src_bpc, dst_pri, dst_trc, dst_bpc)
            md = (1 << dst_bpc) - 1
            assert lut_in.shape == (1 << src_bpc,) and lut_in[0] == 0.0
            assert np.all(np.diff(lut_in) >= 0) and lut_in.max() <= 1.0
            assert np.all((lut_in == 0) | (lut_in >= FLT_MIN)), "a subnormal entry"
            assert lut_out[0] == 0 and lut_out[65535] == md
            assert np.all(np.diff(lut_out.astype(np.int64)) >= 0)
            assert np.abs(m.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22
            if pri == dst_pri:
                assert np.array_equal(m, np.eye(3, dtype=np.float32))
            else:
                assert not np.array_equal(m, np.eye(3, dtype=np.float32))


@pytest.mark.parametrize("dst_trc", [1, 13])
@pytest.mark.parametrize("dst_bpc", [8, 10, 12])
def test_every_output_code_is_reachable(dst_trc, dst_bpc):
    """65536 entries: finer than the finest output step (12-bit sRGB's linear segment)."""
    _, _, lut_out = tables(1, 1, 8, 1, dst_trc, dst_bpc)
    assert np.array_equal(np.unique(lut_out), np.arange(1 << dst_bpc))


@pytest.mark.parametrize("src_bpc", [8, 10, 12])
def test_pq_without_compression_is_the_eotf(src_bpc):
    """dst_peak >= src_peak: maxLum = 1, KS = 1, the tone curve is the identity. Up to the code of
    src_peak the table is the plain EOTF over dst_peak; above it E1 is 1, the table src_peak over
    dst_peak (all of it when src_peak is the PQ maximum)."""
    x = np.arange(1 << src_bpc) / ((1 << src_bpc) - 1)
    for src_peak, dst_peak in ((10000.0, 10000.0), (1000.0, 1000.0), (1000.0, 4000.0)):
        lut_in, _, _ = tables(9, 16, src_bpc, src_peak=src_peak, dst_peak=dst_peak)
        ns = float(T.pq_inv_eotf(src_peak))
        want = np.where(x <= ns, T.pq_eotf(np.minimum(x, ns)), src_peak) / dst_peak
        want[0] = 0.0
        assert_lut_in(lut_in, want)


@pytest.mark.parametrize("src_bpc", [8, 10, 12])
def test_pq_peak_maps_to_one(src_bpc):
    """src_peak 1000 onto dst_peak 100: the code of 1000 nits and every code above it give the
    target peak, linear 1."""
    ms = (1 << src_bpc) - 1
    lut_in, _, _ = tables(9, 16, src_bpc, src_peak=1000.0, dst_peak=100.0)
    first = int(np.ceil(float(T.pq_inv_eotf(1000.0)) * ms))
    assert 0 < first < ms
    assert np.all(np.abs(lut_in[first:].astype(np.float64) - 1.0) <= float(np.spacing(np.float32(1.0))))
    assert lut_in[first // 2] < 0.5      # (the curve is not simply saturated)


@pytest.mark.parametrize("trc", [16, 14], ids=["pq", "curve709"])
@pytest.mark.parametrize("dst_trc", [1, 13])
@pytest.mark.parametrize("dst_bpc", [8, 10, 12])
@pytest.mark.parametrize("src_bpc", [8, 10, 12])
def test_float32_stage_against_float64(src_bpc, dst_bpc, dst_trc, trc):
    """BT.2020 -> BT.709. At most 1 output code: the output rounding gives 0.5, the 16-bit index
    at most 0.5 / 65535 x 12.92 x 4095 = 0.40 (the steepest OETF slope at the deepest output), the
    float32 arithmetic under 0.01."""
    rng = np.random.default_rng(src_bpc * 100 + dst_bpc * 10 + dst_trc + trc)
    ms = (1 << src_bpc) - 1
    rgb = rng.integers(0, ms + 1, (3, 64, 64))
    rgb[:, 0, :8] = np.array([0, ms, ms // 2, 1, ms - 1, 0, ms, 0])     # the extremes, and
    rgb[1, 0, 5:8] = ms                                                  # saturated pairs
    rgb[2, 0, 7] = ms
    lut_in, m, lut_out = tables(9, trc, src_bpc, 1, dst_trc, dst_bpc)
    got = T.apply(rgb, lut_in, m, lut_out)
    want = T.apply_f64(rgb, src_bpc, 9, trc, 1, dst_trc, dst_bpc)
    assert got.min() >= 0 and got.max() <= (1 << dst_bpc) - 1
    assert np.abs(got - want).max() <= 1
