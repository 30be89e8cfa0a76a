"""GPU: the peak= modes of rav1d_amd.stream's helpers. With peak="measured" every shown picture is
mapped with the src_peak a CPU model gives (tests/display_ref.py's histogram, the numpy statistics of
tests/test_light_stats.py, PeakTracker); with peak="metadata" with the stream's mastering display;
with peak=None with the tone map's own. Each equals, bit for bit, the output call made directly with
that src_peak."""
import numpy as np
import pytest
import torch

from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (DisplayImage, ScaledImage, ToneMap, display_picture, display_scaled, display_tensor,
                               even_crop)
from rav1d_amd.stream import (PeakTracker, decode_to_batches, decode_to_ladder, decode_to_tensors, metadata_peak,
                              shown_pictures)
from tests import display_ref as R
from tests.stream_lib import planar_pictures, stream
from tests.test_light_stats import model as stats_model

pytestmark = pytest.mark.gpu

NAME = "av1-1-b10-00-quantizer-63"       # 640 x 360, 10 bits, untagged: declared HDR10 by the overrides
HDR = "itut_t35_10bit"                   # one 3840 x 2160 picture, tagged PQ / BT.2020, with MDCV and CLL
OVERRIDES = dict(primaries=9, transfer=16, matrix=9)
SIZES = [(320, 180), (96, 54)]


def with_peak(tm, peak):
    return ToneMap(tm.dst_pri, tm.dst_trc, tm.dst_bpc, peak, tm.dst_peak)


_peaks = {}


def model_peaks(gpu, tm):
    """The src_peak of every shown picture of NAME under peak="measured", from the CPU model."""
    key = float(tm.dst_peak)
    if key not in _peaks:
        tracker, out = PeakTracker(tm.dst_peak), []
        for planes, bpc, layout in planar_pictures(gpu, NAME):
            hist = np.bincount(R.to_rgb(planes, bpc, layout, 9, 0, 0).max(axis=0).ravel(), minlength=1 << bpc)
            out.append(min(max(tracker.update(stats_model(hist, bpc, 99.99)[3]), float(tm.dst_peak)), 10000.0))
        _peaks[key] = out
    return _peaks[key]


def ladder_direct(gpu, data, tm, peaks):
    """display_scaled per shown picture with the peaks given (None: the tone map's own)."""
    out = []
    for k, (ev, src) in enumerate(shown_pictures(gpu, data)):
        color = MiColorInfo(9, 16, 9, ev.color.range, ev.color.chr)
        images = [ScaledImage(W, H, tm.dst_bpc, src.layout, even_crop((0, 0, src.w, src.h), src.w, src.h, src.layout))
                  for W, H in SIZES]
        display_scaled(gpu, src, images, color, tonemap=tm if peaks is None else with_peak(tm, peaks[k]))
        torch.cuda.synchronize()
        out.append([[t.cpu().numpy() for t in im.tensors()] for im in images])
    return out


def ladder(gpu, data, tm, **kw):
    out = []
    for _, rungs in decode_to_ladder(gpu, data, SIZES, tonemap=tm, **OVERRIDES, **kw):
        torch.cuda.synchronize()
        out.append([[t.cpu().numpy() for t in pair] for pair in rungs])
    return out


def same(a, b):
    assert len(a) == len(b) > 0
    for pa, pb in zip(a, b):
        for ra, rb in zip(pa, pb):
            for ta, tb in zip(ra, rb):
                assert np.array_equal(ta, tb)


def test_ladder_measured(gpu):
    _, data = stream(NAME)
    tm = ToneMap(dst_bpc=8, src_peak=1000.0)
    peaks = model_peaks(gpu, tm)
    assert all(p % 100 == 0 and 100 <= p <= 10000 for p in peaks) and any(p != 1000.0 for p in peaks)
    got = ladder(gpu, data, tm, peak="measured")
    same(got, ladder_direct(gpu, data, tm, peaks))
    assert tm.src_peak == 1000.0                     # the caller's tone map is not modified


def test_ladder_none_is_todays_output(gpu):
    _, data = stream(NAME)
    tm = ToneMap(dst_bpc=10, dst_trc=1, src_peak=1000.0)
    want = ladder_direct(gpu, data, tm, None)
    same(ladder(gpu, data, tm), want)
    same(ladder(gpu, data, tm, peak=None), want)


def test_ladder_metadata(gpu):
    _, data = stream(HDR)
    tm = ToneMap(dst_bpc=8, src_peak=1000.0)
    evs = [(ev.mastering_display.present, ev.mastering_display.max_luminance, ev.content_light.present,
            ev.content_light.max_cll, metadata_peak(ev, tm)) for ev, _ in shown_pictures(gpu, data)]
    assert evs and all(e[0] and e[1] > 0 and e[4] == e[1] / 256.0 for e in evs)
    peaks = [min(max(e[4], 100.0), 10000.0) for e in evs]
    got = []
    for _, rungs in decode_to_ladder(gpu, data, SIZES, tonemap=tm, peak="metadata"):
        torch.cuda.synchronize()
        got.append([[t.cpu().numpy() for t in pair] for pair in rungs])
    want = []
    for k, (ev, src) in enumerate(shown_pictures(gpu, data)):
        images = [ScaledImage(W, H, 8, src.layout, even_crop((0, 0, src.w, src.h), src.w, src.h, src.layout))
                  for W, H in SIZES]
        display_scaled(gpu, src, images, MiColorInfo(*ev.color.astuple()), tonemap=with_peak(tm, peaks[k]))
        torch.cuda.synchronize()
        want.append([[t.cpu().numpy() for t in im.tensors()] for im in images])
    same(got, want)
    # and it differs from the default peak's output: the metadata was used
    assert any(not np.array_equal(a[0][0], b[0][0]) for a, b in zip(got, ladder_direct_plain(gpu, data, tm)))


def ladder_direct_plain(gpu, data, tm):
    out = []
    for _, rungs in decode_to_ladder(gpu, data, SIZES, tonemap=tm):
        torch.cuda.synchronize()
        out.append([[t.cpu().numpy() for t in pair] for pair in rungs])
    return out


def test_peak_needs_a_pq_source(gpu):
    _, data = stream(NAME)
    for mode in ("metadata", "measured"):
        with pytest.raises(ValueError):
            next(decode_to_ladder(gpu, data, SIZES, tonemap=ToneMap(), primaries=9, transfer=1, matrix=9, peak=mode))
        with pytest.raises(ValueError):
            next(decode_to_ladder(gpu, data, SIZES, peak=mode))


def test_tensors_measured(gpu):
    _, data = stream(NAME)
    tm = ToneMap(dst_bpc=8)
    peaks = model_peaks(gpu, tm)
    got = []
    for image, color in decode_to_tensors(gpu, data, format="rgb", tonemap=tm, peak="measured", **OVERRIDES):
        torch.cuda.synchronize()
        got.append(image.numpy()[0])
    want = []
    for k, (ev, src) in enumerate(shown_pictures(gpu, data)):
        image = DisplayImage(src.w, src.h, src.bpc, src.layout, "rgb", out_bpc=8)
        display_picture(gpu, src, image, MiColorInfo(9, 16, 9, ev.color.range, ev.color.chr), None, None,
                        with_peak(tm, peaks[k]))
        torch.cuda.synchronize()
        want.append(image.numpy()[0])
    assert len(got) == len(want) == len(peaks)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_batches_measured(gpu):
    _, data = stream(NAME)
    tm = ToneMap(dst_bpc=8)
    peaks = model_peaks(gpu, tm)
    got = []
    for tensor, colors in decode_to_batches(gpu, data, size=(64, 36), batch=2, dtype=torch.uint8, tonemap=tm,
                                            peak="measured", **OVERRIDES):
        torch.cuda.synchronize()
        got += [tensor[i].cpu().numpy() for i in range(len(colors))]
    want = []
    for k, (ev, src) in enumerate(shown_pictures(gpu, data)):
        out = torch.empty((3, 36, 64), dtype=torch.uint8, device="cuda")
        display_tensor(gpu, src, out, MiColorInfo(9, 16, 9, ev.color.range, ev.color.chr), tonemap=with_peak(tm, peaks[k]))
        torch.cuda.synchronize()
        want.append(out.cpu().numpy())
    assert len(got) == len(want) == len(peaks)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
