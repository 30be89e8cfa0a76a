"""GPU: decode_to_ladder with a tone map (rav1d_amd.stream): every shown picture of a 10-bit stream,
declared HDR10 by the overrides, gives the rungs of tests/scaled_ref.py run on tests/yuv_tm_ref.py's
picture Q over the planar pictures decode_to_muxer writes; without the overrides the untagged stream
is refused; without a tone map the rungs are display_scaled's, as before."""
import numpy as np
import pytest
import torch

from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import ScaledImage, ToneMap, YuvTarget, display_scaled, even_crop, tonemap_tables
from rav1d_amd.stream import decode_ivf, decode_to_ladder, fit_crop
from tests import scaled_ref as Z
from tests import yuv_tm_ref as Q
from tests.stream_lib import planar_pictures, stream

pytestmark = pytest.mark.gpu

NAME = "av1-1-b10-00-quantizer-63"
SIZES = [(40, 24), (16, 10)]


def host(t, bpc):
    a = t.cpu().numpy()
    return a.view("<u2") if bpc > 8 else a


def test_rungs_match_the_model(gpu):
    _, data = stream(NAME)
    pictures = planar_pictures(gpu, NAME)
    tm, target = ToneMap(), YuvTarget(1, 0)
    tables = tonemap_tables(tm, MiColorInfo(9, 16, 9, 0, 0), 10)
    got = []
    for ev, rungs in decode_to_ladder(gpu, data, SIZES, bpc=8, tonemap=tm, target=target, primaries=9, transfer=16, matrix=9):
        assert ev.show_pic >= 0 and len(rungs) == len(SIZES)
        got.append((ev.color.range, ev.color.chr, rungs))
    torch.cuda.synchronize()
    assert len(got) == len(pictures) > 0
    for (full, chr, rungs), (planes, bpc, layout) in zip(got, pictures):
        h, w = planes[0].shape
        assert bpc == 10 and layout == 1
        q = Q.picture_q(planes, bpc, layout, (9, full, chr), tables, (1, 0), 8)
        for (W, H), (y, uv) in zip(SIZES, rungs):
            crop = even_crop(fit_crop(w, h, W, H, "stretch"), w, h, layout)
            my, muv = Z.scaled(q, 8, layout, chr, (W, H), 8, crop)
            assert y.is_cuda and tuple(y.shape) == (H, W) and y.dtype == torch.uint8
            assert np.array_equal(host(y, 8), my)
            assert tuple(uv.shape) == muv.shape and np.array_equal(host(uv, 8), muv)


def test_depth_defaults_to_the_tone_maps(gpu):
    """bpc=None: tonemap.dst_bpc, not the stream's depth; target None: BT.709 limited."""
    _, data = stream(NAME)
    planes, bpc, layout = planar_pictures(gpu, NAME)[0]
    tm = ToneMap(dst_bpc=8)
    ev, rungs = next(decode_to_ladder(gpu, data, SIZES[:1], tonemap=tm, primaries=9, transfer=16, matrix=9))
    torch.cuda.synchronize()
    y, uv = rungs[0]
    assert y.dtype == torch.uint8 and uv.dtype == torch.uint8
    q = Q.picture_q(planes, bpc, layout, (9, ev.color.range, ev.color.chr), tonemap_tables(tm, MiColorInfo(9, 16, 9, 0, 0), 10),
                    (1, 0), 8)
    my, muv = Z.scaled(q, 8, layout, ev.color.chr, SIZES[0], 8)
    assert np.array_equal(host(y, 8), my) and np.array_equal(host(uv, 8), muv)


def test_untagged_stream_needs_the_overrides(gpu):
    _, data = stream(NAME)
    for kw in ({}, {"primaries": 9}, {"transfer": 16}):
        with pytest.raises(ValueError):
            next(decode_to_ladder(gpu, data, SIZES, bpc=8, tonemap=ToneMap(), matrix=9, **kw))


def test_without_a_tone_map_nothing_changes(gpu):
    """The rungs equal display_scaled called directly on the shown pictures; the overrides are not
    read."""
    _, data = stream(NAME)
    want = []
    for src in decode_ivf(gpu, data):
        images = [ScaledImage(W, H, 8, src.layout, even_crop(fit_crop(src.w, src.h, W, H, "stretch"), src.w, src.h, src.layout))
                  for W, H in SIZES]
        display_scaled(gpu, src, images, MiColorInfo(2, 2, 2, 0, 0))
        torch.cuda.synchronize()
        want.append([im.numpy() for im in images])
    got = []
    for ev, rungs in decode_to_ladder(gpu, data, SIZES, bpc=8, primaries=9, transfer=16):
        torch.cuda.synchronize()
        got.append([[host(t, 8) for t in rung] for rung in rungs])
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        for (gy, guv), (wy, wuv) in zip(g, w):
            assert np.array_equal(gy, wy) and np.array_equal(guv, wuv)
