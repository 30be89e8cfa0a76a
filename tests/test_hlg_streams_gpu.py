"""GPU: decode_to_tensors and decode_to_ladder with a tone map on an HLG source (rav1d_amd.stream):
every shown picture of a 10-bit stream, declared BT.2020 HLG by the overrides, on a context of this
module's own that has opted in (rav1d_amd.display.enable_hlg; the helpers never do), equals
tests/hlg_ref.py's model over the planar pictures decode_to_muxer writes; peak= modes stay refused
for HLG, and the session's shared context keeps refusing the source."""
import numpy as np
import pytest
import torch

from rav1d_amd import MiError
from rav1d_amd.display import ToneMap, YuvTarget, enable_hlg, even_crop
from rav1d_amd.frame import Context
from rav1d_amd.stream import decode_to_batches, decode_to_ladder, decode_to_tensors, fit_crop
from tests import display_ref as R
from tests import hlg_ref as H
from tests import scaled_ref as Z
from tests import yuv_tm_ref as Q
from tests.stream_lib import planar_pictures, stream

pytestmark = pytest.mark.gpu

NAME = "av1-1-b10-00-quantizer-63"
HLG = dict(primaries=9, transfer=18, matrix=9)


@pytest.fixture(scope="module")
def hlg(gpu):
    ctx = Context(0)
    enable_hlg(ctx)
    yield ctx
    ctx.close()


def tensors_match_the_model(gpu, hlg):
    _, data = stream(NAME)
    pictures = planar_pictures(gpu, NAME)
    tm = ToneMap(dst_peak=203.0, src_peak=float("nan"))
    tables = H.tables(9, 10, 1, 13, 8, 203.0)
    n = 0
    for image, color in decode_to_tensors(hlg, data, format="rgba", tonemap=tm, **HLG):
        torch.cuda.synchronize()
        planes, bpc, layout = pictures[n]
        h, w = planes[0].shape
        assert bpc == 10 and (color.pri, color.trc, color.mtrx) == (9, 18, 9)
        assert image.bpc == 8 and image.rgba.dtype == torch.uint8 and image.rgba.shape == (h, w, 4)
        rgb = R.to_rgb(planes, bpc, layout, 9, color.range, color.chr)
        assert np.array_equal(image.numpy()[0], H.apply_rgba(rgb, *tables, 8)), n
        n += 1
    assert n == len(pictures)


def one_rung_matches_the_model(gpu, hlg):
    _, data = stream(NAME)
    pictures = planar_pictures(gpu, NAME)
    tm, size = ToneMap(dst_peak=100.0), (40, 24)
    tables = H.tables(9, 10, 1, 13, 8, 100.0)
    got = []
    for ev, rungs in decode_to_ladder(hlg, data, [size], bpc=8, tonemap=tm, target=YuvTarget(1, 0), **HLG):
        got.append((ev.color.range, ev.color.chr, rungs[0]))
    torch.cuda.synchronize()
    assert len(got) == len(pictures) > 0
    for (full, chr, (y, uv)), (planes, bpc, layout) in zip(got, pictures):
        h, w = planes[0].shape
        rgb = H.apply(R.to_rgb(planes, bpc, layout, 9, full, chr), *tables)
        yq, u4, v4 = Q.forward(rgb, 1, 0, 8)
        q = [yq, Q.decimate(u4, layout, chr), Q.decimate(v4, layout, chr)]
        crop = even_crop(fit_crop(w, h, size[0], size[1], "stretch"), w, h, layout)
        my, muv = Z.scaled(q, 8, layout, chr, size, 8, crop)
        assert np.array_equal(y.cpu().numpy(), my) and np.array_equal(uv.cpu().numpy(), muv)


def test_every_picture_matches_the_model(gpu, hlg):
    """decode_to_tensors(format="rgba") and one rung of decode_to_ladder."""
    tensors_match_the_model(gpu, hlg)
    one_rung_matches_the_model(gpu, hlg)


def test_refusals(gpu, hlg):
    """peak= modes choose src_peak, which an HLG source does not read: a ValueError; and the helpers
    never opt in: the shared context refuses the source."""
    _, data = stream(NAME)
    for peak in ("metadata", "measured"):
        with pytest.raises(ValueError):
            next(decode_to_tensors(hlg, data, format="rgba", tonemap=ToneMap(), peak=peak, **HLG))
        with pytest.raises(ValueError):
            next(decode_to_batches(hlg, data, size=(8, 8), tonemap=ToneMap(), peak=peak, **HLG))
        with pytest.raises(ValueError):
            next(decode_to_ladder(hlg, data, [(16, 10)], bpc=8, tonemap=ToneMap(), peak=peak, **HLG))
    with pytest.raises(MiError):
        next(decode_to_tensors(gpu, data, format="rgba", tonemap=ToneMap(), **HLG))
    with pytest.raises(MiError):
        next(decode_to_ladder(gpu, data, [(16, 10)], bpc=8, tonemap=ToneMap(), **HLG))
