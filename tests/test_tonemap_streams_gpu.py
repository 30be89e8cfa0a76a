"""GPU: decode_to_tensors and decode_to_batches with a tone map (rav1d_amd.stream): every shown
picture of a 10-bit stream, declared HDR10 by the overrides, equals tests/tonemap_ref.py's model
over the planar pictures decode_to_muxer writes; without the overrides the untagged stream is
refused."""
import numpy as np
import pytest
import torch

from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import ToneMap, tonemap_tables
from rav1d_amd.stream import decode_to_batches, decode_to_tensors
from tests import display_ref as R
from tests import tensor_ref as T
from tests import tonemap_ref as TM
from tests.stream_lib import planar_pictures, stream

pytestmark = pytest.mark.gpu

NAME = "av1-1-b10-00-quantizer-63"


def test_tensors_match_the_model(gpu):
    _, data = stream(NAME)
    pictures = planar_pictures(gpu, NAME)
    tm = ToneMap()
    lut_in, m, lut_out = tonemap_tables(tm, MiColorInfo(9, 16, 9, 0, 0), 10)
    n = 0
    for image, color in decode_to_tensors(gpu, data, format="rgba", tonemap=tm, primaries=9, transfer=16, matrix=9):
        torch.cuda.synchronize()
        planes, bpc, layout = pictures[n]
        h, w = planes[0].shape
        assert bpc == 10 and (color.pri, color.trc, color.mtrx) == (9, 16, 9)
        assert image.bpc == 8 and image.rgba.dtype == torch.uint8 and image.rgba.shape == (h, w, 4)
        rgb = R.to_rgb(planes, bpc, layout, 9, color.range, color.chr)
        assert np.array_equal(image.numpy()[0], TM.apply_rgba(rgb, lut_in, m, lut_out, 8)), n
        n += 1
    assert n == len(pictures)


def test_untagged_stream_needs_the_overrides(gpu):
    _, data = stream(NAME)
    for kw in ({}, {"primaries": 9}, {"transfer": 16}):
        with pytest.raises(ValueError):
            next(decode_to_tensors(gpu, data, format="rgba", tonemap=ToneMap(), matrix=9, **kw))
        with pytest.raises(ValueError):
            next(decode_to_batches(gpu, data, size=(8, 8), tonemap=ToneMap(), matrix=9, **kw))


def test_batches_match_the_model(gpu):
    _, data = stream(NAME)
    pictures = planar_pictures(gpu, NAME)[::3]
    tm = ToneMap(dst_bpc=10, dst_trc=1)
    lut_in, m, lut_out = tonemap_tables(tm, MiColorInfo(9, 16, 9, 0, 0), 10)
    scale, bias = T.scale_bias(10)
    slots = []
    for tensor, colors in decode_to_batches(gpu, data, size=(40, 24), batch=2, every=3, tonemap=tm, primaries=9, transfer=16,
                                            matrix=9):
        torch.cuda.synchronize()
        host = tensor.view(torch.int16).cpu().numpy().view(np.uint16)
        slots += [(host[i], colors[i]) for i in range(len(colors))]
    assert len(slots) == len(pictures)
    for (slot, color), (planes, bpc, layout) in zip(slots, pictures):
        rgb = TM.apply(R.to_rgb(planes, bpc, layout, 9, color.range, color.chr), lut_in, m, lut_out)
        want = T.finish(T.resize(rgb, 40, 24), 10, T.F16, scale, bias)
        assert np.array_equal(slot, want.view(np.uint16))
