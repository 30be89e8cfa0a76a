"""GPU: resample= of decode_to_batches and decode_to_ladder (rav1d_amd/stream.py) on the smallest
8-bit 4:2:0 stream: every picture equals tests/cubic_ref.py's model of the reference picture."""
import numpy as np
import pytest
import torch

from rav1d_amd.display import Resample, even_crop
from rav1d_amd.stream import decode_to_batches, decode_to_ladder, fit_crop
from tests import cubic_ref as C
from tests import tensor_ref as T
from tests.stream_lib import planar_pictures, stream
from tests.test_scaled_streams_gpu import host, one_to_one_pictures
from tests.test_tensor_streams_gpu import MEAN, STD

pytestmark = pytest.mark.gpu

NAME = "av1-1-b8-01-size-18x16"


def test_batches_with_catmull_rom(gpu):
    """An upscale and a downscale with fit="crop", float16, mean / std."""
    _, data = stream(NAME)
    pictures = planar_pictures(gpu, NAME)
    for size in ((24, 20), (7, 5)):
        W, H = size
        n = 0
        for tensor, colors in decode_to_batches(gpu, data, size=size, batch=4, mean=MEAN, std=STD, fit="crop",
                                                resample=Resample("catmull_rom")):
            torch.cuda.synchronize()
            slots = tensor.view(torch.int16).cpu().numpy().view(np.uint16)
            for slot, color in zip(slots, colors):
                planes, bpc, layout = pictures[n]
                h, w = planes[0].shape
                scale, bias = T.scale_bias(bpc, MEAN, STD)
                want = C.tensor(planes, bpc, layout, (color.mtrx, color.range, color.chr), fit_crop(w, h, W, H, "crop"),
                                size, T.F16, scale, bias, 0.0, 0.5)
                assert np.array_equal(slot, want.view(np.uint16)), (size, n)
                n += 1
        assert n == len(pictures) > 0


def test_ladder_with_mitchell(gpu):
    """Two rungs per picture, one smaller and one larger than the stream."""
    _, data = stream(NAME)
    want = one_to_one_pictures(gpu, NAME)
    sizes = [(10, 8), (30, 22)]
    got = [rungs for _, rungs in decode_to_ladder(gpu, data, sizes, fit="crop", resample=Resample("mitchell"))]
    torch.cuda.synchronize()
    assert len(got) == len(want) > 0
    for rungs, (planes, bpc, layout, chr) in zip(got, want):
        h, w = planes[0].shape
        for (W, H), (y, uv) in zip(sizes, rungs):
            crop = even_crop(fit_crop(w, h, W, H, "crop"), w, h, layout)
            my, muv = C.scaled(planes, bpc, layout, chr, (W, H), bpc, crop, 1.0 / 3.0, 1.0 / 3.0)
            assert np.array_equal(host(y, bpc), my) and np.array_equal(host(uv, bpc), muv)
