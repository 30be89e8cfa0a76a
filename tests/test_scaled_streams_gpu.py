"""GPU: whole streams through decode_to_ladder (rav1d_amd/stream.py): every shown picture's rungs
equal tests/scaled_ref.py applied to the pictures the same stream gives through the existing 1:1
path (decode_to_tensors, semi-planar), in the same number and order."""
import numpy as np
import pytest
import torch

from rav1d_amd.display import even_crop
from rav1d_amd.stream import decode_to_ladder, decode_to_tensors, fit_crop
from tests import scaled_ref as Z
from tests.stream_lib import stream

pytestmark = pytest.mark.gpu

_pictures = {}


def one_to_one_pictures(gpu, name):
    """The planar pictures of a vector from the semi-planar 1:1 path (host copies, LSB-aligned),
    with each picture's colour description; computed once and shared."""
    if name not in _pictures:
        v, data = stream(name)
        out = []
        for image, color in decode_to_tensors(gpu, data, format="nv12", apply_grain=bool(v.get("filmgrain"))):
            torch.cuda.synchronize()
            sh = 16 - image.bpc if image.bpc > 8 else 0
            host = image.numpy()
            planes = [host[0] >> sh] + ([host[1][..., c] >> sh for c in (0, 1)] if image.layout else [])
            out.append((planes, image.bpc, image.layout, color.chr))
        _pictures[name] = out
    return _pictures[name]


def host(t, bpc):
    a = t.cpu().numpy()
    return a.view("<u2") if bpc > 8 else a


def check_ladder(gpu, name, sizes, bpc, fit):
    v, data = stream(name)
    want = one_to_one_pictures(gpu, name)
    got = []
    for ev, rungs in decode_to_ladder(gpu, data, sizes, bpc=bpc, fit=fit, apply_grain=bool(v.get("filmgrain"))):
        assert ev.show_pic >= 0 and len(rungs) == len(sizes)
        got.append(rungs)
    torch.cuda.synchronize()
    assert len(got) == len(want) > 0
    for rungs, (planes, sbpc, layout, chr) in zip(got, want):
        h, w = planes[0].shape
        obpc = sbpc if bpc is None else bpc
        for (W, H), (y, uv) in zip(sizes, rungs):
            crop = even_crop(fit_crop(w, h, W, H, fit), w, h, layout)
            my, muv = Z.scaled(planes, sbpc, layout, chr, (W, H), obpc, crop)
            assert y.is_cuda and tuple(y.shape) == (H, W) and y.dtype == (torch.uint8 if obpc == 8 else torch.int16)
            assert np.array_equal(host(y, obpc), my)
            if layout:
                assert tuple(uv.shape) == muv.shape and np.array_equal(host(uv, obpc), muv)
            else:
                assert uv is None


def test_film_grain_420_10bit(gpu):
    """352 x 288 10-bit 4:2:0 with film grain on every picture: two rungs at 8 bits (the ladder's
    usual 10 -> 8), stretched; the grain is the 1:1 path's."""
    check_ladder(gpu, "av1-1-b10-23-film_grain-50", [(176, 144), (64, 36)], 8, "stretch")


def test_444_10bit_keeps_the_depth(gpu):
    """160 x 90 10-bit 4:4:4, bpc=None: the stream's depth; fit="crop" to a squarer and a larger rung."""
    check_ladder(gpu, "00000943_10bit", [(40, 40), (200, 100)], None, "crop")


def test_odd_width_grain_crop(gpu):
    """179 x 120 8-bit 4:2:0 with film grain: fit="crop" gives crops the chroma grid moves."""
    check_ladder(gpu, "309_odd_width", [(32, 32), (90, 60)], 10, "crop")
