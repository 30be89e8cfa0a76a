"""GPU: whole streams through decode_to_tensors (rav1d_amd/stream.py). The semi-planar tensors,
de-interleaved on the host and fed to the product md5 muxer, give the reference's MD5 of the
vector; the RGB tensors equal tests/display_ref.py applied to the planar pictures
decode_to_muxer writes for the same stream."""
import numpy as np
import pytest
import torch

from rav1d_amd.output import Muxer, host_picture_np
from rav1d_amd.stream import decode_to_tensors
from tests import display_ref as R
from tests.stream_lib import planar_pictures, stream

pytestmark = pytest.mark.gpu

# 8-bit 4:2:0, 10-bit 4:2:0, 10-bit 4:4:4, 8-bit monochrome, film grain (8-bit 4:2:0, odd width)
NAMES = ["av1-1-b8-01-size-18x16", "av1-1-b10-00-quantizer-63", "00000943_10bit", "00001105", "309_odd_width"]


@pytest.mark.parametrize("name", NAMES)
def test_nv12_tensors_give_the_reference_md5(gpu, name):
    v, data = stream(name)
    m = Muxer("md5")
    n = 0
    for image, color in decode_to_tensors(gpu, data, format="nv12", apply_grain=bool(v.get("filmgrain"))):
        torch.cuda.synchronize()
        sh = 16 - image.bpc if image.bpc > 8 else 0
        host = image.numpy()
        planes = [np.ascontiguousarray(host[0] >> sh)]
        if image.layout:
            planes += [np.ascontiguousarray(host[1][..., c] >> sh) for c in (0, 1)]
            assert host[1].shape == (image.ch, image.cw, 2)
        else:
            assert len(host) == 1
        m.write(host_picture_np(planes, image.w, image.h, image.bpc, image.layout))
        assert color.astuple() == (2, 2, 2, 0, 0)      # these vectors carry no colour description
        n += 1
    assert n > 0
    assert m.verify(v["md5"]) == 0, f"{name}: {m.digest()} != {v['md5']}"
    m.close()


@pytest.mark.parametrize("name", NAMES)
def test_rgb_tensors_match_the_planar_pictures(gpu, name):
    v, data = stream(name)
    want = planar_pictures(gpu, name)
    got = []
    for image, color in decode_to_tensors(gpu, data, format="rgb", apply_grain=bool(v.get("filmgrain"))):
        torch.cuda.synchronize()
        # mtrx 2 in the stream: BT.709 from 1280 wide or above 576 high, else BT.601
        assert color.mtrx == (1 if image.w >= 1280 or image.h > 576 else 6)
        got.append((image.numpy()[0], color))
    assert len(got) == len(want)
    for (rgb, color), (planes, bpc, layout) in zip(got, want):
        assert np.array_equal(rgb, R.to_rgb(planes, bpc, layout, color.mtrx, color.range, color.chr))


def test_explicit_matrix_and_rgba(gpu):
    """matrix= overrides the stream's; "rgba" is the packed form of the same conversion."""
    name = NAMES[0]
    v, data = stream(name)
    want = planar_pictures(gpu, name)
    n = 0
    for (image, color), (planes, bpc, layout) in zip(decode_to_tensors(gpu, data, format="rgba", matrix=9), want):
        torch.cuda.synchronize()
        assert color.mtrx == 9
        assert np.array_equal(image.numpy()[0], R.to_rgba(planes, bpc, layout, 9, color.range, color.chr))
        n += 1
    assert n == len(want)
