"""GPU: whole streams through decode_to_batches (rav1d_amd/stream.py): every `every`-th shown
picture as a slot of a float16 batch, equal bit for bit to tests/tensor_ref.py applied to the
planar pictures decode_to_muxer writes for the same stream, for both `fit` values."""
import numpy as np
import pytest
import torch

from rav1d_amd.stream import decode_to_batches, fit_crop
from tests import tensor_ref as T
from tests.stream_lib import planar_pictures, stream

pytestmark = pytest.mark.gpu

# 8-bit 4:2:0, 10-bit 4:2:0, film grain (8-bit 4:2:0, odd width)
NAMES = ["av1-1-b8-01-size-18x16", "av1-1-b10-00-quantizer-63", "309_odd_width"]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def check_batches(gpu, name, fit, size):
    v, data = stream(name)
    pictures = planar_pictures(gpu, name)[::2]
    (W, H), batch = size, 3
    got = []
    for tensor, colors in decode_to_batches(gpu, data, size=size, batch=batch, every=2, mean=MEAN, std=STD, fit=fit,
                                            apply_grain=bool(v.get("filmgrain"))):
        torch.cuda.synchronize()
        assert tensor.dtype == torch.float16 and tensor.is_cuda and tensor.shape[1:] == (3, H, W)
        assert tensor.shape[0] == len(colors)
        got.append((tensor, tensor.view(torch.int16).cpu().numpy().view(np.uint16), colors))
    # batch count, the short last batch, fresh allocations (the tensors are all still held)
    sizes = [len(c) for _, _, c in got]
    assert sum(sizes) == len(pictures)
    assert sizes == [batch] * (len(pictures) // batch) + ([len(pictures) % batch] if len(pictures) % batch else [])
    assert len({t.data_ptr() for t, _, _ in got}) == len(got)
    flat = [(h[i], c[i]) for _, h, c in got for i in range(len(c))]
    for (slot, color), (planes, bpc, layout) in zip(flat, pictures):
        h, w = planes[0].shape
        # these vectors carry no colour description: BT.709 from 1280 wide or above 576 high, else BT.601
        assert color.astuple() == (2, 2, 1 if w >= 1280 or h > 576 else 6, 0, 0)
        scale, bias = T.scale_bias(bpc, MEAN, STD)
        want = T.tensor(planes, bpc, layout, (color.mtrx, color.range, color.chr), fit_crop(w, h, W, H, fit), size,
                        T.F16, scale, bias)
        assert np.array_equal(slot, want.view(np.uint16))


@pytest.mark.parametrize("fit", ["stretch", "crop"])
@pytest.mark.parametrize("name", NAMES)
def test_batches_match_the_planar_pictures(gpu, name, fit):
    """size=(8, 8), batch=3, every=2. av1-1-b10-00-quantizer-63 is 640 x 360: stretched to 8 wide it
    is 80:1, above the 64:1 mi_display_tensor accepts, so that one case is the -EINVAL the header
    promises, and the vector's stretch is compared at (10, 8), exactly 64:1."""
    w = planar_pictures(gpu, name)[0][0][0].shape[1]
    if fit == "stretch" and w > 64 * 8:
        from rav1d_amd import MiError
        with pytest.raises(MiError, match="-22"):
            check_batches(gpu, name, fit, (8, 8))
        check_batches(gpu, name, fit, (10, 8))
    else:
        check_batches(gpu, name, fit, (8, 8))


def test_channels_last_uint8_and_every_picture(gpu):
    """channels_last batches of uint8, every picture, an explicit matrix."""
    name = NAMES[0]
    _, data = stream(name)
    pictures = planar_pictures(gpu, name)
    n = 0
    for tensor, colors in decode_to_batches(gpu, data, size=(12, 5), batch=4, dtype=torch.uint8, channels_last=True,
                                            matrix=9):
        torch.cuda.synchronize()
        assert tensor.is_contiguous(memory_format=torch.channels_last) or tensor.shape[0] < 4
        host = tensor.cpu().numpy()
        for i, color in enumerate(colors):
            planes, bpc, layout = pictures[n]
            assert color.mtrx == 9
            assert np.array_equal(host[i], T.tensor(planes, bpc, layout, (9, color.range, color.chr), None, (12, 5), T.U8))
            n += 1
    assert n == len(pictures)
