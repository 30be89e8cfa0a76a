"""GPU: mi_display_tensor (include/mi_av1out.h, csrc/tensor.hip) against tests/tensor_ref.py, bit
for bit in every dtype (float32 too: the arithmetic is specified); nothing outside the 3 w h
elements of the destination is touched."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (T_BF16, T_F16, T_F32, T_U8, DisplayImage, MiTensorImage, display_picture, display_tensor,
                               tensor_image)
from rav1d_amd.frame import _stream_ptr
from rav1d_amd.synth import make_fg_params
from tests import display_ref as R
from tests import tensor_ref as T
from tests.test_display_gpu import grain_reference, make_planes
from tests.test_lr_gpu import to_frame

pytestmark = pytest.mark.gpu

FILL = 0xA5
EINVAL = -22
DTYPES = [T_U8, T_F16, T_BF16, T_F32]
ES = {T_U8: 1, T_F16: 2, T_BF16: 2, T_F32: 4}
BITS = {T_U8: np.uint8, T_F16: np.uint16, T_BF16: np.uint16, T_F32: np.uint32}
# a per-channel mean / std whose scale and bias are not exactly representable
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class Dest:
    """A 3 x h x w destination in one guarded device buffer filled with FILL. order: "chw", "hwc"
    or a tuple of three element strides (channel, row, column); pad: extra elements per row;
    offset: elements in front of element (0, 0, 0), on top of a 64-byte guard band."""

    def __init__(self, w, h, dtype, order="chw", pad=0, offset=0):
        self.w, self.h, self.dtype, self.es = w, h, dtype, ES[dtype]
        if order == "chw":
            strides = ((w + pad) * h, w + pad, 1)
        elif order == "hwc":
            strides = (1, 3 * w + pad, 3)
        else:
            strides = order
        self.strides = tuple(s * self.es for s in strides)
        self.first = 64 + offset * self.es
        last = 2 * self.strides[0] + (h - 1) * self.strides[1] + (w - 1) * self.strides[2]
        self.buf = torch.full((self.first + last + self.es + 96,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 64 == 0

    def image(self, bpc, crop=None, scale=None, bias=None):
        im = MiTensorImage()
        im.data = self.buf.data_ptr() + self.first
        for i in range(3):
            im.stride[i] = self.strides[i]
        im.w, im.h, im.dtype = self.w, self.h, self.dtype
        if crop is not None:
            im.crop_x, im.crop_y, im.crop_w, im.crop_h = crop
        for c in range(3):
            im.scale[c] = 1.0 if scale is None else float(scale[c])
            im.bias[c] = 0.0 if bias is None else float(bias[c])
        return im

    def elements(self):
        """The (3, h, w) stored bit patterns; asserts that every other byte still holds FILL."""
        host = self.buf.cpu().numpy()
        c, y, x = np.meshgrid(np.arange(3), np.arange(self.h), np.arange(self.w), indexing="ij")
        at = self.first + c * self.strides[0] + y * self.strides[1] + x * self.strides[2]
        byte = at[..., None] + np.arange(self.es)
        assert len(np.unique(byte)) == byte.size
        rest = np.ones(host.shape, dtype=bool)
        rest[byte.reshape(-1)] = False
        assert np.all(host[rest] == FILL), "bytes outside the 3 w h elements"
        return np.ascontiguousarray(host[byte]).view(BITS[self.dtype])[..., 0]

    def untouched(self):
        return bool(np.all(self.buf.cpu().numpy() == FILL))


def bits(a):
    """A model result as the bit patterns Dest.elements returns."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def call(ctx, src, im, color, fg=None):
    pic = src.picture()
    return lib().mi_display_tensor(ctx.h, ctypes.byref(pic), ctypes.byref(im), ctypes.byref(color),
                                   ctypes.byref(fg) if fg is not None else None, _stream_ptr(None))


def model(rgb, bpc, size, dtype, crop=None, scale=None, bias=None):
    if crop is not None:
        x, y, w, h = crop
        rgb = rgb[:, y:y + h, x:x + w]
    return bits(T.finish(T.resize(rgb, size[0], size[1]), bpc, dtype, scale or (1.0, 1.0, 1.0), bias or (0.0, 0.0, 0.0)))


def run(ctx, src, rgb, bpc, color, size, dtype, order="chw", crop=None, norm=False, pad=0, offset=0, fg=None):
    """One call into a guarded destination, compared with the model of the R'G'B' picture `rgb`."""
    scale, bias = T.scale_bias(bpc, MEAN, STD) if norm else T.scale_bias(bpc)
    d = Dest(size[0], size[1], dtype, order, pad, offset)
    assert call(ctx, src, d.image(bpc, crop, scale, bias), color, fg) == 0
    torch.cuda.synchronize()
    want = model(rgb, bpc, size, dtype, crop, scale, bias)
    got = d.elements()
    assert np.array_equal(got, want), (size, dtype, order, crop, norm, pad, offset,
                                       int(np.count_nonzero(got != want)), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("size", [(17, 9), (65, 33), (136, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_to_one_is_the_rgb_picture(gpu, size):
    """No crop, no resize, uint8 at 8 bpc, CHW: mi_display_picture's planar R'G'B', and the model."""
    w, h = size
    for layout in range(4):
        rng = np.random.default_rng(w + layout)
        planes = make_planes(rng, w, h, 8, layout, "random")
        src = to_frame(planes, w, h, 8, layout)
        color = MiColorInfo(1, 1, 6, 0, 0)
        image = DisplayImage(w, h, 8, layout, "rgb")
        display_picture(gpu, src, image, color)
        d = Dest(w, h, T_U8)
        assert call(gpu, src, d.image(8), color) == 0
        torch.cuda.synchronize()
        got = d.elements()
        assert np.array_equal(got, image.numpy()[0]), layout
        assert np.array_equal(got, R.to_rgb(planes, 8, layout, 6, 0, 0)), layout


OUTPUTS = [(10, 6), (1, 1), (64, 33)]
# (mtrx, full range, chr): chr 0 and 2, limited and full range
COLORS = [(1, 0, 0), (6, 1, 2), (9, 0, 2), (1, 1, 0)]


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("size", [(67, 35), (136, 70), (1100, 6), (512, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_resampling(gpu, size, bpc):
    """Non-integer ratios both ways, upscaling, a single output, the 64:1 extreme (512 x 8 ->
    8 x 8); random data and the 0 / M / H block pattern; dtype and order rotate over the cases.
    A pair above 64:1 is -EINVAL with a live context too, and writes nothing."""
    w, h = size
    n = 0
    for layout in range(4):
        rng = np.random.default_rng(w * 100 + layout * 10 + bpc)
        sources = {}
        for kind in ("random", "blocks"):
            planes = make_planes(rng, w, h, bpc, layout, kind)
            sources[kind] = (planes, to_frame(planes, w, h, bpc, layout))
        for ci, (mtrx, full, chr) in enumerate(COLORS):
            planes, src = sources["random" if (ci + layout) % 2 == 0 else "blocks"]
            rgb = R.to_rgb(planes, bpc, layout, mtrx, full, chr)
            color = MiColorInfo(1, 1, mtrx, full, chr)
            for out in ([(8, 8)] if size == (512, 8) else OUTPUTS):
                dtype, order = DTYPES[n % 4], ("chw", "hwc")[(n // 4) % 2]
                n += 1
                if w > 64 * out[0] or h > 64 * out[1]:
                    d = Dest(out[0], out[1], dtype, order)
                    assert call(gpu, src, d.image(bpc), color) == EINVAL
                    torch.cuda.synchronize()
                    assert d.untouched()
                else:
                    run(gpu, src, rgb, bpc, color, out, dtype, order, norm=bool(n % 3))


@pytest.mark.parametrize("src_size,out", [((1100, 6), (1500, 4)), ((2500, 4), (40, 2)), ((2500, 4), (1030, 7))],
                         ids=["upscale", "downscale", "mixed"])
def test_rows_wider_than_a_segment(gpu, src_size, out):
    """The horizontal pass splits a row's outputs into workgroup segments: at most 1024 outputs,
    and no more than reach 2048 source columns (2500 -> 40 takes 31 per segment)."""
    w, h = src_size
    for layout, bpc, dtype in ((1, 8, T_U8), (3, 10, T_F16), (2, 12, T_F32), (0, 10, T_BF16)):
        rng = np.random.default_rng(w + layout)
        planes = make_planes(rng, w, h, bpc, layout, "random")
        rgb = R.to_rgb(planes, bpc, layout, 1, 0, 0)
        src = to_frame(planes, w, h, bpc, layout)
        run(gpu, src, rgb, bpc, MiColorInfo(1, 1, 1, 0, 0), out, dtype, "chw")
        run(gpu, src, rgb, bpc, MiColorInfo(1, 1, 1, 0, 0), out, dtype, "hwc", crop=(37, 1, w - 50, h - 1))


@pytest.mark.parametrize("layout", [1, 2, 3, 0])
def test_crops(gpu, layout):
    """Odd origin and odd size (4:2:0: the chroma is upsampled over the whole picture, so the crop
    changes no sample), a crop touching the right and bottom edges, 1 x 1 crops; outputs smaller,
    equal, larger and a single element."""
    w, h, bpc = 67, 35, 10
    rng = np.random.default_rng(layout)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    n = 0
    for chr in (0, 2):
        color = MiColorInfo(1, 1, 1, 0, chr)
        rgb = R.to_rgb(planes, bpc, layout, 1, 0, chr)
        for crop in ((3, 5, 41, 23), (26, 12, 41, 23), (66, 34, 1, 1), (5, 7, 1, 1), (0, 0, 67, 35), (1, 33, 66, 2)):
            for out in ((10, 6), (crop[2], crop[3]), (64, 33), (1, 1)):
                if crop[2] > 64 * out[0] or crop[3] > 64 * out[1]:
                    continue
                run(gpu, src, rgb, bpc, color, out, DTYPES[n % 4], ("chw", "hwc")[(n // 4) % 2], crop=crop, norm=True)
                n += 1


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_dtype(gpu, dtype, bpc):
    """Default scale and bias ([0, 1]) and a per-channel mean / std, resized and 1:1 (1:1 reaches
    every sample value of the blocks pattern: 0, M and the uint8 rounding's clip at 255)."""
    w, h, layout = 67, 35, 1
    rng = np.random.default_rng(bpc + dtype)
    color = MiColorInfo(1, 1, 1, 1, 0)
    for kind in ("random", "blocks"):
        planes = make_planes(rng, w, h, bpc, layout, kind)
        rgb = R.to_rgb(planes, bpc, layout, 1, 1, 0)
        src = to_frame(planes, w, h, bpc, layout)
        for norm in (False, True):
            for out in ((10, 6), (67, 35)):
                for order in ("chw", "hwc"):
                    run(gpu, src, rgb, bpc, color, out, dtype, order, norm=norm)


@pytest.mark.parametrize("dtype", DTYPES)
def test_destination_strides(gpu, dtype):
    """CHW and HWC, tight, with a padded row and one element off their alignment (the stores fall
    back from whole vectors to elements), and strides that are neither order."""
    w, h, bpc, layout = 67, 35, 10, 1
    rng = np.random.default_rng(dtype)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    rgb = R.to_rgb(planes, bpc, layout, 9, 0, 0)
    src = to_frame(planes, w, h, bpc, layout)
    color = MiColorInfo(1, 1, 9, 0, 0)
    for ow, oh in ((16, 6), (13, 5), (3, 2)):
        for order in ("chw", "hwc"):
            for pad, offset in ((0, 0), (4, 0), (3, 0), (0, 1), (5, 3)):
                run(gpu, src, rgb, bpc, color, (ow, oh), dtype, order, norm=True, pad=pad, offset=offset)
        # a column stride of 2 elements; rows before channels; columns slowest
        for strides in ((2 * ow * oh + 7, 2 * ow + 1, 2), (1, 3, 3 * oh + 2), (oh * ow, 1, oh)):
            run(gpu, src, rgb, bpc, color, (ow, oh), dtype, strides, norm=True)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.bfloat16, torch.float32])
def test_batch_tensors(gpu, dtype):
    """display_tensor into batch[n] of an NCHW and of a channels-last batch, into an (H, W, 3)
    tensor with channels_last, with crop, mean and std; the other slots stay as they were."""
    w, h, bpc, layout = 67, 35, 10, 1
    rng = np.random.default_rng(5)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    rgb = R.to_rgb(planes, bpc, layout, 1, 0, 0)
    src = to_frame(planes, w, h, bpc, layout)
    color = MiColorInfo(1, 1, 1, 0, 0)
    code = {torch.uint8: T_U8, torch.float16: T_F16, torch.bfloat16: T_BF16, torch.float32: T_F32}[dtype]
    crop = (3, 5, 41, 23)
    scale, bias = T.scale_bias(bpc, MEAN, STD)
    want = model(rgb, bpc, (12, 7), code, crop, scale, bias)
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[ES[code]]

    def host(t):      # bit patterns of a (3, H, W) tensor
        return bits(t.contiguous().view(view).cpu().numpy())

    for fmt in (torch.contiguous_format, torch.channels_last):
        batch = torch.zeros((3, 3, 7, 12), dtype=dtype, device="cuda").contiguous(memory_format=fmt)
        display_tensor(gpu, src, batch[1], color, crop=crop, mean=MEAN, std=STD)
        torch.cuda.synchronize()
        assert np.array_equal(host(batch[1]), want), fmt
        assert not host(batch[0]).any() and not host(batch[2]).any()
    hwc = torch.zeros((7, 12, 3), dtype=dtype, device="cuda")
    display_tensor(gpu, src, hwc, color, crop=crop, mean=MEAN, std=STD, channels_last=True)
    torch.cuda.synchronize()
    assert np.array_equal(host(hwc.permute(2, 0, 1)), want)
    im = tensor_image(batch[1], bpc, crop, MEAN, STD)
    assert (im.stride[0], im.stride[2]) == (ES[code], 3 * ES[code]) and (im.w, im.h, im.dtype) == (12, 7, code)
    assert [np.float32(v) for v in im.scale] == scale and [np.float32(v) for v in im.bias] == bias


def test_film_grain(gpu):
    """Grain on, 8-bit 4:2:0, odd width: the model is fed the oracle's grained picture."""
    from tests.test_oracle_lr import planes_for
    from rav1d_amd.frame import film_grain_data
    w, h, bpc, layout = 65, 33, 8, 1
    rng = np.random.default_rng(2)
    planes = planes_for(w, h, bpc, layout, rng)
    fg = make_fg_params(rng, layout)
    src = to_frame(planes, w, h, bpc, layout)
    ref = grain_reference(planes, w, h, bpc, layout, fg)
    rgb = R.to_rgb(ref, bpc, layout, 6, 0, 0)
    assert not np.array_equal(rgb, R.to_rgb(planes, bpc, layout, 6, 0, 0))
    color = MiColorInfo(1, 1, 6, 0, 0)
    data = film_grain_data(fg)
    run(gpu, src, rgb, bpc, color, (w, h), T_U8, fg=data)
    run(gpu, src, rgb, bpc, color, (20, 11), T_F16, "hwc", crop=(3, 5, 41, 23), norm=True, fg=data)
    for p in range(3):      # the device picture is untouched
        assert np.array_equal(src.plane_np(p), planes[p])


def test_scratch_reuse(gpu):
    """Calls of different geometry on one context and stream, enqueued back to back, each get
    their own result: the scratch grows, is reused by a smaller call and again by a larger one,
    and calls with the geometry of the one before them reuse its tap tables."""
    from rav1d_amd.frame import Context
    ctx = Context(0)      # a context of its own: the scratch starts unallocated
    rng = np.random.default_rng(7)
    jobs = []
    for (w, h, bpc, layout), out, dtype, crop in (((67, 35, 10, 1), (10, 6), T_F16, None),
                                                  ((136, 70, 8, 3), (64, 33), T_U8, (3, 5, 100, 60)),
                                                  ((17, 9, 12, 2), (5, 4), T_F32, None),
                                                  ((136, 70, 8, 3), (150, 80), T_BF16, None),
                                                  # the same two axes again: the tap tables are reused
                                                  ((136, 70, 10, 3), (150, 80), T_U8, None),
                                                  ((141, 73, 10, 1), (150, 80), T_F16, (5, 3, 136, 70)),
                                                  ((141, 73, 10, 1), (150, 81), T_F16, (5, 3, 136, 70))):
        planes = make_planes(rng, w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        d = Dest(out[0], out[1], dtype)
        scale, bias = T.scale_bias(bpc, MEAN, STD)
        assert call(ctx, src, d.image(bpc, crop, scale, bias), MiColorInfo(1, 1, 1, 0, 0)) == 0
        jobs.append((d, model(R.to_rgb(planes, bpc, layout, 1, 0, 0), bpc, out, dtype, crop, scale, bias), src))
    torch.cuda.synchronize()
    for i, (d, want, _) in enumerate(jobs):
        assert np.array_equal(d.elements(), want), i
    ctx.close()


def test_identity_matrix(gpu):
    """mtrx 0 with 4:4:4: G = Y, B = U, R = V, then the same resize."""
    w, h, layout = 65, 33, 3
    for bpc, dtype in ((8, T_U8), (10, T_F32), (12, T_F16)):
        rng = np.random.default_rng(bpc)
        planes = make_planes(rng, w, h, bpc, layout, "random")
        rgb = R.to_rgb(planes, bpc, layout, 0, 1, 0)
        assert np.array_equal(rgb[1], planes[0])
        src = to_frame(planes, w, h, bpc, layout)
        for out in ((w, h), (10, 6), (70, 40)):
            run(gpu, src, rgb, bpc, MiColorInfo(1, 13, 0, 1, 0), out, dtype, norm=True)


def test_rejections_with_a_context(gpu):
    """The host checks hold with a live context too, and leave the destination alone."""
    src = to_frame(make_planes(np.random.default_rng(1), 67, 35, 8, 1, "random"), 67, 35, 8, 1)
    d = Dest(10, 6, T_F16)
    for color, want in ((MiColorInfo(1, 1, 2, 0, 0), -22), (MiColorInfo(1, 1, 0, 0, 0), -22), (MiColorInfo(1, 1, 8, 0, 0), -95)):
        assert call(gpu, src, d.image(8), color) == want
    assert call(gpu, src, d.image(8, crop=(60, 0, 8, 8)), MiColorInfo(1, 1, 1, 0, 0)) == -22
    assert call(gpu, src, d.image(8, scale=(float("inf"), 1.0, 1.0)), MiColorInfo(1, 1, 1, 0, 0)) == -22
    torch.cuda.synchronize()
    assert d.untouched()
