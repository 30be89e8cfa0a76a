"""GPU: mi_display_picture (include/mi_av1out.h, csrc/display.hip). The semi-planar formats are
the source's visible area re-interleaved (with grain: the oracle's rav1d_apply_grain of the same
input), the RGB formats are tests/display_ref.py's integer model, all bit for bit; nothing
outside w x h of the destination is touched."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (OUT_RGB_PLANAR, OUT_RGBA_PACKED, OUT_SEMIPLANAR, DisplayImage, MiDisplayImage,
                               display_picture)
from rav1d_amd.synth import make_fg_params
from tests import display_ref as R
from tests import oracle_lib
from tests.test_lr_gpu import to_frame
from tests.test_oracle_lf import pad_planes

pytestmark = pytest.mark.gpu

# odd both ways; crossing an 8-pixel run, a 64-lane row, a 128-aligned plane edge
SIZES = [(2, 2), (17, 9), (65, 33), (136, 70)]
FILL = 0xA5


def make_planes(rng, w, h, bpc, layout, kind):
    m, half = (1 << bpc) - 1, 1 << (bpc - 1)
    cw, ch = R.chroma_size(w, h, layout)
    shapes = [(h, w)] + ([(ch, cw)] * 2 if layout else [])
    dt = np.uint8 if bpc == 8 else np.uint16
    if kind == "random":
        return [rng.integers(0, m + 1, s).astype(dt) for s in shapes]
    # 3 x 3 blocks of 0, M and H, independent per plane: every clip of the matrix fires
    return [rng.choice([0, m, half], size=((s[0] + 2) // 3, (s[1] + 2) // 3)).repeat(3, 0).repeat(3, 1)[:s[0], :s[1]]
            .astype(dt) for s in shapes]


class Dest:
    """Destination planes in one guarded device buffer each: `offset` bytes in front, `pad`
    bytes after every row, a guard band after the last row, all filled with FILL."""

    def __init__(self, fmt, w, h, bpc, layout, pad=0, offset=0):
        self.pxb = 1 if bpc == 8 else 2
        cw, ch = R.chroma_size(w, h, layout)
        if fmt == OUT_SEMIPLANAR:
            self.shapes = [(h, w)] + ([(ch, 2 * cw)] if layout else [])
        elif fmt == OUT_RGB_PLANAR:
            self.shapes = [(h, w)] * 3
        else:
            self.shapes = [(h, 4 * w)]
        self.offset = offset
        self.strides = [s[1] * self.pxb + pad for s in self.shapes]
        self.bufs = [torch.full((offset + s[0] * st + 96,), FILL, dtype=torch.uint8, device="cuda")
                     for s, st in zip(self.shapes, self.strides)]
        self.im = MiDisplayImage()
        self.im.w, self.im.h, self.im.format, self.im.bpc = w, h, fmt, bpc
        for p, b in enumerate(self.bufs):
            assert b.data_ptr() % 16 == 0
            self.im.data[p], self.im.stride[p] = b.data_ptr() + offset, self.strides[p]

    def planes(self):
        """The written samples per plane; asserts that every other byte still holds FILL."""
        out = []
        for (rows, n), st, b in zip(self.shapes, self.strides, self.bufs):
            host = b.cpu().numpy()
            body = host[self.offset:self.offset + rows * st].reshape(rows, st)
            assert np.all(host[:self.offset] == FILL) and np.all(host[self.offset + rows * st:] == FILL), "guard band"
            assert np.all(body[:, n * self.pxb:] == FILL), "row padding"
            vis = np.ascontiguousarray(body[:, :n * self.pxb])
            out.append(vis.view("<u2") if self.pxb == 2 else vis)
        return out


def check_semiplanar(got, planes, bpc, layout):
    y, uv = R.semiplanar(planes, bpc, layout)
    assert np.array_equal(got[0], y), "Y"
    if layout:
        assert np.array_equal(got[1].reshape(uv.shape), uv), "UV"
    else:
        assert len(got) == 1


def pad_for(bpc, odd):
    """A padded, odd stride: an odd number of bytes (8 bpc) or of 16-bit samples."""
    return 0 if not odd else (13 if bpc == 8 else 26)


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_semiplanar_is_the_picture(gpu, size, layout, bpc):
    w, h = size
    rng = np.random.default_rng(w * 1000 + layout * 10 + bpc)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    for odd, offset in ((False, 0), (True, 0), (True, 2)):
        d = Dest(OUT_SEMIPLANAR, w, h, bpc, layout, pad_for(bpc, odd), offset)
        display_picture(gpu, src, d.im)      # colour may be NULL
        torch.cuda.synchronize()
        check_semiplanar(d.planes(), planes, bpc, layout)
    for p in range(len(planes)):
        assert np.array_equal(src.plane_np(p), planes[p])


# (mtrx, full range, chr): matrices 1, 6 and 9, both ranges, every chroma siting
COMBOS = [(1, 0, 0), (1, 1, 2), (6, 0, 1), (6, 1, 0), (9, 0, 2), (9, 1, 1)]


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgb_matches_integer_model(gpu, size, layout, bpc):
    w, h = size
    rng = np.random.default_rng(w * 1000 + layout * 10 + bpc + 1)
    sources = []
    for kind in ("random", "blocks"):
        planes = make_planes(rng, w, h, bpc, layout, kind)
        sources.append((kind, planes, to_frame(planes, w, h, bpc, layout)))
    combos = COMBOS + ([(0, 1, 0), (0, 0, 2)] if layout == 3 else [])
    for i, (mtrx, full, chr) in enumerate(combos):
        color = MiColorInfo(1, 1, mtrx, full, chr)
        for kind, planes, src in sources:
            want = R.to_rgb(planes, bpc, layout, mtrx, full, chr)
            # aligned and tight, then 2 bytes off 16-byte alignment with a padded, odd stride
            for pad, offset in ((0, 0), (pad_for(bpc, True), 2)):
                # (alternate which format takes which destination, both across the combinations)
                fmt = OUT_RGB_PLANAR if (i + (offset > 0) + (kind == "blocks")) % 2 == 0 else OUT_RGBA_PACKED
                d = Dest(fmt, w, h, bpc, layout, pad, offset)
                display_picture(gpu, src, d.im, color)
                torch.cuda.synchronize()
                got = d.planes()
                what = (mtrx, full, chr, kind, fmt, offset)
                if fmt == OUT_RGB_PLANAR:
                    assert np.array_equal(np.stack(got), want), what
                else:
                    assert np.array_equal(got[0].reshape(h, w, 4), R.to_rgba(planes, bpc, layout, mtrx, full, chr)), what


@pytest.mark.parametrize("bpc,layout", [(8, 1), (10, 1), (12, 3), (10, 2), (8, 0), (10, 3)])
def test_both_rgb_formats_every_destination(gpu, bpc, layout):
    """Planar and packed, each aligned and each on the tail path, at one size with both an 8-pixel
    run tail and a row-pair tail."""
    w, h = 77, 35
    rng = np.random.default_rng(bpc + layout)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color = MiColorInfo(1, 1, 9, 0, 0)
    for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED):
        for pad, offset in ((0, 0), (pad_for(bpc, True), 0), (0, 2)):
            d = Dest(fmt, w, h, bpc, layout, pad, offset)
            display_picture(gpu, src, d.im, color)
            torch.cuda.synchronize()
            got = d.planes()
            if fmt == OUT_RGB_PLANAR:
                assert np.array_equal(np.stack(got), R.to_rgb(planes, bpc, layout, 9, 0, 0))
            else:
                assert np.array_equal(got[0].reshape(h, w, 4), R.to_rgba(planes, bpc, layout, 9, 0, 0))


@pytest.mark.parametrize("bpc,layout", [(8, 1), (10, 1), (12, 3), (8, 0), (10, 2)])
def test_packed_rgba_wide_rows(gpu, bpc, layout):
    """Wider than a wave's 512 columns: the first wave of a row stores its runs through the LDS
    hand-off, the second (partly outside the row) and every unaligned destination lane by lane."""
    w, h = 1100, 5
    rng = np.random.default_rng(bpc * 7 + layout)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    want = R.to_rgba(planes, bpc, layout, 1, 0, 1)
    for pad, offset in ((0, 0), (16 * 3, 0), (pad_for(bpc, True), 2)):
        d = Dest(OUT_RGBA_PACKED, w, h, bpc, layout, pad, offset)
        display_picture(gpu, src, d.im, MiColorInfo(1, 1, 1, 0, 1))
        torch.cuda.synchronize()
        assert np.array_equal(d.planes()[0].reshape(h, w, 4), want), (pad, offset)


def grain_reference(planes, w, h, bpc, layout, fg, is_id=0):
    ref = oracle_lib.film_grain(pad_planes(planes, w, h, bpc, layout), bpc, layout, w, h, fg, is_id)
    return [ref[p][:planes[p].shape[0], :planes[p].shape[1]] for p in range(len(planes))]


@pytest.mark.parametrize("bpc,layout,size,seed", [(8, 1, (65, 33), 2), (10, 1, (136, 70), 1), (12, 3, (65, 33), 3),
                                                   (10, 2, (136, 70), 4), (8, 0, (136, 70), 5)])
def test_semiplanar_with_grain_matches_oracle(gpu, bpc, layout, size, seed):
    from tests.test_oracle_lr import planes_for
    w, h = size
    rng = np.random.default_rng(seed)
    planes = planes_for(w, h, bpc, layout, rng)
    fg = make_fg_params(rng, layout)
    src = to_frame(planes, w, h, bpc, layout)
    d = Dest(OUT_SEMIPLANAR, w, h, bpc, layout, pad_for(bpc, True), 0)
    display_picture(gpu, src, d.im, None, fg)
    torch.cuda.synchronize()
    check_semiplanar(d.planes(), grain_reference(planes, w, h, bpc, layout, fg), bpc, layout)
    for p in range(len(planes)):      # the device picture is untouched
        assert np.array_equal(src.plane_np(p), planes[p])


def test_grain_scratch_across_geometries(gpu):
    """The context's grained picture is reused by a smaller or equal geometry and replaced by a
    larger one; RGB reads the grained chroma (identity matrix: the grain's own clip)."""
    from rav1d_amd.frame import Context
    from tests.test_oracle_lr import planes_for
    ctx = Context(0)      # a context of its own: the scratch starts unallocated
    rng = np.random.default_rng(11)
    for w, h, bpc, layout in ((136, 70, 10, 1), (65, 33, 10, 1), (136, 70, 8, 3), (136, 70, 10, 1), (260, 140, 12, 3),
                              (65, 33, 8, 0)):
        planes = planes_for(w, h, bpc, layout, rng)
        fg = make_fg_params(rng, layout)
        src = to_frame(planes, w, h, bpc, layout)
        mtrx = 0 if layout == 3 else 6
        color = MiColorInfo(1, 1, mtrx, 1, 0)
        image = DisplayImage(w, h, bpc, layout, "rgb")
        display_picture(ctx, src, image, color, fg)
        d = Dest(OUT_SEMIPLANAR, w, h, bpc, layout)
        display_picture(ctx, src, d.im, color, fg)
        torch.cuda.synchronize()
        ref = grain_reference(planes, w, h, bpc, layout, fg, int(mtrx == 0))
        check_semiplanar(d.planes(), ref, bpc, layout)
        assert np.array_equal(image.numpy()[0], R.to_rgb(ref, bpc, layout, mtrx, 1, 0)), (w, h, bpc, layout)
    ctx.close()


def test_display_image_tensors(gpu):
    """DisplayImage allocates the tensors the formats name; display_picture fills them."""
    w, h, bpc, layout = 17, 9, 10, 1
    rng = np.random.default_rng(3)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color = MiColorInfo(1, 1, 1, 0, 1)
    nv = DisplayImage(w, h, bpc, layout, "nv12")
    assert nv.y.shape == (h, w) and nv.uv.shape == (5, 9, 2) and nv.y.dtype == torch.int16 and nv.y.is_cuda
    rgb, rgba = DisplayImage(w, h, bpc, layout, "rgb"), DisplayImage(w, h, bpc, layout, OUT_RGBA_PACKED)
    assert rgb.rgb.shape == (3, h, w) and rgba.rgba.shape == (h, w, 4)
    assert DisplayImage(w, h, 8, 0, "nv12").uv is None and DisplayImage(w, h, 8, 0, "nv12").y.dtype == torch.uint8
    for im in (nv, rgb, rgba):
        display_picture(gpu, src, im, color)
    torch.cuda.synchronize()
    y, uv = R.semiplanar(planes, bpc, layout)
    assert np.array_equal(nv.numpy()[0], y) and np.array_equal(nv.numpy()[1], uv)
    assert np.array_equal(rgb.numpy()[0], R.to_rgb(planes, bpc, layout, 1, 0, 1))
    assert np.array_equal(rgba.numpy()[0], R.to_rgba(planes, bpc, layout, 1, 0, 1))


def test_rejections_with_a_context(gpu):
    """The host checks hold with a live context too, and leave the destination alone."""
    src = to_frame(make_planes(np.random.default_rng(1), 17, 9, 8, 1, "random"), 17, 9, 8, 1)
    pic = src.picture()
    d = Dest(OUT_RGB_PLANAR, 17, 9, 8, 1)
    for color, want in ((None, -22), (MiColorInfo(1, 1, 2, 0, 0), -22), (MiColorInfo(1, 1, 0, 0, 0), -22),
                        (MiColorInfo(1, 1, 8, 0, 0), -95)):
        r = lib().mi_display_picture(gpu.h, ctypes.byref(pic), ctypes.byref(d.im),
                                     ctypes.byref(color) if color is not None else None, None, None)
        assert r == want
    torch.cuda.synchronize()
    d.planes()
    assert all(np.all(b.cpu().numpy() == FILL) for b in d.bufs)
