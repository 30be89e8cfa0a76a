"""GPU: mi_display_scaled (include/mi_av1out.h, csrc/scaled.hip) against tests/scaled_ref.py, bit
for bit; nothing outside the w x h luma samples and the cw x ch UV pairs of a destination is
touched (fill byte, guard bands in front and behind, row padding)."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (OUT_SEMIPLANAR, MiScaledImage, ScaledImage, display_picture, display_scaled,
                               display_tensor)
from rav1d_amd.frame import _stream_ptr, film_grain_data
from rav1d_amd.synth import make_fg_params
from tests import display_ref as R
from tests import scaled_ref as Z
from tests import tensor_ref as T
from tests.test_display_gpu import Dest as DisplayDest
from tests.test_display_gpu import SIZES, grain_reference, make_planes
from tests.test_lr_gpu import to_frame

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64
EINVAL = -22


class Dest:
    """One rung's destination: the Y and the UV plane in one guarded device buffer each, filled
    with FILL: a guard band and `offset` samples in front, `pad` samples after every row, a guard
    band after the last row."""

    def __init__(self, w, h, bpc, layout, crop=None, pad=0, offset=0):
        self.w, self.h, self.bpc, self.layout, self.crop = w, h, bpc, layout, crop
        self.es = 1 if bpc == 8 else 2
        cw, ch = R.chroma_size(w, h, layout)
        self.shapes = [(h, w)] + ([(ch, 2 * cw)] if layout else [])
        self.first = GUARD + offset * self.es
        self.strides = [(s[1] + pad) * self.es for s in self.shapes]
        self.bufs = [torch.full((self.first + s[0] * st + GUARD,), FILL, dtype=torch.uint8, device="cuda")
                     for s, st in zip(self.shapes, self.strides)]
        self.im = MiScaledImage()
        self.im.w, self.im.h, self.im.bpc = w, h, bpc
        for p, b in enumerate(self.bufs):
            assert b.data_ptr() % 64 == 0
            self.im.data[p], self.im.stride[p] = b.data_ptr() + self.first, self.strides[p]
        if crop is not None:
            self.im.crop_x, self.im.crop_y, self.im.crop_w, self.im.crop_h = crop

    def planes(self):
        """(Y (h, w), UV (ch, cw, 2) or None); asserts that every other byte still holds FILL."""
        out = []
        for (rows, n), st, b in zip(self.shapes, self.strides, self.bufs):
            host = b.cpu().numpy()
            body = host[self.first:self.first + rows * st].reshape(rows, st)
            assert np.all(host[:self.first] == FILL) and np.all(host[self.first + rows * st:] == FILL), "guard band"
            assert np.all(body[:, n * self.es:] == FILL), "row padding"
            vis = np.ascontiguousarray(body[:, :n * self.es])
            out.append(vis.view("<u2") if self.es == 2 else vis)
        return out[0], (out[1].reshape(out[1].shape[0], -1, 2) if self.layout else None)

    def untouched(self):
        return all(bool(np.all(b.cpu().numpy() == FILL)) for b in self.bufs)


def call(ctx, src, dests, chr=0, fg=None, color=True):
    pic = src.picture()
    ims = (MiScaledImage * len(dests))(*[d.im for d in dests])
    col = MiColorInfo(1, 1, 1, 0, chr)
    return lib().mi_display_scaled(ctx.h, ctypes.byref(pic), ims, len(dests), ctypes.byref(col) if color else None,
                                   ctypes.byref(fg) if fg is not None else None, _stream_ptr(None))


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), ("Y",) + what + (np.argwhere(got[0] != want[0])[:4].tolist(),)
    if want[1] is None:
        assert got[1] is None
    else:
        assert np.array_equal(got[1], want[1]), ("UV",) + what + (np.argwhere(got[1] != want[1])[:4].tolist(),)


def run(ctx, src, planes, bpc, layout, chr, size, obpc=None, crop=None, pad=0, offset=0, fg=None):
    """One single-rung call into a guarded destination, compared with the model of `planes`."""
    obpc = bpc if obpc is None else obpc
    d = Dest(size[0], size[1], obpc, layout, crop, pad, offset)
    assert call(ctx, src, [d], chr, fg) == 0
    torch.cuda.synchronize()
    got = d.planes()
    same(got, Z.scaled(planes, bpc, layout, chr, size, obpc, crop), (size, bpc, obpc, layout, chr, crop, pad, offset))
    return got


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_to_one_is_the_semiplanar_picture(gpu, size):
    """1:1, the source's depth, no crop: mi_display_picture's MI_OUT_SEMIPLANAR on the same input,
    for every layout and depth, and the model."""
    w, h = size
    for layout in range(4):
        for bpc in (8, 10, 12):
            rng = np.random.default_rng(w * 1000 + layout * 10 + bpc)
            planes = make_planes(rng, w, h, bpc, layout, "random")
            src = to_frame(planes, w, h, bpc, layout)
            ref = DisplayDest(OUT_SEMIPLANAR, w, h, bpc, layout)
            display_picture(gpu, src, ref.im)
            got = run(gpu, src, planes, bpc, layout, 2, size)
            want = ref.planes()
            assert np.array_equal(got[0], want[0]), (layout, bpc)
            if layout:
                assert np.array_equal(got[1].reshape(want[1].shape), want[1]), (layout, bpc)


# per source size: a downscale, an upscale, down in x with up in y, and (where the source has them)
# 128 columns to 2: 64:1 on the luma axis and on the chroma axis
OUTPUTS = {(2, 2): [(1, 1), (5, 3), (1, 4)],
           (17, 9): [(5, 4), (33, 20), (9, 14)],
           (65, 33): [(24, 10), (70, 40), (30, 40)],
           (136, 70): [(50, 31), (150, 81), (40, 90), ((2, 9), (0, 0, 128, 70)), ((2, 2), (8, 6, 128, 64))]}
# (layout, chr): every subsampling, and every siting of 4:2:0
SITINGS = [(0, 0), (1, 0), (1, 1), (1, 2), (2, 0), (3, 0)]


@pytest.mark.parametrize("layout,chr", SITINGS, ids=[f"layout{a}-chr{b}" for a, b in SITINGS])
def test_resampling(gpu, layout, chr):
    n = 0
    for (w, h), outs in OUTPUTS.items():
        for bpc in (8, 10, 12):
            rng = np.random.default_rng(w * 100 + layout * 10 + bpc)
            planes = make_planes(rng, w, h, bpc, layout, "random" if (n + bpc) % 4 else "blocks")
            src = to_frame(planes, w, h, bpc, layout)
            for out in outs:
                size, crop = out if isinstance(out[0], tuple) else (out, None)
                run(gpu, src, planes, bpc, layout, chr, size, crop=crop)
                n += 1


@pytest.mark.parametrize("src_size,out", [((1100, 6), (1500, 4)), ((2500, 4), (40, 2)), ((2500, 4), (1030, 7))],
                         ids=["upscale", "downscale", "mixed"])
def test_rows_wider_than_a_segment(gpu, src_size, out):
    """The horizontal pass splits a row's outputs into workgroup segments (at most 1024 outputs,
    and no more than reach 2048 source columns), the vertical pass into workgroups of 1024
    columns; luma and chroma split differently."""
    w, h = src_size
    for layout, bpc, obpc in ((1, 8, 8), (3, 10, 8), (2, 12, 10), (0, 10, 12)):
        rng = np.random.default_rng(w + layout)
        planes = make_planes(rng, w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        run(gpu, src, planes, bpc, layout, 0, out, obpc)
        run(gpu, src, planes, bpc, layout, 2, out, obpc, crop=(36, 0, w - 50, h))


@pytest.mark.parametrize("obpc", [8, 10, 12])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_depth_to_every_depth(gpu, bpc, obpc):
    """Random planes and the 0 / M / half block pattern, resized and 1:1 (1:1 reaches every value of
    the block pattern: 0, M and the clip of the rounding at Md)."""
    w, h = 65, 33
    for layout, chr in ((1, 2), (3, 0)):
        rng = np.random.default_rng(bpc * 16 + obpc + layout)
        for kind in ("random", "blocks"):
            planes = make_planes(rng, w, h, bpc, layout, kind)
            src = to_frame(planes, w, h, bpc, layout)
            for size in ((24, 10), (w, h), (70, 40)):
                run(gpu, src, planes, bpc, layout, chr, size, obpc)


@pytest.mark.parametrize("layout", [1, 2, 3, 0])
def test_crops(gpu, layout):
    """An even-origin crop, a crop reaching the odd right and bottom edges with odd extents, crops
    of one chroma sample (inside, and the single luma sample of the odd corner); outputs smaller,
    equal and larger."""
    w, h, bpc = 65, 33, 10
    rng = np.random.default_rng(layout)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    for chr in (0, 2):
        for crop in ((4, 6, 40, 22), (26, 12, 39, 21), (10, 8, 2, 2), (64, 32, 1, 1), (0, 0, 65, 33)):
            for size in ((10, 6), (crop[2], crop[3]), (64, 33)):
                if crop[2] > 64 * size[0] or crop[3] > 64 * size[1]:
                    continue
                run(gpu, src, planes, bpc, layout, chr, size, 8 if chr else 10, crop=crop)


@pytest.mark.parametrize("obpc", [8, 10])
def test_destination_strides_and_offsets(gpu, obpc):
    """Tight, a padded odd stride, a pointer one sample off, both: the stores fall back from whole
    vectors to samples. Widths that end inside a lane's run of 4 and on it."""
    w, h, bpc = 65, 33, 10
    for layout in (1, 3, 0):
        rng = np.random.default_rng(obpc + layout)
        planes = make_planes(rng, w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        for size in ((16, 6), (13, 5), (3, 2), (65, 33)):
            for pad, offset in ((0, 0), (4, 0), (3, 0), (0, 1), (5, 3), (8, 4)):
                run(gpu, src, planes, bpc, layout, 0, size, obpc, pad=pad, offset=offset)


def test_film_grain(gpu):
    """Grain on: the model is fed the oracle's grained picture; every rung reads it."""
    from tests.test_oracle_lr import planes_for
    for (w, h, bpc, layout), seed in (((65, 33, 8, 1), 2), ((136, 70, 10, 1), 1), ((65, 33, 12, 3), 3)):
        rng = np.random.default_rng(seed)
        planes = planes_for(w, h, bpc, layout, rng)
        fg = make_fg_params(rng, layout)
        src = to_frame(planes, w, h, bpc, layout)
        ref = grain_reference(planes, w, h, bpc, layout, fg)
        assert not np.array_equal(ref[0], planes[0])
        data = film_grain_data(fg)
        run(gpu, src, ref, bpc, layout, 0, (w, h), fg=data)
        run(gpu, src, ref, bpc, layout, 2, (20, 11), 8, crop=(2, 4, 40, 22), fg=data)
        dests = [Dest(30, 17, bpc, layout), Dest(9, 40, 8, layout, (0, 0, w, h))]
        assert call(gpu, src, dests, 1, data) == 0
        torch.cuda.synchronize()
        same(dests[0].planes(), Z.scaled(ref, bpc, layout, 1, (30, 17)), ("rung 0",))
        same(dests[1].planes(), Z.scaled(ref, bpc, layout, 1, (9, 40), 8), ("rung 1",))
        for p in range(len(planes)):      # the device picture is untouched
            assert np.array_equal(src.plane_np(p), planes[p])


@pytest.mark.parametrize("layout,bpc", [(1, 10), (3, 8), (2, 12), (0, 10)])
def test_ladder_equals_single_calls(gpu, layout, bpc):
    """Three rungs of different sizes, depths and crops in one call equal three single calls and
    the model; no rung's guard band or padding is touched."""
    w, h = 136, 70
    rng = np.random.default_rng(layout * 3 + bpc)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    rungs = [((68, 35), 8, None, 0, 0), ((45, 22), bpc, (8, 6, 120, 60), 3, 1), ((150, 20), 12, (100, 40, 36, 30), 0, 0)]
    for chr in (0, 2):
        ladder = [Dest(s[0], s[1], obpc, layout, crop, pad, off) for s, obpc, crop, pad, off in rungs]
        assert call(gpu, src, ladder, chr) == 0
        single = [Dest(s[0], s[1], obpc, layout, crop, pad, off) for s, obpc, crop, pad, off in rungs]
        for d in single:
            assert call(gpu, src, [d], chr) == 0
        torch.cuda.synchronize()
        for i, (s, obpc, crop, _, _) in enumerate(rungs):
            got = ladder[i].planes()
            same(got, single[i].planes(), ("single", i, chr))
            same(got, Z.scaled(planes, bpc, layout, chr, s, obpc, crop), ("model", i, chr))


def test_eight_rungs(gpu):
    w, h, bpc, layout = 65, 33, 8, 1
    planes = make_planes(np.random.default_rng(8), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    sizes = [(65, 33), (33, 17), (16, 8), (8, 4), (4, 2), (2, 1), (100, 50), (7, 60)]
    dests = [Dest(s[0], s[1], (8, 10, 12)[i % 3], layout) for i, s in enumerate(sizes)]
    assert call(gpu, src, dests, 0, color=False) == 0       # NULL color: chr 0
    torch.cuda.synchronize()
    for i, (s, d) in enumerate(zip(sizes, dests)):
        same(d.planes(), Z.scaled(planes, bpc, layout, 0, s, d.bpc), (i,))


def test_scratch_and_tap_table_reuse(gpu):
    """One context of its own, calls enqueued back to back: alternating geometries, the same
    geometry again (its tables are reused), the same extents with another siting (they are not),
    and mi_display_tensor in between with the same extents (its tables and these are never taken
    for one another). Each result equals its model."""
    from rav1d_amd.frame import Context
    ctx = Context(0)      # a context of its own: the scratch starts unallocated
    rng = np.random.default_rng(7)
    color = MiColorInfo(1, 1, 1, 0, 0)
    sources = {}
    for w, h, bpc, layout in ((136, 70, 10, 1), (65, 33, 8, 3), (136, 70, 8, 1)):
        planes = make_planes(rng, w, h, bpc, layout, "random")
        sources[(w, h, bpc, layout)] = (planes, to_frame(planes, w, h, bpc, layout))
    jobs = []
    plan = [("scaled", (136, 70, 10, 1), (50, 31), 0), ("tensor", (136, 70, 10, 1), (50, 31), 0),
            ("scaled", (136, 70, 10, 1), (50, 31), 0), ("scaled", (136, 70, 10, 1), (50, 31), 2),
            ("scaled", (65, 33, 8, 3), (70, 40), 0), ("tensor", (65, 33, 8, 3), (70, 40), 0),
            ("scaled", (136, 70, 8, 1), (50, 31), 2), ("tensor", (136, 70, 8, 1), (25, 16), 0),
            ("scaled", (136, 70, 8, 1), (25, 16), 0), ("scaled", (136, 70, 10, 1), (150, 81), 1),
            ("tensor", (136, 70, 10, 1), (50, 31), 0), ("scaled", (136, 70, 10, 1), (50, 31), 0)]
    for kind, key, size, chr in plan:
        planes, src = sources[key]
        w, h, bpc, layout = key
        if kind == "scaled":
            d = Dest(size[0], size[1], bpc, layout)
            assert call(ctx, src, [d], chr) == 0
            jobs.append((d, Z.scaled(planes, bpc, layout, chr, size)))
        else:
            out = torch.zeros((3, size[1], size[0]), dtype=torch.uint8, device="cuda")
            display_tensor(ctx, src, out, color)
            jobs.append((out, T.tensor(planes, bpc, layout, (1, 0, 0), None, size, T.U8)))
    torch.cuda.synchronize()
    for i, (d, want) in enumerate(jobs):
        if isinstance(d, Dest):
            same(d.planes(), want, (i,))
        else:
            assert np.array_equal(d.cpu().numpy(), want), i
    ctx.close()


def test_tensor_and_scaled_share_luma_axes(gpu):
    """The two outputs fill their tap tables with one kernel and key them by the axis list. One
    context of its own, a 4:2:0 source with chr 2, mi_display_tensor and mi_display_scaled to the
    same 24 x 10 in turn, three times round: the luma axes of the two are identical (66 -> 24 and
    34 -> 10, centred) and only the scaled output's co-sited chroma axes differ, the smallest case
    in which tables or keys taken for one another would show. Each result equals its model."""
    from rav1d_amd.frame import Context
    ctx = Context(0)
    w, h, bpc, layout, chr, size = 66, 34, 8, 1, 2, (24, 10)
    planes = make_planes(np.random.default_rng(11), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    want_t = T.tensor(planes, bpc, layout, (1, 0, chr), None, size, T.U8)
    want_s = Z.scaled(planes, bpc, layout, chr, size)
    jobs = []
    for _ in range(3):
        out = torch.zeros((3, size[1], size[0]), dtype=torch.uint8, device="cuda")
        display_tensor(ctx, src, out, MiColorInfo(1, 1, 1, 0, chr))
        d = Dest(size[0], size[1], bpc, layout)
        assert call(ctx, src, [d], chr) == 0
        jobs.append((out, d))
    torch.cuda.synchronize()
    for i, (out, d) in enumerate(jobs):
        assert np.array_equal(out.cpu().numpy(), want_t), i
        same(d.planes(), want_s, (i,))
    ctx.close()


def test_scaled_image_tensors(gpu):
    """ScaledImage allocates the tensors; display_scaled fills one image or a list of them."""
    w, h, bpc, layout = 17, 9, 10, 1
    planes = make_planes(np.random.default_rng(3), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color = MiColorInfo(1, 1, 1, 0, 2)
    a, b = ScaledImage(8, 4, 10, layout), ScaledImage(9, 5, 8, layout, crop=(2, 2, 15, 7))
    y, uv = a.tensors()
    assert y.shape == (4, 8) and uv.shape == (2, 4, 2) and y.dtype == torch.int16 and y.is_cuda
    assert b.y.dtype == torch.uint8 and b.uv.shape == (3, 5, 2)
    mono = ScaledImage(8, 4, 8, 0)
    assert mono.tensors()[1] is None and len(mono.numpy()) == 1
    display_scaled(gpu, src, [a, b], color)
    c = ScaledImage(8, 4, 10, layout)
    display_scaled(gpu, src, c, color)
    torch.cuda.synchronize()
    for im, want in ((a, Z.scaled(planes, bpc, layout, 2, (8, 4))), (b, Z.scaled(planes, bpc, layout, 2, (9, 5), 8, (2, 2, 15, 7))),
                     (c, Z.scaled(planes, bpc, layout, 2, (8, 4)))):
        got = im.numpy()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_arguments_with_a_context(gpu):
    """The tables of tests/test_scaled_args.py with a live context: every PASSING call returns 0,
    every REJECTED call -EINVAL and leaves the destination alone."""
    from tests.test_scaled_args import BASE, PASSING, REJECTED, arguments
    frames = {}
    buf = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 64 == 0

    def one(case):
        k = dict(BASE, **case)
        key = (k["w"], k["h"], k["bpc"], k["layout"])
        if key not in frames:
            frames[key] = to_frame(make_planes(np.random.default_rng(1), *key, "random"), *key)
        pic = frames[key].picture()
        args, _keep = arguments(case, pic, buf.data_ptr() + 64, buf.data_ptr() + 32768)
        return lib().mi_display_scaled(gpu.h, *args[:-1], _stream_ptr(None))

    for name, case in REJECTED:
        assert one(case) == EINVAL, name
    torch.cuda.synchronize()
    assert bool(np.all(buf.cpu().numpy() == FILL))
    for name, case in PASSING:
        assert one(case) == 0, name
    torch.cuda.synchronize()
    assert not bool(np.all(buf.cpu().numpy() == FILL))
