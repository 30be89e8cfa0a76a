"""GPU: mi_display_yuv_tm and mi_display_scaled_tm (include/mi_av1out.h, csrc/yuv_tm.hip) against
tests/yuv_tm_ref.py's model of the picture Q over the library's own tone tables, and
tests/scaled_ref.py / tests/cubic_ref.py run on Q: bit for bit; nothing outside the w x h luma
samples and the cw x ch UV pairs of a destination is touched (fill byte, guard bands in front and
behind, row padding), the source planes stay what they were."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (OUT_SEMIPLANAR, DisplayImage, MiDisplayImage, MiScaledImage, Resample, ScaledImage, ToneMap,
                               YuvTarget, display_scaled, display_yuv, output_colour, tonemap_tables)
from rav1d_amd.frame import _stream_ptr, film_grain_data
from rav1d_amd.synth import make_fg_params
from tests import cubic_ref as C
from tests import display_ref as R
from tests import scaled_ref as Z
from tests import yuv_tm_ref as Q
from tests.test_display_gpu import grain_reference, make_planes
from tests.test_lr_gpu import to_frame
from tests.test_scaled_gpu import FILL, GUARD, Dest, same
from tests.test_tonemap_gpu import setup, unchanged

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
PQ, SDR709, P3 = 0, 3, 2      # indices into SETUPS: PQ / BT.2020 -> sRGB / BT.709; BT.709 / BT.709; sRGB / P3 -> BT.2020


def planes_of(rng, w, h, bpc, layout, kind):
    """make_planes's "random" and "blocks" (3 x 3 blocks of 0, M and H), and all 0, all M and a
    checkerboard of 0 and M in every plane."""
    if kind in ("random", "blocks"):
        return make_planes(rng, w, h, bpc, layout, kind)
    m = (1 << bpc) - 1
    cw, ch = R.chroma_size(w, h, layout)
    dt = np.uint8 if bpc == 8 else np.uint16
    out = []
    for ph, pw in [(h, w)] + ([(ch, cw)] * 2 if layout else []):
        yy, xx = np.mgrid[0:ph, 0:pw]
        out.append({"zeros": np.zeros((ph, pw)), "max": np.full((ph, pw), m), "checker": ((xx + yy) & 1) * m}[kind].astype(dt))
    return out


class AlignedDest(Dest):
    """tests/test_scaled_gpu.py's Dest with the row padding chosen per plane: every row starts 16-byte
    aligned and ends in 16 to 31 bytes of padding, so the stores are whole vectors wherever a run
    lies inside the row, whatever the width, and sample by sample in the row's last run."""

    def __init__(self, w, h, bpc, layout):
        super().__init__(w, h, bpc, layout)
        self.strides = [((s[1] * self.es + 15) & ~15) + 16 for s in self.shapes]
        self.bufs = [torch.full((self.first + s[0] * st + GUARD,), FILL, dtype=torch.uint8, device="cuda")
                     for s, st in zip(self.shapes, self.strides)]
        for p, b in enumerate(self.bufs):
            assert b.data_ptr() % 64 == 0
            self.im.data[p], self.im.stride[p] = b.data_ptr() + self.first, self.strides[p]


def yuv_image(d):
    """The MiDisplayImage over a tests/test_scaled_gpu.py Dest."""
    im = MiDisplayImage()
    im.w, im.h, im.format, im.bpc = d.w, d.h, OUT_SEMIPLANAR, d.bpc
    for p in range(len(d.bufs)):
        im.data[p], im.stride[p] = d.im.data[p], d.im.stride[p]
    return im


def call_yuv(ctx, src, d, color, tm, target, fg=None):
    pic, im = src.picture(), yuv_image(d)
    return lib().mi_display_yuv_tm(ctx.h, ctypes.byref(pic), ctypes.byref(im), ctypes.byref(color), ctypes.byref(tm),
                                   ctypes.byref(target), ctypes.byref(fg) if fg is not None else None, _stream_ptr(None))


def call_scaled(ctx, src, dests, color, tm, target, rs=None, fg=None):
    pic = src.picture()
    ims = (MiScaledImage * len(dests))(*[d.im for d in dests])
    return lib().mi_display_scaled_tm(ctx.h, ctypes.byref(pic), ims, len(dests), ctypes.byref(color), ctypes.byref(tm),
                                      ctypes.byref(target), ctypes.byref(rs) if rs is not None else None,
                                      ctypes.byref(fg) if fg is not None else None, _stream_ptr(None))


def run_yuv(ctx, src, planes, bpc, layout, source, i, d, target, pad=None, offset=0, fg=None, what=()):
    """One mi_display_yuv_tm call into a guarded destination against the model of `planes`.
    source: (mtrx, full, chr); i: index into SETUPS; target: (mtrx, range); pad None: an
    AlignedDest (the vector stores), else Dest's pad and offset in samples."""
    h, w = planes[0].shape
    color, tm, tables = setup(i, bpc, d, *source)
    dest = AlignedDest(w, h, d, layout) if pad is None else Dest(w, h, d, layout, None, pad, offset)
    assert call_yuv(ctx, src, dest, color, tm, YuvTarget(*target), fg) == 0
    torch.cuda.synchronize()
    got = dest.planes()
    same(got, Q.semiplanar_q(planes, bpc, layout, source, tables, target, d),
         ((w, h), bpc, d, layout, source, i, target, pad, offset) + what)
    return got


# a source description per layout: (mtrx, full, chr)
SOURCES = {0: (9, 0, 0), 1: (9, 0, 2), 2: (6, 1, 0), 3: (9, 0, 1)}


@pytest.mark.parametrize("size", [(1, 1), (2, 1), (1, 2), (9, 7), (17, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_sizes_every_layout(gpu, size):
    w, h = size
    n = 0
    for layout in range(4):
        for bpc, d in ((10, 8), (8, 10)):
            rng = np.random.default_rng(w * 100 + h * 10 + layout + bpc)
            planes = planes_of(rng, w, h, bpc, layout, "random")
            src = to_frame(planes, w, h, bpc, layout)
            for chr in ((0, 2) if layout == 1 else (SOURCES[layout][2],)):
                source = SOURCES[layout][:2] + (chr,)
                run_yuv(gpu, src, planes, bpc, layout, source, PQ, d, (1, 0))
                run_yuv(gpu, src, planes, bpc, layout, source, n, d, (6, 1), pad=3, offset=1)
                n += 1
            assert unchanged(src, planes)


@pytest.mark.parametrize("layout,chr", [(1, 0), (1, 2), (2, 0), (3, 0), (0, 0)], ids=lambda v: str(v))
def test_left_neighbour_across_a_workgroup(gpu, layout, chr):
    """521 x 5: a workgroup stores 504 columns, so column 503 is the left neighbour of another
    workgroup's first run; the last run is one column wide."""
    w, h = 521, 5
    for bpc, d in ((10, 8), (12, 12)):
        rng = np.random.default_rng(layout * 10 + chr + bpc)
        planes = planes_of(rng, w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        run_yuv(gpu, src, planes, bpc, layout, (9, 0, chr), PQ, d, (1, 0))
        run_yuv(gpu, src, planes, bpc, layout, (9, 0, chr), PQ, d, (1, 0), pad=5, offset=3)


@pytest.mark.parametrize("size", [(24, 19), (24, 16), (9, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_above_across_row_units(gpu, size):
    """4:2:0 co-located: the row above a row unit is the unit above's odd row, from the wave above
    inside a block of 4 units and from another block across it (19 rows: 10 units, the last of one
    row); the centred siting beside it."""
    w, h = size
    for bpc, d in ((10, 8), (8, 8), (12, 10)):
        rng = np.random.default_rng(h + bpc)
        for kind in ("random", "blocks"):
            planes = planes_of(rng, w, h, bpc, 1, kind)
            src = to_frame(planes, w, h, bpc, 1)
            for chr in (2, 1):
                run_yuv(gpu, src, planes, bpc, 1, (9, 0, chr), PQ, d, (1, 0), what=(kind,))


@pytest.mark.parametrize("d", [8, 10, 12])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_depth_to_every_depth(gpu, bpc, d):
    w, h = 17, 9
    for layout in (1, 3):
        rng = np.random.default_rng(bpc * 16 + d + layout)
        planes = planes_of(rng, w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        for pad, offset in ((None, 0), (1, 1)):
            run_yuv(gpu, src, planes, bpc, layout, SOURCES[layout], PQ, d, (1, 0), pad, offset)
            run_yuv(gpu, src, planes, bpc, layout, SOURCES[layout], SDR709, d, (9, 1), pad, offset)


@pytest.mark.parametrize("target", [(1, 0), (1, 1), (6, 0), (6, 1), (9, 0), (9, 1)], ids=lambda t: f"mtrx{t[0]}-range{t[1]}")
def test_sitings_ranges_targets_sources(gpu, target):
    """Every siting of 4:2:0 and both source ranges under every target; the sources PQ / BT.2020,
    BT.709 / BT.709 and sRGB / P3 in turn."""
    w, h, bpc, d = 17, 9, 10, 8
    rng = np.random.default_rng(target[0] * 2 + target[1])
    planes = planes_of(rng, w, h, bpc, 1, "random")
    src = to_frame(planes, w, h, bpc, 1)
    for chr in (0, 1, 2):
        for full in (0, 1):
            for i in (PQ, SDR709, P3):
                run_yuv(gpu, src, planes, bpc, 1, (9 if i == PQ else 1, full, chr), i, d, target)
    planes = planes_of(rng, w, h, bpc, 2, "random")
    src = to_frame(planes, w, h, bpc, 2)
    run_yuv(gpu, src, planes, bpc, 2, (6, 1, 0), P3, 10, target)


def test_gbr_identity_source(gpu):
    """A 4:4:4 source with mtrx 0: G = Y, B = U, R = V in, the target's Y'CbCr out."""
    w, h = 17, 9
    for bpc, d in ((10, 8), (8, 12)):
        planes = planes_of(np.random.default_rng(bpc), w, h, bpc, 3, "random")
        src = to_frame(planes, w, h, bpc, 3)
        for i in (PQ, P3):
            run_yuv(gpu, src, planes, bpc, 3, (0, 1, 0), i, d, (1, 0))
            run_yuv(gpu, src, planes, bpc, 3, (0, 1, 0), i, d, (9, 1), pad=2, offset=1)


@pytest.mark.parametrize("kind", ["zeros", "max", "checker", "blocks"])
def test_pixel_patterns(gpu, kind):
    """All 0, all M, a checkerboard of the two (the largest step the decimation can meet) and the
    3 x 3 blocks of 0, M and H: every clip of both matrices fires."""
    w, h = 17, 9
    for layout in range(4):
        for bpc, d in ((10, 8), (12, 12), (8, 10)):
            planes = planes_of(np.random.default_rng(layout + bpc), w, h, bpc, layout, kind)
            src = to_frame(planes, w, h, bpc, layout)
            for target in ((1, 0), (9, 1)):
                run_yuv(gpu, src, planes, bpc, layout, SOURCES[layout], PQ, d, target, what=(kind,))


@pytest.mark.parametrize("d", [8, 10])
def test_destination_strides_and_offsets(gpu, d):
    """Tight and aligned (whole-vector stores), a padded stride, a pointer one sample off, both
    (sample by sample); widths that end inside a lane's run and on it."""
    bpc = 10
    for layout in (1, 2, 3, 0):
        for w, h in ((16, 6), (13, 5), (65, 4)):
            planes = planes_of(np.random.default_rng(d + layout + w), w, h, bpc, layout, "random")
            src = to_frame(planes, w, h, bpc, layout)
            for pad, offset in ((None, 0), (0, 0), (16, 0), (3, 0), (0, 1), (5, 3), (8, 8)):
                run_yuv(gpu, src, planes, bpc, layout, SOURCES[layout], PQ, d, (1, 0), pad, offset)


def test_film_grain(gpu):
    """Grain on: applied once to the source, before the tone map; the model is fed the oracle's
    grained picture, for both entries."""
    from tests.test_oracle_lr import planes_for
    w, h, bpc, d, layout = 65, 33, 10, 8, 1
    rng = np.random.default_rng(1)
    planes = planes_for(w, h, bpc, layout, rng)
    fg = make_fg_params(rng, layout)
    src = to_frame(planes, w, h, bpc, layout)
    ref = grain_reference(planes, w, h, bpc, layout, fg)
    assert not np.array_equal(ref[0], planes[0])
    data = film_grain_data(fg)
    run_yuv(gpu, src, ref, bpc, layout, (9, 0, 2), PQ, d, (1, 0), fg=data)
    color, tm, tables = setup(PQ, bpc, d, 9, 0, 2)
    q = Q.picture_q(ref, bpc, layout, (9, 0, 2), tables, (1, 0), d)
    dests = [Dest(30, 17, 8, layout), Dest(w, h, 10, layout)]
    assert call_scaled(gpu, src, dests, color, tm, YuvTarget(), fg=data) == 0
    torch.cuda.synchronize()
    same(dests[0].planes(), Z.scaled(q, d, layout, 2, (30, 17), 8), ("rung 0",))
    same(dests[1].planes(), Z.scaled(q, d, layout, 2, (w, h), 10), ("rung 1",))
    assert unchanged(src, planes)


# ---- mi_display_scaled_tm ----

RUNGS = [(16, 10), (33, 21), (40, 24)]
MITCHELL = (1.0 / 3.0, 1.0 / 3.0)
_q = {}


def source_q(layout, chr):
    """The 33 x 21 10-bit source of the scaled cases, its frame, and its Q at 8 bits (PQ / BT.2020
    to sRGB / BT.709, BT.709 limited): computed once and shared."""
    if (layout, chr) not in _q:
        w, h, bpc = 33, 21, 10
        planes = planes_of(np.random.default_rng(layout * 3 + chr), w, h, bpc, layout, "random")
        color, tm, tables = setup(PQ, bpc, 8, 9, 0, chr)
        _q[(layout, chr)] = (planes, to_frame(planes, w, h, bpc, layout), color, tm,
                             Q.picture_q(planes, bpc, layout, (9, 0, chr), tables, (1, 0), 8))
    return _q[(layout, chr)]


def model(q, layout, chr, size, obpc, crop=None, bc=None):
    if bc is None:
        return Z.scaled(q, 8, layout, chr, size, obpc, crop)
    return C.scaled(q, 8, layout, chr, size, obpc, crop, b=bc[0], c=bc[1])


@pytest.mark.parametrize("bc", [None, MITCHELL], ids=["triangle", "mitchell"])
@pytest.mark.parametrize("layout,chr", [(1, 0), (1, 2), (3, 0)], ids=["420", "420-colocated", "444"])
def test_scaled_rungs(gpu, layout, chr, bc):
    """10 -> 8 bits from 33 x 21: a downscale, 1:1 and an upscale in one call and as three calls of
    one rung, a crop with odd extents reaching the edge, rungs at 8 and at 10 bits (converted from
    d = 8); each equals the scaled model run on Q."""
    planes, src, color, tm, q = source_q(layout, chr)
    rs = None if bc is None else Resample("mitchell")
    ladder = [Dest(s[0], s[1], 8, layout, None, pad, off) for s, (pad, off) in zip(RUNGS, ((0, 0), (3, 1), (0, 0)))]
    assert call_scaled(gpu, src, ladder, color, tm, YuvTarget(), rs) == 0
    single = [Dest(s[0], s[1], 8, layout) for s in RUNGS]
    for d in single:
        assert call_scaled(gpu, src, [d], color, tm, YuvTarget(), rs) == 0
    crop = (2, 2, 31, 19)
    cropped = [Dest(16, 10, 8, layout, crop), Dest(31, 19, 10, layout, crop)]
    assert call_scaled(gpu, src, cropped, color, tm, YuvTarget(), rs) == 0
    torch.cuda.synchronize()
    for i, s in enumerate(RUNGS):
        got = ladder[i].planes()
        same(got, single[i].planes(), ("single", i))
        same(got, model(q, layout, chr, s, 8, None, bc), ("model", i))
    same(cropped[0].planes(), model(q, layout, chr, (16, 10), 8, crop, bc), ("crop",))
    same(cropped[1].planes(), model(q, layout, chr, (31, 19), 10, crop, bc), ("crop 1:1 at 10 bits",))
    assert unchanged(src, planes)


@pytest.mark.parametrize("layout,chr", [(1, 2), (1, 0), (2, 0), (3, 0), (0, 0)], ids=lambda v: str(v))
def test_one_to_one_rung_is_the_yuv_picture(gpu, layout, chr):
    """The 1:1 uncropped rung at d is mi_display_yuv_tm: the planar store into the scratch picture
    and the interleaved store are one computation."""
    for (w, h), bpc, d in (((33, 21), 10, 8), ((521, 5), 10, 10), ((24, 19), 8, 12)):
        planes = planes_of(np.random.default_rng(w + layout), w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        color, tm, tables = setup(PQ, bpc, d, 9, 0, chr)
        a, b = Dest(w, h, d, layout), Dest(w, h, d, layout)
        assert call_yuv(gpu, src, a, color, tm, YuvTarget(6, 1)) == 0
        assert call_scaled(gpu, src, [b], color, tm, YuvTarget(6, 1)) == 0
        torch.cuda.synchronize()
        want = Q.semiplanar_q(planes, bpc, layout, (9, 0, chr), tables, (6, 1), d)
        same(a.planes(), want, ("yuv", w, h, layout))
        same(b.planes(), want, ("scaled", w, h, layout))


def test_scratch_and_table_reuse_beside_the_plain_call(gpu):
    """One context of its own, calls enqueued back to back: tone-mapped calls with changing
    geometry (the scratch picture grows), depth and tone map, the same call again, and plain
    mi_display_scaled of the same source in between, whose output stays the plain model's."""
    from rav1d_amd.frame import Context
    ctx = Context(0)      # a context of its own: every scratch starts unallocated
    jobs = []
    sources = {}
    for key in ((17, 9, 10, 1), (33, 21, 10, 1), (33, 21, 8, 3)):
        planes = planes_of(np.random.default_rng(sum(key)), *key, "random")
        sources[key] = (planes, to_frame(planes, *key))
    # (source, chr, SETUPS index, dst_bpc, target, size, rung bpc; None for the tone map: plain)
    plan = [((17, 9, 10, 1), 2, PQ, 8, (1, 0), (8, 4), 8), ((17, 9, 10, 1), 2, None, None, None, (8, 4), 10),
            ((33, 21, 10, 1), 2, PQ, 8, (1, 0), (16, 10), 8), ((33, 21, 10, 1), 2, None, None, None, (16, 10), 8),
            ((33, 21, 10, 1), 2, PQ, 8, (1, 0), (16, 10), 8), ((33, 21, 10, 1), 0, PQ, 10, (9, 1), (16, 10), 8),
            ((33, 21, 8, 3), 0, P3, 12, (6, 0), (40, 24), 10), ((33, 21, 8, 3), 0, None, None, None, (40, 24), 8),
            ((17, 9, 10, 1), 2, SDR709, 8, (1, 0), (8, 4), 8), ((33, 21, 10, 1), 2, PQ, 8, (1, 0), (16, 10), 8)]
    for key, chr, i, d, target, size, obpc in plan:
        planes, src = sources[key]
        w, h, bpc, layout = key
        dest = Dest(size[0], size[1], obpc, layout)
        if i is None:
            pic, col = src.picture(), MiColorInfo(1, 1, 1, 0, chr)
            ims = (MiScaledImage * 1)(dest.im)
            assert lib().mi_display_scaled(ctx.h, ctypes.byref(pic), ims, 1, ctypes.byref(col), None, _stream_ptr(None)) == 0
            jobs.append((dest, Z.scaled(planes, bpc, layout, chr, size, obpc)))
        else:
            color, tm, tables = setup(i, bpc, d, 9 if i == PQ else 1, 0, chr)
            assert call_scaled(ctx, src, [dest], color, tm, YuvTarget(*target)) == 0
            q = Q.picture_q(planes, bpc, layout, (9 if i == PQ else 1, 0, chr), tables, target, d)
            jobs.append((dest, Z.scaled(q, d, layout, chr, size, obpc)))
    torch.cuda.synchronize()
    for n, (dest, want) in enumerate(jobs):
        same(dest.planes(), want, (n,))
    ctx.close()


def test_python_surface(gpu):
    """display_yuv into a DisplayImage, display_scaled(tonemap=) into ScaledImages (target None:
    BT.709 limited), output_colour."""
    planes, src, color, tm, q = source_q(1, 2)
    image = DisplayImage(33, 21, 10, 1, "nv12", out_bpc=8)
    assert image.y.dtype == torch.uint8 and image.uv.shape == (11, 17, 2)
    display_yuv(gpu, src, image, color, tm, YuvTarget())
    a, b = ScaledImage(16, 10, 8, 1), ScaledImage(40, 24, 10, 1)
    display_scaled(gpu, src, [a, b], color, tonemap=tm)
    c = ScaledImage(16, 10, 8, 1)
    display_scaled(gpu, src, c, color, tonemap=tm, target=YuvTarget(1, 0), resample=Resample("mitchell"))
    torch.cuda.synchronize()
    y, uv = R.semiplanar(q, 8, 1)
    got = image.numpy()
    assert np.array_equal(got[0], y) and np.array_equal(got[1], uv)
    for im, want in ((a, model(q, 1, 2, (16, 10), 8)), (b, model(q, 1, 2, (40, 24), 10)),
                     (c, model(q, 1, 2, (16, 10), 8, None, MITCHELL))):
        got = im.numpy()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert output_colour(tm, None, color.chr).astuple() == (1, 13, 1, 0, 2)
    assert output_colour(ToneMap(9, 1, 10), YuvTarget(9, 1), 0).astuple() == (9, 1, 9, 1, 0)
    with pytest.raises(ValueError):
        display_scaled(gpu, src, a, color, target=YuvTarget())
    assert tonemap_tables(tm, color, 10)[0].shape == (1024,)


def test_rejections_with_a_context(gpu):
    """The host checks hold with a live context and leave every destination byte alone."""
    planes, src, color, tm, _ = source_q(1, 2)
    y, s = Dest(33, 21, 8, 1), Dest(16, 10, 8, 1)
    hdr = MiColorInfo(9, 16, 9, 0, 2)
    cases = [(hdr, tm, YuvTarget(0, 0), EINVAL), (hdr, tm, YuvTarget(2, 0), EINVAL), (hdr, tm, YuvTarget(8, 0), EINVAL),
             (hdr, tm, YuvTarget(10, 0), EINVAL), (hdr, tm, YuvTarget(15, 0), EINVAL), (hdr, tm, YuvTarget(1, 2), EINVAL),
             (MiColorInfo(9, 18, 9, 0, 2), tm, YuvTarget(), ENOTSUP), (MiColorInfo(2, 16, 9, 0, 2), tm, YuvTarget(), EINVAL),
             (hdr, ToneMap(src_peak=0.0), YuvTarget(), EINVAL), (hdr, ToneMap(dst_trc=16), YuvTarget(), EINVAL),
             (MiColorInfo(9, 16, 2, 0, 2), tm, YuvTarget(), EINVAL)]
    for col, t, target, want in cases:
        assert call_yuv(gpu, src, y, col, t, target) == want
        assert call_scaled(gpu, src, [s], col, t, target) == want
    assert call_yuv(gpu, src, y, hdr, ToneMap(dst_bpc=10), YuvTarget()) == EINVAL      # out->bpc != dst_bpc
    pic, im = src.picture(), yuv_image(y)
    for fmt in (1, 2, 3):
        im.format = fmt
        assert lib().mi_display_yuv_tm(gpu.h, ctypes.byref(pic), ctypes.byref(im), ctypes.byref(hdr), ctypes.byref(tm),
                                       ctypes.byref(YuvTarget()), None, _stream_ptr(None)) == EINVAL
    im = yuv_image(y)
    im.data[1] = None
    assert lib().mi_display_yuv_tm(gpu.h, ctypes.byref(pic), ctypes.byref(im), ctypes.byref(hdr), ctypes.byref(tm),
                                   ctypes.byref(YuvTarget()), None, _stream_ptr(None)) == EINVAL
    for null in ("tm", "target"):
        assert lib().mi_display_yuv_tm(gpu.h, ctypes.byref(pic), ctypes.byref(yuv_image(y)), ctypes.byref(hdr),
                                       ctypes.byref(tm) if null != "tm" else None,
                                       ctypes.byref(YuvTarget()) if null != "target" else None, None, _stream_ptr(None)) == EINVAL
    bad = Dest(16, 10, 8, 1, (1, 0, 16, 10))      # an odd crop origin: mi_display_scaled's rule
    assert call_scaled(gpu, src, [bad], hdr, tm, YuvTarget()) == EINVAL
    torch.cuda.synchronize()
    assert y.untouched() and s.untouched() and bad.untouched()
    assert FILL == 0xA5
