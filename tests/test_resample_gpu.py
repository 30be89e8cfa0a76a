"""GPU: the cubic filters of mi_display_tensor_rs and mi_display_scaled_rs (include/mi_av1out.h)
against tests/cubic_ref.py, bit for bit, in guarded destinations (tests/test_tensor_gpu.py's and
tests/test_scaled_gpu.py's: every byte outside the output still holds the fill); the triangle
through the new entries against the old ones; the tap tables of one context across filters."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (T_BF16, T_F16, T_F32, T_U8, MiResample, MiScaledImage, Resample, ScaledImage,
                               display_scaled, display_tensor)
from rav1d_amd.frame import _stream_ptr, film_grain_data
from rav1d_amd.synth import make_fg_params
from tests import cubic_ref as C
from tests import display_ref as R
from tests import scaled_ref as Z
from tests import tensor_ref as T
from tests import tonemap_ref as TM
from tests.test_display_gpu import grain_reference, make_planes
from tests.test_lr_gpu import to_frame
from tests.test_scaled_gpu import Dest as ScaledDest
from tests.test_scaled_gpu import same
from tests.test_tensor_gpu import MEAN, STD, bits
from tests.test_tensor_gpu import Dest as TensorDest

pytestmark = pytest.mark.gpu

EINVAL = -22
CATMULL, MITCHELL, SWS, KEYS75 = (0.0, 0.5), (1.0 / 3.0, 1.0 / 3.0), (0.0, 0.6), (0.0, 0.75)


def ref(x):
    return ctypes.byref(x) if x is not None else None


def cubic(bc):
    return Resample("cubic", *bc)


def tensor_call(ctx, src, im, color, rs, tm=None, fg=None):
    pic = src.picture()
    return lib().mi_display_tensor_rs(ctx.h, ctypes.byref(pic), ctypes.byref(im), ctypes.byref(color), ref(tm), ref(rs),
                                      ref(fg), _stream_ptr(None))


def scaled_call(ctx, src, dests, chr, rs, fg=None):
    pic = src.picture()
    ims = (MiScaledImage * len(dests))(*[d.im for d in dests])
    col = MiColorInfo(1, 1, 1, 0, chr)
    return lib().mi_display_scaled_rs(ctx.h, ctypes.byref(pic), ims, len(dests), ctypes.byref(col), ref(rs), ref(fg),
                                      _stream_ptr(None))


def field_planes(layout=1):
    """The 64 x 48 field of 0 / 255 (tests/cubic_ref.py) as luma, chroma of the same kind."""
    cw, ch = R.chroma_size(64, 48, layout)
    return [C.field().astype(np.uint8)] + ([C.field(cw, ch, 21 + p).astype(np.uint8) for p in range(2)] if layout else [])


def run_tensor(ctx, src, rgb, depth, color, size, bc, dtype=T_U8, order="chw", crop=None, norm=False, pad=0, offset=0,
               tm=None, fg=None):
    """One call into a guarded destination against the model of the R'G'B' picture `rgb` of
    `depth` bits (the picture the passes resize)."""
    scale, bias = T.scale_bias(depth, MEAN, STD) if norm else T.scale_bias(depth)
    d = TensorDest(size[0], size[1], dtype, order, pad, offset)
    assert tensor_call(ctx, src, d.image(depth, crop, scale, bias), color, cubic(bc), tm, fg) == 0
    torch.cuda.synchronize()
    want = bits(C.tensor(None, depth, None, (0, 0, 0), crop, size, dtype, scale, bias, bc[0], bc[1], rgb=rgb))
    got = d.elements()
    assert np.array_equal(got, want), (size, bc, dtype, order, crop, int(np.count_nonzero(got != want)),
                                       np.argwhere(got != want)[:4].tolist())
    return got


def run_scaled(ctx, src, planes, bpc, layout, chr, size, bc, obpc=None, crop=None, pad=0, offset=0, fg=None):
    obpc = bpc if obpc is None else obpc
    d = ScaledDest(size[0], size[1], obpc, layout, crop, pad, offset)
    assert scaled_call(ctx, src, [d], chr, cubic(bc), fg) == 0
    torch.cuda.synchronize()
    got = d.planes()
    same(got, C.scaled(planes, bpc, layout, chr, size, obpc, crop, bc[0], bc[1]), (size, bc, bpc, obpc, layout, chr, crop))
    return got


# ---- tensor ----
@pytest.mark.parametrize("size", [(40, 30), (96, 80)], ids=["down", "up"])
def test_tensor_field(gpu, size):
    """The 0 / 255 field, 8-bit 4:2:0, full-range so that the extremes survive the matrix: the
    horizontal pass overshoots on both sides and the clamp between the passes decides the result
    (the model without it is another picture)."""
    planes = field_planes()
    src = to_frame(planes, 64, 48, 8, 1)
    rgb = R.to_rgb(planes, 8, 1, 1, 1, 0)
    for bc in (CATMULL, MITCHELL, KEYS75):
        got = run_tensor(gpu, src, rgb, 8, MiColorInfo(1, 1, 1, 1, 0), size, bc)
        if bc == CATMULL and size == (40, 30):
            loose = np.clip(C.resize(rgb, 40, 30, 255, clamp=False), 0, 255)
            assert not np.array_equal(got, loose.astype(np.uint8))


def test_tensor_odd_crop_10bit_444(gpu):
    w, h, bpc, layout = 67, 35, 10, 3
    rng = np.random.default_rng(31)
    for kind in ("random", "blocks"):
        planes = make_planes(rng, w, h, bpc, layout, kind)
        src = to_frame(planes, w, h, bpc, layout)
        rgb = R.to_rgb(planes, bpc, layout, 9, 0, 0)
        for size in ((16, 9), (50, 40)):
            run_tensor(gpu, src, rgb, bpc, MiColorInfo(1, 1, 9, 0, 0), size, SWS, T_F16, crop=(3, 5, 41, 23), norm=True)


def test_tensor_12bit_422(gpu):
    w, h, bpc, layout = 65, 33, 12, 2
    rng = np.random.default_rng(32)
    for kind in ("random", "blocks"):
        planes = make_planes(rng, w, h, bpc, layout, kind)
        src = to_frame(planes, w, h, bpc, layout)
        rgb = R.to_rgb(planes, bpc, layout, 6, 1, 0)
        for size, bc in (((20, 11), (0.0, 1.0)), ((97, 50), CATMULL), ((65, 12), (1.0, 0.0))):
            run_tensor(gpu, src, rgb, bpc, MiColorInfo(1, 1, 6, 1, 0), size, bc, T_U8)


@pytest.mark.parametrize("src_w,out_w", [(1920, 30), (300, 1100)], ids=["down64", "up"])
def test_tensor_two_segments(gpu, src_w, out_w):
    """Rows the horizontal pass splits: 1920 -> 30 is 64:1 with 257 slots per output (28 outputs
    per segment), 300 -> 1100 has more than 1024 outputs."""
    from rav1d_amd.display import resample_plan
    assert resample_plan(cubic(CATMULL), src_w, out_w)[1] < out_w
    h, bpc, layout = 8, 8, 1
    planes = make_planes(np.random.default_rng(src_w), src_w, h, bpc, layout, "blocks")
    src = to_frame(planes, src_w, h, bpc, layout)
    rgb = R.to_rgb(planes, bpc, layout, 1, 0, 0)
    run_tensor(gpu, src, rgb, bpc, MiColorInfo(1, 1, 1, 0, 0), (out_w, 8), CATMULL)
    run_tensor(gpu, src, rgb, bpc, MiColorInfo(1, 1, 1, 0, 0), (out_w, 5), MITCHELL, T_F16, "hwc", crop=(36, 0, src_w - 50, h))


STORES = [(T_U8, "chw", 0, 0), (T_F16, "chw", 0, 0), (T_BF16, "chw", 3, 1), (T_F32, "chw", 0, 0), (T_F16, "hwc", 0, 0),
          (T_F32, (700, 150, 3), 0, 0)]


@pytest.mark.parametrize("store", STORES, ids=["u8", "f16", "bf16-unaligned", "f32", "hwc", "any-stride"])
def test_tensor_store_paths(gpu, store):
    dtype, order, pad, offset = store
    w, h, bpc, layout = 65, 33, 10, 1
    planes = make_planes(np.random.default_rng(33), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    rgb = R.to_rgb(planes, bpc, layout, 1, 0, 2)
    # (the arbitrary strides: columns 3 elements apart in rows of 150, channels 700 apart)
    size = (21, 12) if isinstance(order, str) else (20, 4)
    run_tensor(gpu, src, rgb, bpc, MiColorInfo(1, 1, 1, 0, 2), size, CATMULL, dtype, order, norm=True, pad=pad, offset=offset)


def test_tensor_tone_map(gpu):
    """PQ BT.2020 10-bit to 8-bit sRGB: the passes resize the tone-mapped picture and clamp at 255."""
    from rav1d_amd.display import ToneMap, tonemap_tables
    w, h, bpc, layout = 65, 33, 10, 1
    planes = make_planes(np.random.default_rng(34), w, h, bpc, layout, "blocks")
    src = to_frame(planes, w, h, bpc, layout)
    color, tm = MiColorInfo(9, 16, 9, 0, 2), ToneMap(1, 13, 8, 1000.0, 100.0)
    lut_in, m, lut_out = tonemap_tables(tm, color, bpc)
    rgb = TM.apply(R.to_rgb(planes, bpc, layout, 9, 0, 2), lut_in, m, lut_out)
    for size, dtype in (((20, 11), T_U8), ((97, 50), T_F16)):
        run_tensor(gpu, src, rgb, 8, color, size, CATMULL, dtype, norm=True, tm=tm)
    # the python wrapper takes both arguments
    out = torch.empty((3, 11, 20), dtype=torch.uint8, device="cuda")
    display_tensor(gpu, src, out, color, tonemap=tm, resample=Resample("catmull_rom"))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), C.tensor(None, 8, None, (0, 0, 0), None, (20, 11), T.U8, rgb=rgb))


def test_tensor_film_grain(gpu):
    from tests.test_oracle_lr import planes_for
    w, h, bpc, layout = 65, 33, 8, 1
    rng = np.random.default_rng(2)
    planes = planes_for(w, h, bpc, layout, rng)
    fg = make_fg_params(rng, layout)
    src = to_frame(planes, w, h, bpc, layout)
    rgb = R.to_rgb(grain_reference(planes, w, h, bpc, layout, fg), bpc, layout, 6, 0, 0)
    assert not np.array_equal(rgb, R.to_rgb(planes, bpc, layout, 6, 0, 0))
    run_tensor(gpu, src, rgb, bpc, MiColorInfo(1, 1, 6, 0, 0), (20, 11), MITCHELL, T_F16, "hwc", crop=(3, 5, 41, 23),
               norm=True, fg=film_grain_data(fg))
    for p in range(3):
        assert np.array_equal(src.plane_np(p), planes[p])


# ---- scaled ----
SCALED = [("420-nv12-chr0", 8, 1, 0, None), ("420-nv12-chr2", 8, 1, 2, None), ("420-p010", 10, 1, 1, None),
          ("422", 12, 2, 0, None), ("444", 10, 3, 0, None), ("400", 8, 0, 0, None),
          ("10to8", 10, 1, 2, 8), ("8to10", 8, 1, 0, 10)]


@pytest.mark.parametrize("case", SCALED, ids=[c[0] for c in SCALED])
def test_scaled(gpu, case):
    """Every subsampling and siting, the depth conversions; a downscale, an upscale and down in x
    with up in y, on random planes and on the 0 / M / half blocks that overshoot."""
    _, bpc, layout, chr, obpc = case
    w, h = 66, 34
    rng = np.random.default_rng(bpc * 10 + layout + chr)
    for kind, bc in (("random", CATMULL), ("blocks", MITCHELL), ("blocks", KEYS75)):
        planes = make_planes(rng, w, h, bpc, layout, kind)
        src = to_frame(planes, w, h, bpc, layout)
        for size in ((24, 10), (70, 40), (30, 40)):
            run_scaled(gpu, src, planes, bpc, layout, chr, size, bc, obpc)


def test_scaled_field(gpu):
    """The 0 / 255 field in NV12, both sitings of the vertical axis."""
    planes = field_planes()
    src = to_frame(planes, 64, 48, 8, 1)
    for chr in (0, 2):
        got = run_scaled(gpu, src, planes, 8, 1, chr, (40, 30), CATMULL)
        loose = np.clip(C.resize(planes[0], 40, 30, 255, clamp=False), 0, 255)
        assert not np.array_equal(got[0], loose.astype(np.uint8))


def test_scaled_even_crop_and_strides(gpu):
    w, h, bpc, layout = 66, 34, 10, 1
    planes = make_planes(np.random.default_rng(41), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    for crop, size, pad, offset in (((4, 6, 40, 22), (10, 6), 0, 0), ((4, 6, 40, 22), (64, 33), 3, 1), ((26, 12, 40, 22), (13, 5), 4, 0)):
        run_scaled(gpu, src, planes, bpc, layout, 2, size, SWS, 8, crop=crop, pad=pad, offset=offset)


def test_scaled_two_segments(gpu):
    for (w, h), out in (((1920, 4), (30, 2)), ((300, 4), (1100, 7))):
        planes = make_planes(np.random.default_rng(w), w, h, 8, 1, "blocks")
        src = to_frame(planes, w, h, 8, 1)
        run_scaled(gpu, src, planes, 8, 1, 0, out, CATMULL)


def test_scaled_ladder_equals_single_calls(gpu):
    """Three rungs of different sizes, depths and crops in one call equal three single calls and
    the model."""
    w, h, bpc, layout = 136, 70, 10, 1
    planes = make_planes(np.random.default_rng(42), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    rungs = [((68, 35), 8, None, 0, 0), ((45, 22), bpc, (8, 6, 120, 60), 3, 1), ((150, 20), 12, (100, 40, 36, 30), 0, 0)]
    rs = cubic(MITCHELL)
    ladder = [ScaledDest(s[0], s[1], obpc, layout, crop, pad, off) for s, obpc, crop, pad, off in rungs]
    assert scaled_call(gpu, src, ladder, 2, rs) == 0
    single = [ScaledDest(s[0], s[1], obpc, layout, crop, pad, off) for s, obpc, crop, pad, off in rungs]
    for d in single:
        assert scaled_call(gpu, src, [d], 2, rs) == 0
    torch.cuda.synchronize()
    for i, (s, obpc, crop, _, _) in enumerate(rungs):
        got = ladder[i].planes()
        same(got, single[i].planes(), ("single", i))
        same(got, C.scaled(planes, bpc, layout, 2, s, obpc, crop, *MITCHELL), ("model", i))


def test_scaled_image_wrapper(gpu):
    w, h, bpc, layout = 17, 9, 10, 1
    planes = make_planes(np.random.default_rng(3), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    a, b = ScaledImage(8, 4, 10, layout), ScaledImage(30, 20, 8, layout)
    display_scaled(gpu, src, [a, b], MiColorInfo(1, 1, 1, 0, 2), resample=Resample("mitchell"))
    torch.cuda.synchronize()
    for im, want in ((a, C.scaled(planes, bpc, layout, 2, (8, 4), None, None, *MITCHELL)),
                     (b, C.scaled(planes, bpc, layout, 2, (30, 20), 8, None, *MITCHELL))):
        got = im.numpy()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- triangle equivalence, identity, tables ----
def test_triangle_through_the_new_entries_is_the_old_call(gpu):
    """rs NULL and MI_RS_TRIANGLE (its b and c are not read) equal mi_display_tensor,
    mi_display_tensor_tm and mi_display_scaled bit for bit."""
    from rav1d_amd.display import ToneMap
    from tests.test_scaled_gpu import call as scaled_old
    from tests.test_tensor_gpu import call as tensor_old
    w, h, bpc, layout = 67, 35, 10, 1
    planes = make_planes(np.random.default_rng(51), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color = MiColorInfo(9, 16, 9, 0, 2)
    tm = ToneMap(1, 13, 8, 1000.0, 100.0)
    for size in ((20, 11), (97, 50), (67, 35)):
        old = TensorDest(size[0], size[1], T_F16)
        assert tensor_old(gpu, src, old.image(bpc), color) == 0
        old_tm = TensorDest(size[0], size[1], T_U8)
        pic = src.picture()
        assert lib().mi_display_tensor_tm(gpu.h, ctypes.byref(pic), ctypes.byref(old_tm.image(8)), ctypes.byref(color),
                                          ctypes.byref(tm), None, _stream_ptr(None)) == 0
        olds = ScaledDest(size[0], size[1], 8, layout)
        assert scaled_old(gpu, src, [olds], 2) == 0
        torch.cuda.synchronize()
        for rs in (None, Resample("triangle"), MiResample(0, 5.0, float("nan"))):
            d = TensorDest(size[0], size[1], T_F16)
            assert tensor_call(gpu, src, d.image(bpc), color, rs) == 0
            d_tm = TensorDest(size[0], size[1], T_U8)
            assert tensor_call(gpu, src, d_tm.image(8), color, rs, tm) == 0
            ds = ScaledDest(size[0], size[1], 8, layout)
            assert scaled_call(gpu, src, [ds], 2, rs) == 0
            torch.cuda.synchronize()
            assert np.array_equal(d.elements(), old.elements())
            assert np.array_equal(d_tm.elements(), old_tm.elements())
            same(ds.planes(), olds.planes(), (size,))


def test_unresized_axis_is_the_identity_under_mitchell(gpu):
    """B > 0 blurs, but not an axis with n_in == n_out: resizing one axis equals the model whose
    other axis is untouched, and 1:1 on both is the picture itself."""
    w, h, bpc, layout = 66, 34, 8, 1
    planes = make_planes(np.random.default_rng(52), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    got = run_scaled(gpu, src, planes, bpc, layout, 0, (w, h), MITCHELL)
    assert np.array_equal(got[0], planes[0]) and np.array_equal(got[1][..., 0], planes[1])
    got = run_scaled(gpu, src, planes, bpc, layout, 0, (40, h), MITCHELL)
    assert np.array_equal(got[0], C.resize_axis(planes[0], 40, -1, 255, b=MITCHELL[0], c=MITCHELL[1]))
    rgb = R.to_rgb(planes, bpc, layout, 1, 0, 0)
    got = run_tensor(gpu, src, rgb, bpc, MiColorInfo(1, 1, 1, 0, 0), (w, 20), MITCHELL)
    assert np.array_equal(got, C.resize_axis(rgb, 20, -2, 255, b=MITCHELL[0], c=MITCHELL[1]))
    assert np.array_equal(run_tensor(gpu, src, rgb, bpc, MiColorInfo(1, 1, 1, 0, 0), (w, h), MITCHELL), rgb)


def test_tables_follow_the_filter(gpu):
    """One context of its own, one geometry, calls enqueued back to back: triangle, (0, .5),
    (1/3, 1/3), triangle, through both outputs. The geometry never changes, so tables kept by
    geometry alone would serve the wrong filter (and with the wrong capacity). Each result equals
    its own model."""
    from rav1d_amd.frame import Context
    ctx = Context(0)
    w, h, bpc, layout, size = 66, 34, 8, 1, (24, 10)
    planes = make_planes(np.random.default_rng(53), w, h, bpc, layout, "blocks")
    src = to_frame(planes, w, h, bpc, layout)
    rgb = R.to_rgb(planes, bpc, layout, 1, 0, 2)
    color = MiColorInfo(1, 1, 1, 0, 2)
    jobs = []
    for bc in (None, CATMULL, MITCHELL, None, CATMULL):
        rs = cubic(bc) if bc else None
        t = TensorDest(size[0], size[1], T_U8)
        assert tensor_call(ctx, src, t.image(bpc), color, rs) == 0
        s = ScaledDest(size[0], size[1], bpc, layout)
        assert scaled_call(ctx, src, [s], 2, rs) == 0
        if bc:
            want = (C.tensor(None, bpc, None, (0, 0, 0), None, size, T.U8, b=bc[0], c=bc[1], rgb=rgb),
                    C.scaled(planes, bpc, layout, 2, size, None, None, *bc))
        else:
            want = (T.finish(T.resize(rgb, *size), bpc, T.U8), Z.scaled(planes, bpc, layout, 2, size))
        jobs.append((t, s, want, bc))
    torch.cuda.synchronize()
    for t, s, (want_t, want_s), bc in jobs:
        assert np.array_equal(t.elements(), want_t), bc
        same(s.planes(), want_s, (bc,))
    ctx.close()


def test_filter_arguments_with_a_context(gpu):
    """tests/test_resample_args.py's filters with a live context: a bad one is -EINVAL and writes
    nothing, a good one returns 0."""
    from tests.test_resample_args import BAD, GOOD
    w, h, bpc, layout = 32, 16, 8, 1
    planes = make_planes(np.random.default_rng(1), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color = MiColorInfo(1, 1, 1, 0, 0)
    for name, rs in BAD:
        t, s = TensorDest(8, 4, T_F16), ScaledDest(8, 4, 8, layout)
        assert tensor_call(gpu, src, t.image(bpc), color, rs) == EINVAL, name
        assert scaled_call(gpu, src, [s], 0, rs) == EINVAL, name
        torch.cuda.synchronize()
        assert t.untouched() and s.untouched(), name
    for name, rs in GOOD:
        t, s = TensorDest(8, 4, T_F16), ScaledDest(8, 4, 8, layout)
        assert tensor_call(gpu, src, t.image(bpc), color, rs) == 0, name
        assert scaled_call(gpu, src, [s], 0, rs) == 0, name
        torch.cuda.synchronize()
        assert not t.untouched() and not s.untouched(), name
