"""GPU: the colour-volume stage of the display outputs (include/mi_av1out.h: mi_display_picture_tm,
mi_display_tensor_tm; csrc/display.h tone_run) against tests/tonemap_ref.py's float32 model over
the library's own tables (mi_tonemap_tables; tests/test_tonemap_tables.py pins those), composed
with tests/display_ref.py's integer R'G'B' and tests/tensor_ref.py's resize and finish: bit for
bit, nothing outside the destination's samples touched, the source planes unchanged."""
import numpy as np
import pytest
import torch

from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (OUT_RGB_PLANAR, OUT_RGBA_PACKED, T_F16, T_U8, DisplayImage, ToneMap, display_picture,
                               display_tensor, tonemap_tables)
from rav1d_amd.synth import make_fg_params
from tests import display_ref as R
from tests import tensor_ref as T
from tests import tonemap_ref as TM
from tests.test_display_gpu import SIZES, Dest, grain_reference, make_planes, pad_for
from tests.test_lr_gpu import to_frame
from tests.test_tensor_gpu import Dest as TensorDest
from tests.test_tensor_gpu import MEAN, STD, model

pytestmark = pytest.mark.gpu

# (source pri, trc), (dst_pri, dst_trc), (src_peak, dst_peak): HDR10 to sRGB / BT.709 with the tone
# curve, SDR BT.2020 to BT.709, P3 sRGB widened to BT.2020, equal primaries (identity matrix), PQ
# with no compression into P3
SETUPS = [((9, 16), (1, 13), (1000.0, 100.0)), ((9, 14), (1, 1), (1000.0, 100.0)), ((12, 13), (9, 13), (1000.0, 100.0)),
          ((1, 1), (1, 13), (1000.0, 100.0)), ((9, 16), (12, 1), (600.0, 4000.0))]
# (mtrx, full range, chr) per layout: both ranges, every siting; 4:4:4 takes the identity too
COLORS = {0: [(9, 0, 0)], 1: [(9, 0, 2), (1, 1, 1)], 2: [(6, 1, 0)], 3: [(0, 1, 0), (9, 0, 1)]}

_tables = {}


def setup(i, src_bpc, dst_bpc, mtrx, full, chr):
    """(MiColorInfo, MiToneMap, the library's tables) of SETUPS[i]; the tables computed once."""
    (pri, trc), (dst_pri, dst_trc), (src_peak, dst_peak) = SETUPS[i % len(SETUPS)]
    color, tm = MiColorInfo(pri, trc, mtrx, full, chr), ToneMap(dst_pri, dst_trc, dst_bpc, src_peak, dst_peak)
    key = (i % len(SETUPS), src_bpc, dst_bpc)
    if key not in _tables:
        _tables[key] = tonemap_tables(tm, color, src_bpc)
    return color, tm, _tables[key]


def unchanged(src, planes):
    return all(np.array_equal(src.plane_np(p), planes[p]) for p in range(len(planes)))


# source depth -> destination depth: narrowing, equal, widening; u16 -> u8 and u8 -> u16 samples
DEPTHS = [(10, 8), (10, 10), (12, 8), (8, 8), (8, 12), (12, 12)]


@pytest.mark.parametrize("depths", DEPTHS, ids=lambda d: f"{d[0]}to{d[1]}")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_picture_matches_the_model(gpu, size, depths):
    (w, h), (bpc, dst_bpc) = size, depths
    rng = np.random.default_rng(w * 1000 + bpc * 10 + dst_bpc)
    n = 0
    for layout in range(4):
        for kind in ("random", "extremes"):
            planes = make_planes(rng, w, h, bpc, layout, kind)
            src = to_frame(planes, w, h, bpc, layout)
            for mtrx, full, chr in COLORS[layout]:
                color, tm, (lut_in, m, lut_out) = setup(n, bpc, dst_bpc, mtrx, full, chr)
                rgb = R.to_rgb(planes, bpc, layout, mtrx, full, chr)
                want = TM.apply(rgb, lut_in, m, lut_out)
                # aligned and tight, then 2 bytes off 16-byte alignment with a padded, odd stride;
                # which format takes which destination alternates
                for pad, offset in ((0, 0), (pad_for(dst_bpc, True), 2)):
                    fmt = OUT_RGB_PLANAR if (n + (offset > 0)) % 2 == 0 else OUT_RGBA_PACKED
                    d = Dest(fmt, w, h, dst_bpc, layout, pad, offset)
                    display_picture(gpu, src, d.im, color, tonemap=tm)
                    torch.cuda.synchronize()
                    got = d.planes()
                    what = (layout, kind, mtrx, full, chr, n % len(SETUPS), fmt, offset)
                    if fmt == OUT_RGB_PLANAR:
                        assert np.array_equal(np.stack(got), want), what
                    else:
                        rgba = TM.apply_rgba(rgb, lut_in, m, lut_out, dst_bpc)
                        assert np.array_equal(got[0].reshape(h, w, 4), rgba), what
                n += 1
            assert unchanged(src, planes)


@pytest.mark.parametrize("depths", [(10, 8), (8, 12), (12, 10)], ids=lambda d: f"{d[0]}to{d[1]}")
def test_packed_rgba_wide_rows(gpu, depths):
    """Wider than a wave's 512 columns: the LDS hand-off of packed RGBA with a destination sample
    type that is not the source's (and the lane-by-lane path beside it)."""
    bpc, dst_bpc = depths
    w, h, layout = 1100, 5, 1
    rng = np.random.default_rng(bpc + dst_bpc)
    planes = make_planes(rng, w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color, tm, (lut_in, m, lut_out) = setup(0, bpc, dst_bpc, 9, 0, 0)
    want = TM.apply_rgba(R.to_rgb(planes, bpc, layout, 9, 0, 0), lut_in, m, lut_out, dst_bpc)
    for pad, offset in ((0, 0), (16 * 3, 0), (pad_for(dst_bpc, True), 2)):
        d = Dest(OUT_RGBA_PACKED, w, h, dst_bpc, layout, pad, offset)
        display_picture(gpu, src, d.im, color, tonemap=tm)
        torch.cuda.synchronize()
        assert np.array_equal(d.planes()[0].reshape(h, w, 4), want), (pad, offset)


@pytest.mark.parametrize("depths", [(12, 12), (10, 8), (8, 10)], ids=lambda d: f"{d[0]}to{d[1]}")
def test_every_entry_of_lut_in(gpu, depths):
    """64 x 64 4:4:4 with the identity matrix: the planes are three different permutations of every
    code 0 .. Ms (tiled where Ms + 1 < 4096), so each channel reads every entry of lut_in."""
    bpc, dst_bpc = depths
    n = 1 << bpc
    rng = np.random.default_rng(bpc)
    dt = np.uint8 if bpc == 8 else np.uint16
    planes = [np.concatenate([rng.permutation(n) for _ in range(4096 // n)]).reshape(64, 64).astype(dt) for _ in range(3)]
    assert all(np.array_equal(np.unique(p), np.arange(n)) for p in planes)
    src = to_frame(planes, 64, 64, bpc, 3)
    for i in (0, 1, 2):
        color, tm, (lut_in, m, lut_out) = setup(i, bpc, dst_bpc, 0, 1, 0)
        rgb = R.to_rgb(planes, bpc, 3, 0, 1, 0)
        for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED):
            d = Dest(fmt, 64, 64, dst_bpc, 3)
            display_picture(gpu, src, d.im, color, tonemap=tm)
            torch.cuda.synchronize()
            if fmt == OUT_RGB_PLANAR:
                assert np.array_equal(np.stack(d.planes()), TM.apply(rgb, lut_in, m, lut_out)), i
            else:
                assert np.array_equal(d.planes()[0].reshape(64, 64, 4), TM.apply_rgba(rgb, lut_in, m, lut_out, dst_bpc)), i
    assert unchanged(src, planes)


# (output size, crop): a downscale, an upscale, an odd-origin crop (resized too)
RESIZES = {(65, 33): [((20, 11), None), ((97, 50), None), ((16, 9), (3, 5, 41, 23))],
           (136, 70): [((31, 17), None), ((150, 77), None), ((40, 24), (7, 11, 101, 47))]}


@pytest.mark.parametrize("depths", [(10, 8), (8, 12), (12, 10)], ids=lambda d: f"{d[0]}to{d[1]}")
@pytest.mark.parametrize("size", sorted(RESIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_tensor_matches_the_model(gpu, size, depths):
    """finish(resize(crop(P))) with P the tone-mapped picture and M = 2^dst_bpc - 1."""
    (w, h), (bpc, dst_bpc) = size, depths
    rng = np.random.default_rng(w + bpc + dst_bpc)
    n = 0
    for layout in (1, 3, 0, 2):
        planes = make_planes(rng, w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        mtrx, full, chr = COLORS[layout][-1]
        color, tm, (lut_in, m, lut_out) = setup(n, bpc, dst_bpc, mtrx, full, chr)
        rgb = TM.apply(R.to_rgb(planes, bpc, layout, mtrx, full, chr), lut_in, m, lut_out)
        for out_size, crop in RESIZES[size]:
            for order in ("chw", "hwc"):
                for dtype in (T_U8, T_F16):
                    scale, bias = T.scale_bias(dst_bpc, MEAN, STD)
                    pad, offset = (0, 0) if (n + (order == "hwc")) % 2 == 0 else (3, 1)
                    d = TensorDest(out_size[0], out_size[1], dtype, order, pad, offset)
                    display_tensor(gpu, src, d.image(dst_bpc, crop, scale, bias), color, tonemap=tm)
                    torch.cuda.synchronize()
                    want = model(rgb, dst_bpc, out_size, dtype, crop, scale, bias)
                    assert np.array_equal(d.elements(), want), (layout, out_size, crop, order, dtype, n % len(SETUPS))
        n += 1
        assert unchanged(src, planes)


def test_tensor_image_scale_follows_dst_bpc(gpu):
    """display_tensor on a torch tensor: (v / M - mean) / std with M of the output depth."""
    w, h, bpc, dst_bpc, layout = 65, 33, 10, 8, 1
    planes = make_planes(np.random.default_rng(5), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color, tm, (lut_in, m, lut_out) = setup(0, bpc, dst_bpc, 9, 0, 0)
    out = torch.empty((3, 12, 20), dtype=torch.float16, device="cuda")
    display_tensor(gpu, src, out, color, mean=MEAN, std=STD, tonemap=tm)
    torch.cuda.synchronize()
    rgb = TM.apply(R.to_rgb(planes, bpc, layout, 9, 0, 0), lut_in, m, lut_out)
    scale, bias = T.scale_bias(dst_bpc, MEAN, STD)
    assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), model(rgb, dst_bpc, (20, 12), T_F16, None, scale, bias))


@pytest.mark.parametrize("bpc,dst_bpc,layout,size,seed", [(10, 8, 1, (136, 70), 1), (8, 12, 1, (65, 33), 2), (12, 10, 3, (65, 33), 3),
                                                           (10, 10, 2, (136, 70), 4), (8, 8, 0, (136, 70), 5)])
def test_film_grain_goes_through_the_scratch_picture(gpu, bpc, dst_bpc, layout, size, seed):
    """With `fg` both entries convert the oracle's grained picture."""
    from tests.test_oracle_lr import planes_for
    w, h = size
    rng = np.random.default_rng(seed)
    planes = planes_for(w, h, bpc, layout, rng)
    fg = make_fg_params(rng, layout)
    src = to_frame(planes, w, h, bpc, layout)
    mtrx = 0 if layout == 3 else 9
    color, tm, (lut_in, m, lut_out) = setup(seed, bpc, dst_bpc, mtrx, 0, 0)
    ref = grain_reference(planes, w, h, bpc, layout, fg, int(mtrx == 0))
    rgb = R.to_rgb(ref, bpc, layout, mtrx, 0, 0)
    want = TM.apply(rgb, lut_in, m, lut_out)
    assert not np.array_equal(rgb, R.to_rgb(planes, bpc, layout, mtrx, 0, 0)), "the grain changes the picture"
    d = Dest(OUT_RGB_PLANAR, w, h, dst_bpc, layout, pad_for(dst_bpc, True), 0)
    display_picture(gpu, src, d.im, color, fg, tonemap=tm)
    t = TensorDest(33, 20, T_F16, "chw")
    display_tensor(gpu, src, t.image(dst_bpc), color, fg, tonemap=tm)
    torch.cuda.synchronize()
    assert np.array_equal(np.stack(d.planes()), want)
    assert np.array_equal(t.elements(), model(want, dst_bpc, (33, 20), T_F16))
    assert unchanged(src, planes)


def test_table_changes_back_to_back(gpu):
    """Calls with different tone maps, source descriptions and depths on one stream with no
    synchronise in between: each gets the picture of its own tables (a table upload is ordered
    behind the kernels that still read the old tables, and its staging buffer is not rewritten
    under an upload in flight), a repeated description reuses the tables on the device."""
    from rav1d_amd.frame import Context
    ctx = Context(0)      # a context of its own: the tables start unallocated
    w, h, layout = 136, 70, 1
    rng = np.random.default_rng(9)
    sources = {bpc: make_planes(rng, w, h, bpc, layout, "random") for bpc in (10, 8)}
    frames = {bpc: to_frame(p, w, h, bpc, layout) for bpc, p in sources.items()}
    # (source bpc, pri, trc, ToneMap): peaks, OETF, primaries, depth and source change in turn
    calls = [(10, 9, 16, ToneMap()), (10, 9, 16, ToneMap(dst_peak=300.0)), (10, 9, 16, ToneMap()),
             (10, 9, 16, ToneMap()), (10, 9, 16, ToneMap(dst_trc=1)), (10, 9, 16, ToneMap(dst_pri=12)),
             (10, 9, 16, ToneMap(dst_bpc=10)), (10, 9, 14, ToneMap(dst_bpc=10)), (8, 9, 14, ToneMap(dst_bpc=10)),
             (8, 1, 13, ToneMap(dst_pri=9)), (10, 9, 16, ToneMap(src_peak=4000.0))]
    dests = []
    for bpc, pri, trc, tm in calls:
        d = Dest(OUT_RGB_PLANAR, w, h, tm.dst_bpc, layout)
        display_picture(ctx, frames[bpc], d.im, MiColorInfo(pri, trc, 9, 0, 0), tonemap=tm)
        dests.append(d)
    # the tensor entry shares the context's tables
    t = TensorDest(31, 17, T_U8)
    display_tensor(ctx, frames[10], t.image(8), MiColorInfo(9, 16, 9, 0, 0), tonemap=ToneMap())
    torch.cuda.synchronize()
    pictures = set()
    for (bpc, pri, trc, tm), d in zip(calls, dests):
        lut_in, m, lut_out = tonemap_tables(tm, MiColorInfo(pri, trc, 9, 0, 0), bpc)
        want = TM.apply(R.to_rgb(sources[bpc], bpc, layout, 9, 0, 0), lut_in, m, lut_out)
        assert np.array_equal(np.stack(d.planes()), want), (bpc, pri, trc)
        pictures.add(want.tobytes())
    assert len(pictures) == len(calls) - 2      # (the first description is used three times)
    lut_in, m, lut_out = tonemap_tables(ToneMap(), MiColorInfo(9, 16, 9, 0, 0), 10)
    want = TM.apply(R.to_rgb(sources[10], 10, layout, 9, 0, 0), lut_in, m, lut_out)
    assert np.array_equal(t.elements(), model(want, 8, (31, 17), T_U8))
    ctx.close()


def test_plain_entries_are_unchanged_beside_the_stage(gpu):
    """mi_display_picture and mi_display_tensor before, between and after tone-mapped calls on the
    same context: the integer models of their own, as before."""
    w, h, bpc, layout = 136, 70, 10, 1
    planes = make_planes(np.random.default_rng(21), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color, tm, (lut_in, m, lut_out) = setup(0, bpc, 8, 9, 0, 0)
    rgb = R.to_rgb(planes, bpc, layout, 9, 0, 0)
    for _ in range(2):
        plain, plain_a = DisplayImage(w, h, bpc, layout, "rgb"), DisplayImage(w, h, bpc, layout, "rgba")
        mapped = DisplayImage(w, h, bpc, layout, "rgba", out_bpc=8)
        assert mapped.rgba.dtype == torch.uint8 and mapped.bpc == 8
        display_picture(gpu, src, plain, color)
        display_picture(gpu, src, mapped, color, tonemap=tm)
        display_picture(gpu, src, plain_a, color)
        t_plain, t_mapped = TensorDest(31, 17, T_F16), TensorDest(31, 17, T_F16)
        display_tensor(gpu, src, t_plain.image(bpc), color)
        display_tensor(gpu, src, t_mapped.image(8), color, tonemap=tm)
        torch.cuda.synchronize()
        assert np.array_equal(plain.numpy()[0], rgb)
        assert np.array_equal(plain_a.numpy()[0], R.to_rgba(planes, bpc, layout, 9, 0, 0))
        assert np.array_equal(mapped.numpy()[0], TM.apply_rgba(rgb, lut_in, m, lut_out, 8))
        assert np.array_equal(t_plain.elements(), model(rgb, bpc, (31, 17), T_F16))
        assert np.array_equal(t_mapped.elements(), model(TM.apply(rgb, lut_in, m, lut_out), 8, (31, 17), T_F16))


def test_rejections_with_a_context(gpu):
    """The host checks hold with a live context too, and leave the destination alone."""
    from rav1d_amd import MiError
    src = to_frame(make_planes(np.random.default_rng(1), 17, 9, 10, 1, "random"), 17, 9, 10, 1)
    d = Dest(OUT_RGB_PLANAR, 17, 9, 8, 1)
    for color, tm in ((MiColorInfo(2, 16, 9, 0, 0), ToneMap()), (MiColorInfo(9, 18, 9, 0, 0), ToneMap()),
                      (MiColorInfo(9, 16, 9, 0, 0), ToneMap(dst_bpc=10)), (MiColorInfo(9, 16, 9, 0, 0), ToneMap(src_peak=0.0))):
        with pytest.raises(MiError):
            display_picture(gpu, src, d.im, color, tonemap=tm)
    torch.cuda.synchronize()
    d.planes()
    assert all(np.all(b.cpu().numpy() == 0xA5) for b in d.bufs)
