"""GPU: HLG sources (include/mi_av1out.h, "HLG sources"; csrc/display.h tone_run) through the five
entries that carry the colour-volume stage, on a context of this module's own that has opted in
(mi_ctx_enable_hlg; the session's shared context never does, and keeps refusing trc 18), against
tests/hlg_ref.py's float32 model over its own tables (tests/test_hlg_args.py pins the library's
tables to them), composed with tests/display_ref.py's integer R'G'B', tests/tensor_ref.py /
tests/cubic_ref.py, tests/yuv_tm_ref.py's forward matrix and decimation and tests/scaled_ref.py:
bit for bit, in guarded destinations (every byte outside the samples still holds the fill)."""
import numpy as np
import pytest
import torch

from rav1d_amd import MiError
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import (OUT_RGB_PLANAR, OUT_RGBA_PACKED, T_F16, T_U8, ToneMap, YuvTarget, display_picture,
                               display_tensor, enable_hlg, tonemap_tables)
from rav1d_amd.frame import Context, film_grain_data
from rav1d_amd.synth import make_fg_params
from tests import display_ref as R
from tests import hlg_ref as H
from tests import scaled_ref as Z
from tests import tensor_ref as T
from tests import tonemap_ref as TM
from tests import yuv_tm_ref as Q
from tests.test_display_gpu import Dest, grain_reference, make_planes, pad_for
from tests.test_lr_gpu import to_frame
from tests.test_resample_gpu import run_tensor
from tests.test_scaled_gpu import Dest as ScaledDest
from tests.test_scaled_gpu import same
from tests.test_tensor_gpu import MEAN, STD, model
from tests.test_tensor_gpu import Dest as TensorDest
from tests.test_yuv_tm_gpu import AlignedDest, call_scaled, call_yuv, planes_of

pytestmark = pytest.mark.gpu

ENOTSUP = -95
# (source pri, dst_pri, dst_trc, dst_peak): BT.2020 to BT.709 at a gamma below 1, BT.2020 kept
# (identity m) at 1.2, BT.709-tagged HLG kept, BT.2020 to P3 at a bright display
SETUPS = [(9, 1, 13, 100.0), (9, 9, 1, 1000.0), (1, 1, 13, 100.0), (9, 12, 13, 1000.0)]
# (mtrx, full range, chr) per layout: both ranges
COLORS = {0: [(9, 0, 0)], 1: [(9, 0, 2), (9, 1, 0)], 2: [(6, 1, 0)], 3: [(9, 0, 1)]}
CATMULL = (0.0, 0.5)


@pytest.fixture(scope="module")
def hlg(gpu):
    """A context of this module's own with HLG on (`gpu`: the skip without a device)."""
    ctx = Context(0)
    enable_hlg(ctx)
    yield ctx
    ctx.close()


_tables = {}


def setup(i, src_bpc, dst_bpc, mtrx, full, chr):
    """(MiColorInfo, MiToneMap, the model's five tables) of SETUPS[i]; the tables computed once.
    src_peak is NaN: an HLG source does not read it."""
    pri, dst_pri, dst_trc, peak = SETUPS[i % len(SETUPS)]
    key = (i % len(SETUPS), src_bpc, dst_bpc)
    if key not in _tables:
        _tables[key] = H.tables(pri, src_bpc, dst_pri, dst_trc, dst_bpc, peak)
    return MiColorInfo(pri, 18, mtrx, full, chr), ToneMap(dst_pri, dst_trc, dst_bpc, float("nan"), peak), _tables[key]


def run_picture(ctx, src, planes, bpc, layout, source, i, dst_bpc, fmt, pad=0, offset=0, fg=None, what=()):
    """One mi_display_picture_tm call into a guarded destination against the model of `planes`."""
    h, w = planes[0].shape
    color, tm, tables = setup(i, bpc, dst_bpc, *source)
    rgb = R.to_rgb(planes, bpc, layout, *source)
    d = Dest(fmt, w, h, dst_bpc, layout, pad, offset)
    display_picture(ctx, src, d.im, color, fg, tonemap=tm)
    torch.cuda.synchronize()
    got = d.planes()
    what = ((w, h), bpc, dst_bpc, layout, source, i % len(SETUPS), fmt, pad, offset) + what
    if fmt == OUT_RGB_PLANAR:
        assert np.array_equal(np.stack(got), H.apply(rgb, *tables)), what
    else:
        assert np.array_equal(got[0].reshape(h, w, 4), H.apply_rgba(rgb, *tables, dst_bpc)), what


def hlg_q(planes, bpc, layout, source, tables, target, d):
    """tests/yuv_tm_ref.py's picture_q with the HLG stage."""
    rgb = H.apply(R.to_rgb(planes, bpc, layout, *source), *tables)
    y, u4, v4 = Q.forward(rgb, target[0], target[1], d)
    return [y] if layout == 0 else [y, Q.decimate(u4, layout, source[2]), Q.decimate(v4, layout, source[2])]


def run_yuv(ctx, src, planes, bpc, layout, source, i, d, target, pad=None, offset=0, fg=None):
    h, w = planes[0].shape
    color, tm, tables = setup(i, bpc, d, *source)
    dest = AlignedDest(w, h, d, layout) if pad is None else ScaledDest(w, h, d, layout, None, pad, offset)
    assert call_yuv(ctx, src, dest, color, tm, YuvTarget(*target), fg) == 0
    torch.cuda.synchronize()
    same(dest.planes(), R.semiplanar(hlg_q(planes, bpc, layout, source, tables, target, d), d, layout),
         ((w, h), bpc, d, layout, source, i % len(SETUPS), target, pad, offset))


# ---- mi_display_picture_tm ----

def small_sizes_every_layout(hlg, size):
    w, h = size
    n = 0
    for layout in range(4):
        for bpc, dst_bpc in ((10, 8), (8, 10)):
            rng = np.random.default_rng(w * 100 + h * 10 + layout + bpc)
            planes = make_planes(rng, w, h, bpc, layout, "random")
            src = to_frame(planes, w, h, bpc, layout)
            for source in COLORS[layout]:
                run_picture(hlg, src, planes, bpc, layout, source, n, dst_bpc, OUT_RGB_PLANAR)
                run_picture(hlg, src, planes, bpc, layout, source, n, dst_bpc, OUT_RGBA_PACKED)
                fmt = OUT_RGBA_PACKED if n % 2 else OUT_RGB_PLANAR
                run_picture(hlg, src, planes, bpc, layout, source, n + 1, dst_bpc, fmt, pad_for(dst_bpc, True), 2)
                n += 1


def across_workgroups(hlg, size):
    """521 x 5: past a workgroup's 512 columns (packed RGBA: the LDS hand-off of the full wave and the
    lane-by-lane path of the last 9 columns); 24 x 19: past a block's 4 row units, the last unit of
    one row for 4:2:0."""
    w, h = size
    for n, (layout, bpc, dst_bpc) in enumerate(((1, 10, 8), (3, 8, 12), (1, 12, 10))):
        planes = make_planes(np.random.default_rng(w + layout + bpc), w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        for fmt in (OUT_RGB_PLANAR, OUT_RGBA_PACKED):
            run_picture(hlg, src, planes, bpc, layout, COLORS[layout][0], n, dst_bpc, fmt)
            run_picture(hlg, src, planes, bpc, layout, COLORS[layout][0], n, dst_bpc, fmt, pad_for(dst_bpc, True), 2)


def test_picture_sizes(hlg):
    """Both RGB formats for every layout at 1 x 1, 2 x 2, 9 x 7 and 17 x 9, then across a workgroup's
    columns and a block's row units. (One test item for all sizes, as for the cases below: the
    failing case is named in the assertion's message.)"""
    for size in ((1, 1), (2, 2), (9, 7), (17, 9)):
        small_sizes_every_layout(hlg, size)
    for size in ((521, 5), (24, 19)):
        across_workgroups(hlg, size)


def every_depth_to_every_depth(hlg, bpc, dst_bpc):
    """Every setup (pri 9 -> 1, 9 -> 9, 1 -> 1, 9 -> 12; dst_peak 100 and 1000) at every depth pair,
    limited and full range."""
    w, h = 17, 9
    planes = make_planes(np.random.default_rng(bpc * 16 + dst_bpc), w, h, bpc, 1, "random")
    src = to_frame(planes, w, h, bpc, 1)
    for i in range(len(SETUPS)):
        for source in COLORS[1]:
            run_picture(hlg, src, planes, bpc, 1, source, i, dst_bpc, OUT_RGBA_PACKED if i % 2 else OUT_RGB_PLANAR)


def gbr_source(hlg):
    """A 4:4:4 source with mtrx 0 (G = Y, B = U, R = V): the planes are the stage's input as they are."""
    w, h = 17, 9
    for bpc, dst_bpc in ((10, 8), (8, 12), (12, 10)):
        planes = make_planes(np.random.default_rng(bpc), w, h, bpc, 3, "random")
        src = to_frame(planes, w, h, bpc, 3)
        for i in (0, 1):
            run_picture(hlg, src, planes, bpc, 3, (0, 1, 0), i, dst_bpc, OUT_RGB_PLANAR)
            run_picture(hlg, src, planes, bpc, 3, (0, 1, 0), i, dst_bpc, OUT_RGBA_PACKED, pad_for(dst_bpc, True), 2)


def patterns(hlg, kind):
    """All 0 (Y = 0: node 0 of the gain table), all M (white: at dst_peak 100 the gain pushes no
    channel above 1, the matrix to BT.709 does, and the clamp takes it), a checkerboard of the two
    and 3 x 3 blocks of 0, M and H (saturated colours: Y far from every channel)."""
    w, h = 17, 9
    for layout in (1, 3, 0):
        for bpc, dst_bpc in ((10, 8), (12, 12), (8, 10)):
            planes = planes_of(np.random.default_rng(layout + bpc), w, h, bpc, layout, kind)
            src = to_frame(planes, w, h, bpc, layout)
            for i in (0, 1):
                for full in (0, 1):
                    run_picture(hlg, src, planes, bpc, layout, (9, full, 0), i, dst_bpc, OUT_RGB_PLANAR, what=(kind,))


def white_is_clamped_below_gamma_one(hlg):
    """Full-range GBR white and a mid grey at dst_peak 100 (gamma 0.846, the gain above 1 for
    Y < 1) and at 1000: white is the top code at both."""
    bpc, w, h = 10, 16, 2
    planes = [np.full((h, w), v, dtype=np.uint16) for v in (1023, 1023, 1023)]
    planes[0][1], planes[1][1], planes[2][1] = 512, 512, 512
    src = to_frame(planes, w, h, bpc, 3)
    for i in (0, 1):
        color, tm, tables = setup(i, bpc, 8, 0, 1, 0)
        d = Dest(OUT_RGB_PLANAR, w, h, 8, 3)
        display_picture(hlg, src, d.im, color, tonemap=tm)
        torch.cuda.synchronize()
        out = np.stack(d.planes())
        assert np.array_equal(out, H.apply(R.to_rgb(planes, bpc, 3, 0, 1, 0), *tables))
        assert np.all(out[:, 0] == 255) and np.all((out[:, 1] > 0) & (out[:, 1] < 255))


def film_grain(hlg):
    from tests.test_oracle_lr import planes_for
    w, h, bpc, dst_bpc, layout = 65, 33, 10, 8, 1
    rng = np.random.default_rng(3)
    planes = planes_for(w, h, bpc, layout, rng)
    fg = make_fg_params(rng, layout)
    src = to_frame(planes, w, h, bpc, layout)
    ref = grain_reference(planes, w, h, bpc, layout, fg)
    assert not np.array_equal(ref[0], planes[0])
    run_picture(hlg, src, ref, bpc, layout, (9, 0, 0), 0, dst_bpc, OUT_RGB_PLANAR, fg=fg)
    run_yuv(hlg, src, ref, bpc, layout, (9, 0, 0), 0, dst_bpc, (1, 0), fg=film_grain_data(fg))


def test_picture_depths_sources_and_patterns(hlg):
    """The nine depth pairs under every setup, a GBR source, the constant, checkerboard and block
    patterns, white at both peaks, film grain (picture and YUV entries)."""
    for bpc in (8, 10, 12):
        for dst_bpc in (8, 10, 12):
            every_depth_to_every_depth(hlg, bpc, dst_bpc)
    gbr_source(hlg)
    for kind in ("zeros", "max", "checker", "blocks"):
        patterns(hlg, kind)
    white_is_clamped_below_gamma_one(hlg)
    film_grain(hlg)


# ---- mi_display_tensor_tm, mi_display_tensor_rs ----

def tensor_matches_the_model(hlg, depths, crop):
    """40 x 24 -> 16 x 8: finish(resize(crop(P))) with P the HLG picture and M = 2^dst_bpc - 1, the
    triangle through mi_display_tensor_tm and Catmull-Rom through mi_display_tensor_rs."""
    (bpc, dst_bpc), (w, h), size = depths, (40, 24), (16, 8)
    for n, layout in enumerate((1, 3)):
        planes = make_planes(np.random.default_rng(bpc + layout), w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        source = COLORS[layout][0]
        color, tm, tables = setup(n, bpc, dst_bpc, *source)
        rgb = H.apply(R.to_rgb(planes, bpc, layout, *source), *tables)
        scale, bias = T.scale_bias(dst_bpc, MEAN, STD)
        for dtype, order in ((T_F16, "chw"), (T_U8, "hwc")):
            d = TensorDest(size[0], size[1], dtype, order)
            display_tensor(hlg, src, d.image(dst_bpc, crop, scale, bias), color, tonemap=tm)
            torch.cuda.synchronize()
            assert np.array_equal(d.elements(), model(rgb, dst_bpc, size, dtype, crop, scale, bias)), (layout, dtype, order)
            run_tensor(hlg, src, rgb, dst_bpc, color, size, CATMULL, dtype, order, crop, norm=True, tm=tm)


def test_tensor_matches_the_model(hlg):
    for depths in ((10, 8), (8, 12)):
        for crop in (None, (3, 5, 33, 17)):
            tensor_matches_the_model(hlg, depths, crop)


# ---- mi_display_yuv_tm ----

def yuv_every_layout(hlg, layout, chr, size):
    """4:2:0 centred and co-located, 4:2:2, 4:4:4 and 4:0:0, to 8 and to 10 bits; 521 columns: the
    left neighbour of a workgroup's first run is another workgroup's."""
    w, h = size
    for n, (bpc, d) in enumerate(((10, 8), (10, 10), (8, 10), (12, 8))):
        planes = planes_of(np.random.default_rng(w + layout * 10 + chr + bpc + d), w, h, bpc, layout, "random")
        src = to_frame(planes, w, h, bpc, layout)
        run_yuv(hlg, src, planes, bpc, layout, (9, n & 1, chr), n, d, (1, 0))
        run_yuv(hlg, src, planes, bpc, layout, (9, n & 1, chr), n, d, (9, 1), pad=3, offset=1)


def yuv_row_above_across_row_units(hlg):
    """24 x 19 4:2:0 co-located: the row above a unit comes from the wave above, or is recomputed."""
    w, h = 24, 19
    for bpc, d in ((10, 8), (8, 10)):
        planes = planes_of(np.random.default_rng(bpc), w, h, bpc, 1, "blocks")
        src = to_frame(planes, w, h, bpc, 1)
        run_yuv(hlg, src, planes, bpc, 1, (9, 0, 2), 0, d, (1, 0))


# ---- mi_display_scaled_tm ----

def scaled_ladder(hlg):
    """Two rungs from 64 x 36 in one call: each equals the scaled model run on the HLG picture Q."""
    w, h, bpc, d, layout, chr = 64, 36, 10, 8, 1, 2
    planes = planes_of(np.random.default_rng(64), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color, tm, tables = setup(0, bpc, d, 9, 0, chr)
    q = hlg_q(planes, bpc, layout, (9, 0, chr), tables, (1, 0), d)
    rungs = [ScaledDest(32, 18, 8, layout), ScaledDest(16, 10, 10, layout, None, 3, 1)]
    assert call_scaled(hlg, src, rungs, color, tm, YuvTarget(1, 0)) == 0
    torch.cuda.synchronize()
    same(rungs[0].planes(), Z.scaled(q, d, layout, chr, (32, 18), 8), ("rung 0",))
    same(rungs[1].planes(), Z.scaled(q, d, layout, chr, (16, 10), 10), ("rung 1",))


def test_yuv_and_scaled_match_the_model(hlg):
    for size in ((17, 9), (521, 5)):
        for layout, chr in ((1, 0), (1, 2), (2, 0), (3, 0), (0, 0)):
            yuv_every_layout(hlg, layout, chr, size)
    yuv_row_above_across_row_units(hlg)
    scaled_ladder(hlg)


# ---- the context's tables and its flag ----

def test_table_keys_and_the_flag(gpu):
    """On one context of its own, back to back on one stream: HLG at dst_peak 100, at 1000 (only the
    gain table changes), a PQ call, an SDR call, HLG at 100 again, each with the picture of its own
    tables; then the flag off: trc 18 is ENOTSUP again, the refused call writes nothing, and a PQ call
    still matches; and on again."""
    ctx = Context(0)      # (`gpu`: the skip without a device; the shared context is not touched)
    enable_hlg(ctx)
    w, h, bpc, layout = 136, 70, 10, 1
    planes = make_planes(np.random.default_rng(9), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    rgb = R.to_rgb(planes, bpc, layout, 9, 0, 0)
    hlg_c, pq_c, sdr_c = MiColorInfo(9, 18, 9, 0, 0), MiColorInfo(9, 16, 9, 0, 0), MiColorInfo(9, 14, 9, 0, 0)

    def want(color, tm):
        if color.trc == 18:
            return H.apply(rgb, *H.tables(color.pri, bpc, tm.dst_pri, tm.dst_trc, tm.dst_bpc, tm.dst_peak))
        return TM.apply(rgb, *tonemap_tables(tm, color, bpc))

    calls = [(hlg_c, ToneMap(dst_peak=100.0)), (hlg_c, ToneMap(dst_peak=1000.0)), (pq_c, ToneMap()), (sdr_c, ToneMap()),
             (hlg_c, ToneMap(dst_peak=100.0)), (hlg_c, ToneMap(dst_peak=100.0, src_peak=4000.0)),
             (MiColorInfo(1, 18, 9, 0, 0), ToneMap(dst_peak=100.0)), (hlg_c, ToneMap(dst_peak=100.0, dst_bpc=10))]
    dests = []
    for color, tm in calls:
        d = Dest(OUT_RGB_PLANAR, w, h, tm.dst_bpc, layout)
        display_picture(ctx, src, d.im, color, tonemap=tm)
        dests.append(d)
    torch.cuda.synchronize()
    pictures = set()
    for n, ((color, tm), d) in enumerate(zip(calls, dests)):
        w_ = want(color, tm)
        assert np.array_equal(np.stack(d.planes()), w_), n
        pictures.add(w_.tobytes())
    assert len(pictures) == len(calls) - 2      # (HLG at 100 three times: src_peak is not read)

    enable_hlg(ctx, False)
    refused = Dest(OUT_RGB_PLANAR, w, h, 8, layout)
    with pytest.raises(MiError) as err:
        display_picture(ctx, src, refused.im, hlg_c, tonemap=ToneMap())
    assert f"{ENOTSUP}" in str(err.value)
    after = Dest(OUT_RGB_PLANAR, w, h, 8, layout)
    display_picture(ctx, src, after.im, pq_c, tonemap=ToneMap())
    torch.cuda.synchronize()
    refused.planes()
    assert all(np.all(b.cpu().numpy() == 0xA5) for b in refused.bufs), "the refused call wrote"
    assert np.array_equal(np.stack(after.planes()), want(pq_c, ToneMap()))

    enable_hlg(ctx, True)
    again = Dest(OUT_RGB_PLANAR, w, h, 8, layout)
    display_picture(ctx, src, again.im, hlg_c, tonemap=ToneMap(dst_peak=1000.0))
    torch.cuda.synchronize()
    assert np.array_equal(np.stack(again.planes()), want(hlg_c, ToneMap(dst_peak=1000.0)))
    ctx.close()


def test_a_context_that_never_opted_in_refuses(hlg):
    """Two contexts side by side: the flag is the context's own."""
    other = Context(0)
    w, h, bpc, layout = 17, 9, 10, 1
    planes = make_planes(np.random.default_rng(2), w, h, bpc, layout, "random")
    src = to_frame(planes, w, h, bpc, layout)
    color, tm, tables = setup(0, bpc, 8, 9, 0, 0)
    d = Dest(OUT_RGB_PLANAR, w, h, 8, layout)
    with pytest.raises(MiError) as err:
        display_picture(other, src, d.im, color, tonemap=tm)
    assert f"{ENOTSUP}" in str(err.value)
    y = ScaledDest(w, h, 8, layout)
    assert call_yuv(other, src, y, color, tm, YuvTarget()) == ENOTSUP
    assert call_scaled(other, src, [y], color, tm, YuvTarget()) == ENOTSUP
    t = TensorDest(8, 4, T_U8)
    with pytest.raises(MiError):
        display_tensor(other, src, t.image(8), color, tonemap=tm)
    torch.cuda.synchronize()
    d.planes()
    assert all(np.all(b.cpu().numpy() == 0xA5) for b in d.bufs) and y.untouched() and t.untouched()
    run_picture(hlg, src, planes, bpc, layout, (9, 0, 0), 0, 8, OUT_RGB_PLANAR)
    other.close()
