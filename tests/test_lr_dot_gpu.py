"""GPU parity of loop restoration at the shapes and values where its dot-product form can go
wrong: the Wiener passes on 16-bit pair dot products (row pairs of the horizontal result, so
odd window heights; tap pairs at the coefficient corners; horizontal results at 0 and at the
clip) and the self-guided box sums on pair dot products walked without a row ring (every
parameter set, weight extremes, p = 0, z >= 255, the largest sums). Bit-exact against the
oracle on every pixel of every plane.

Frame accepts odd picture sizes (chroma rounds up), so odd widths and heights are cases here."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import lib
from rav1d_amd.frame import Frame, LrMeta, lr_frame
from rav1d_amd.synth import make_lr_meta, make_texture
from tests import oracle_lib
from tests.test_dsp_calls_gpu import _SGR, P, _o
from tests.test_lr_gpu import to_frame
from tests.test_oracle_lf import pad_planes
from tests.test_oracle_lr import planes_for

pytestmark = pytest.mark.gpu

WIENER, SGR = 2, 3
# coded ranges of the three free Wiener taps (the centre follows from them)
TAP_MIN, TAP_MAX = (-5, -23, -17), (10, 8, 46)


def dims(w, h, layout, p):
    ssh = 1 if (p and layout in (1, 2)) else 0
    ssv = 1 if (p and layout == 1) else 0
    return (w + ssh) >> ssh, (h + ssv) >> ssv


def dt(bpc):
    return np.uint8 if bpc == 8 else np.uint16


def pattern(kind, w, h, bpc, layout):
    """Planes of one synthetic content: 'cols' / 'rows' alternate 0 and bdmax by column / row,
    'checker' by both, 'max' and 'zero' are flat; a leading '~' inverts."""
    inv = (len(kind) - len(kind.lstrip("~"))) & 1
    kind = kind.lstrip("~")
    bdmax = (1 << bpc) - 1
    out = []
    for p in range(3 if layout else 1):
        pw, ph = dims(w, h, layout, p)
        y, x = np.mgrid[0:ph, 0:pw]
        on = {"cols": x & 1, "rows": y & 1, "checker": (x ^ y) & 1, "max": np.ones_like(x),
              "zero": np.zeros_like(x)}[kind]
        out.append(((on ^ inv) * bdmax).astype(dt(bpc)))
    return out


def check(gpu, c, d, w, h, bpc, layout, lr, ordered=False):
    fc, fd = to_frame(c, w, h, bpc, layout), to_frame(d, w, h, bpc, layout)
    fo = Frame(w, h, bpc, layout)
    lr_frame(gpu, fc, fd, fo, LrMeta(lr, geometry=(w, h, layout) if ordered else None))
    torch.cuda.synchronize()
    ref = oracle_lib.lr_frame(pad_planes(c, w, h, bpc, layout), pad_planes(d, w, h, bpc, layout),
                              bpc, layout, w, h, lr)
    for p in range(len(c)):
        ph, pw = c[p].shape
        got = fo.plane_np(p)
        assert np.array_equal(got, ref[p][:ph, :pw]), (f"plane {p}", np.argwhere(got != ref[p][:ph, :pw])[:4])


def meta(w, h, layout, unit_log2, sb128, seed=1, **kw):
    return make_lr_meta(w, h, layout, np.random.default_rng(seed), sb128=sb128, unit_log2=unit_log2, **kw)


def wiener_meta(w, h, layout, unit_log2, sb128, hmax, vmax):
    """Every unit Wiener, filter_h and filter_v each at the minimum or the maximum of their
    ranges; chroma 5-tap (filter[0] = 0)."""
    lr = meta(w, h, layout, unit_log2, sb128)
    u = lr["lr_mask"]["lr"]
    u["type"] = WIENER
    fh = np.broadcast_to(np.array(TAP_MAX if hmax else TAP_MIN), u["filter_h"].shape).copy()
    fv = np.broadcast_to(np.array(TAP_MAX if vmax else TAP_MIN), u["filter_v"].shape).copy()
    fh[:, :, 1:, :, 0] = 0
    fv[:, :, 1:, :, 0] = 0
    u["filter_h"], u["filter_v"] = fh, fv
    lr["lr_mask"]["lr"] = u
    return lr


def sgr_meta(w, h, layout, unit_log2, sb128, wt):
    """Every unit self-guided; unit (ux, uy) of plane p takes parameter set (4 uy + ux + 5 p) % 16,
    so a plane of 4 x 4 units holds all 16: both radii, R = 2 only and R = 1 only."""
    lr = meta(w, h, layout, unit_log2, sb128)
    u = lr["lr_mask"]["lr"]
    sby, sbx, pl, ui = np.indices(u["type"].shape)
    if unit_log2[0] == 7:      # one unit per 128 x 128 superblock (entry 0)
        idx = (4 * sby + sbx + ui + 5 * pl) % 16
    else:
        idx = ((2 * sby + (ui >> 1)) * 4 + 2 * sbx + (ui & 1) + 5 * pl) % 16
    u["type"] = SGR + idx
    s0 = np.array([s[0] for s in _SGR])[idx]
    s1 = np.array([s[1] for s in _SGR])[idx]
    # (an absent radius keeps the weight the bitstream implies for it)
    u["sgr_weights"] = np.stack([np.where(s0 == 0, 0, wt[0]), np.where(s1 == 0, 95, wt[1])], -1)
    lr["lr_mask"]["lr"] = u
    return lr


# (w, h, layout, unit_log2, sb128). Heights: 8 is one stripe without neighbours, 57 = 56 + 1,
# 58, 59 and 63 end in stripes of 2, 3 and 7 rows, 121 = 56 + 64 + 1; the 4:2:0 heights 58, 114
# and 118 end chroma in stripes of 1, 1 and 3 rows. Widths: 8, 66, 70, 72 end in tiles of 8, 2,
# 6 and 8 columns; 4:2:0 with 32-px chroma units at 66, 70, 78 leaves a 32-px tile and 1, 3, 7
# columns; 67 and 69 are odd. (With 128 x 128 superblocks a unit is 128 or more, as coded.)
SHAPES = [
    (8, 8, 0, (6, 6), 0), (8, 8, 3, (6, 6), 0),
    (66, 57, 0, (6, 6), 0), (66, 57, 3, (7, 7), 1),
    (70, 58, 1, (6, 5), 0), (72, 114, 1, (7, 6), 1), (78, 118, 1, (6, 5), 0), (66, 118, 1, (6, 5), 0),
    (72, 59, 0, (7, 7), 1), (72, 59, 3, (6, 6), 0),
    (70, 63, 0, (6, 6), 0), (70, 63, 3, (8, 8), 1), (70, 63, 2, (6, 6), 0),
    (66, 121, 0, (6, 6), 0), (72, 121, 3, (7, 7), 0), (70, 121, 2, (8, 8), 1),
    (67, 57, 0, (6, 6), 0), (69, 59, 3, (6, 6), 0), (67, 121, 1, (6, 5), 0),
]


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}l{s[2]}u{s[3][0]}{s[3][1]}sb{s[4]}")
def test_shapes_mixed_units(gpu, bpc, shape):
    """Random textures, Wiener and every kind of self-guided unit mixed."""
    w, h, layout, ul, sb128 = shape
    rng = np.random.default_rng(bpc * 131 + w * 7 + h + layout)
    c, d = planes_for(w, h, bpc, layout, rng), planes_for(w, h, bpc, layout, rng)
    check(gpu, c, d, w, h, bpc, layout, make_lr_meta(w, h, layout, rng, sb128=sb128, unit_log2=ul, p_none=0.1))


WIENER_SHAPES = [(66, 57, 0, (6, 6), 0), (70, 58, 1, (6, 5), 0), (72, 59, 3, (6, 6), 0), (8, 8, 3, (6, 6), 0),
                 (67, 121, 2, (7, 7), 1)]


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("shape", WIENER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}l{s[2]}")
def test_wiener_corners(gpu, bpc, shape):
    """Coefficient corners on 0 / bdmax stripes: with columns alternating the horizontal result
    reaches 0 and its clip (32767 at 10 and 12 bits, 8191 at 8), with rows alternating the
    vertical sum swings over its whole range; the picture across the stripe edges is inverted."""
    w, h, layout, ul, sb128 = shape
    for hmax in (0, 1):
        for vmax in (0, 1):
            lr = wiener_meta(w, h, layout, ul, sb128, hmax, vmax)
            for kind in ("cols", "rows", "~cols", "checker"):
                check(gpu, pattern(kind, w, h, bpc, layout), pattern("~" + kind, w, h, bpc, layout), w, h, bpc,
                      layout, lr)


SGR_WEIGHTS = [(-96, -32), (31, 95), (-96, 95), (31, -32)]


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("geom", [(226, 249, 3, (6, 6), 0), (226, 250, 1, (6, 5), 0), (450, 505, 0, (7, 7), 1)],
                         ids=["444", "420", "400"])
def test_sgr_all_sets_extremes(gpu, bpc, geom):
    """All 16 parameter sets in one picture, the weights at their extremes, on flat bdmax (the
    largest sums, p = 0), flat 0, and 0 / bdmax checkers (z >= 255). The pictures are the smallest
    that hold 4 x 4 units in a plane with a last tile of 2 columns and a last stripe of one row:
    226 x 249 at unit 64 (chroma unit 32 at 4:2:0), and 450 x 505 where 128 x 128 superblocks make
    the unit 128."""
    w, h, layout, ul, sb128 = geom
    for i, wt in enumerate(SGR_WEIGHTS):
        lr = sgr_meta(w, h, layout, ul, sb128, wt)
        for kind in (("max", "zero", "checker") if i == 0 else ("checker", "max")):
            check(gpu, pattern(kind, w, h, bpc, layout), pattern("~" + kind, w, h, bpc, layout), w, h, bpc,
                  layout, lr)


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("shape", [(66, 57, 3, (6, 6), 0), (70, 118, 1, (6, 5), 0), (8, 8, 0, (6, 6), 0)],
                         ids=lambda s: f"{s[0]}x{s[1]}l{s[2]}")
def test_sgr_small_shapes_extremes(gpu, bpc, shape):
    w, h, layout, ul, sb128 = shape
    for wt in SGR_WEIGHTS:
        lr = sgr_meta(w, h, layout, ul, sb128, wt)
        for kind in ("checker", "max"):
            check(gpu, pattern(kind, w, h, bpc, layout), pattern("~" + kind, w, h, bpc, layout), w, h, bpc,
                  layout, lr)


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_tile_ordered_path(gpu, layout):
    """The workgroups in mi_lr_tile_order's order: the same pixels."""
    w, h, bpc = 136, 121, 10
    rng = np.random.default_rng(0xD07 + layout)
    c, d = planes_for(w, h, bpc, layout, rng), planes_for(w, h, bpc, layout, rng)
    ul = (6, 5) if layout == 1 else (6, 6)
    check(gpu, c, d, w, h, bpc, layout, make_lr_meta(w, h, layout, rng, sb128=0, unit_log2=ul, p_none=0.1),
          ordered=True)


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("wh", [(66, 57), (70, 59), (8, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_per_call_entries(gpu, bpc, wh):
    """lr.wiener at the tap corners and lr.sgr with every parameter set through the per-call
    entries, which share the tile filters: random texture and 0 / bdmax stripes, all edges present
    and none."""
    o = _o()
    I = ctypes.c_int
    o.oracle_lr_wiener.argtypes = [ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_void_p, ctypes.c_void_p, I, I,
                                   ctypes.c_void_p, I, I]
    o.oracle_lr_wiener.restype = None
    o.oracle_lr_sgr.argtypes = [I, ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_void_p, ctypes.c_void_p, I, I,
                                ctypes.c_uint, ctypes.c_uint, I, I, I, I]
    o.oracle_lr_sgr.restype = None
    w, h = wh
    rng = np.random.default_rng(77 * bpc + w)
    bdmax = (1 << bpc) - 1
    off = 8 * 96 + 8
    stripes = ((np.arange(96) & 1) * bdmax).astype(dt(bpc))
    pics = [make_texture(rng, 96, 80, bpc), np.broadcast_to(stripes, (80, 96)).copy(),
            np.broadcast_to(stripes[:80, None], (80, 96)).copy()]
    for pic in pics:
        left = np.ascontiguousarray(pic[8:8 + h, 4:8][:, ::-1])
        lpf = np.ascontiguousarray(bdmax - pic[:8])
        for edges in (15, 0):
            for hmax in (0, 1):
                for vmax in (0, 1):
                    f = np.zeros((2, 8), np.int16)
                    for k, t in enumerate((TAP_MAX if hmax else TAP_MIN, TAP_MAX if vmax else TAP_MIN)):
                        cc = -2 * sum(t) + (128 if (k == 1 or bpc > 8) else 0)
                        f[k, :7] = [t[0], t[1], t[2], cc, t[2], t[1], t[0]]
                    ref, got = pic.copy(), pic.copy()
                    o.oracle_lr_wiener(P(ref, off), ref.strides[0], P(left), P(lpf, 8), w, h, P(f), edges, bdmax)
                    assert lib().mi_dsp_lr_wiener(P(got, off), got.strides[0], P(left), P(lpf, 8), w, h, P(f), edges,
                                                  bdmax) == 0
                    assert np.array_equal(got, ref), ("wiener", hmax, vmax, edges, np.argwhere(got != ref)[:4])
            for si, (s0, s1) in enumerate(_SGR):
                kind = (s0 != 0) + 2 * (s1 != 0) - 1
                wt0, wt1 = SGR_WEIGHTS[si % 4]
                prm = np.zeros(6, np.int16)
                prm.view(np.uint32)[:2] = [s0, s1]
                prm[4:6] = [wt0, 128 - (wt0 + wt1)]
                ref, got = pic.copy(), pic.copy()
                o.oracle_lr_sgr(kind, P(ref, off), ref.strides[0], P(left), P(lpf, 8), w, h, s0, s1, int(prm[4]),
                                int(prm[5]), edges, bdmax)
                assert lib().mi_dsp_lr_sgr(kind, P(got, off), got.strides[0], P(left), P(lpf, 8), w, h, P(prm), edges,
                                           bdmax) == 0
                assert np.array_equal(got, ref), ("sgr", si, edges, np.argwhere(got != ref)[:4])
