"""Reference model of the scaled semi-planar output (include/mi_av1out.h, mi_display_scaled),
written from the arithmetic the header states: the integer taps of the triangle filter in both
sitings (centred: (2o+1) / (2i+1); co-sited: (4o+1) / (4i+1)), the separable resize of every plane
on its own (horizontal pass first), the depth conversion and the semi-planar packing. It builds on
tests/tensor_ref.py (the centred taps are its) and tests/display_ref.py (plane sizes, packing). A
float64 triangle filter evaluated at the same sited positions bounds the integer one."""
import numpy as np

from tests import display_ref as R
from tests import tensor_ref as T

S = T.S
CENTRED, COSITED = 2, 4


def weights(n_in, n_out, phase=CENTRED):
    """Per output position: (first tap index i0, [k_0, k_1, ...]); tap j reads sample
    clamp(i0 + j, 0, n_in - 1). Python integers throughout."""
    rr = phase * max(n_in, n_out)
    out = []
    for o in range(n_out):
        c = (phase * o + 1) * n_in
        # every i with wt_i > 0 satisfies |c - (P i + 1) n_out| < rr: scan a range that contains them
        lo = (c - rr) // (phase * n_out) - 2
        hi = (c + rr) // (phase * n_out) + 2
        taps = [(i, rr - abs(c - (phase * i + 1) * n_out)) for i in range(lo, hi + 1)]
        assert taps[0][1] <= 0 and taps[-1][1] <= 0
        taps = [(i, wt) for i, wt in taps if wt > 0]
        assert [i for i, _ in taps] == list(range(taps[0][0], taps[0][0] + len(taps)))
        total = sum(wt for _, wt in taps)
        k = [(wt * (1 << S) + total // 2) // total for _, wt in taps]
        wts = [wt for _, wt in taps]
        k[wts.index(max(wts))] += (1 << S) - sum(k)      # the first tap with the largest weight
        out.append((taps[0][0], k))
    return out


def resize_axis(x, n_out, axis, phase=CENTRED):
    """One pass over `axis` of an integer array."""
    x = np.moveaxis(np.asarray(x, dtype=np.int64), axis, -1)
    n_in = x.shape[-1]
    out = np.empty(x.shape[:-1] + (n_out,), dtype=np.int64)
    for o, (i0, k) in enumerate(weights(n_in, n_out, phase)):
        idx = np.clip(np.arange(i0, i0 + len(k)), 0, n_in - 1)
        out[..., o] = ((x[..., idx] * np.asarray(k, dtype=np.int64)).sum(axis=-1) + (1 << (S - 1))) >> S
    return np.moveaxis(out, -1, axis)


def resize_plane(x, out_w, out_h, phase_x=CENTRED, phase_y=CENTRED):
    """(h, w) -> (out_h, out_w): the horizontal pass, then the vertical pass over its integers."""
    return resize_axis(resize_axis(x, out_w, -1, phase_x), out_h, -2, phase_y)


def phases(layout, chr):
    """(phase_x, phase_y) of the chroma planes: co-sited on the horizontal axis of 4:2:0 and 4:2:2
    and on the vertical axis of 4:2:0 with chr == 2."""
    return (COSITED if layout in (1, 2) else CENTRED, COSITED if layout == 1 and chr == 2 else CENTRED)


def depth(v, s, d):
    """The vertical pass's integers at depth s as codes of depth d."""
    v = np.asarray(v, dtype=np.int64)
    if d == s:
        return v
    if d < s:
        return np.minimum((1 << d) - 1, (v + (1 << (s - d - 1))) >> (s - d))
    return v << (d - s)


def crops(w, h, layout, crop):
    """(luma crop, chroma crop) as (x, y, w, h) in samples of their planes; crop None: everything."""
    sh, sv = int(layout in (1, 2)), int(layout == 1)
    x, y, cw, ch = (0, 0, w, h) if crop is None else crop
    return (x, y, cw, ch), (x >> sh, y >> sv, (cw + sh) >> sh, (ch + sv) >> sv)


def scaled(planes, bpc, layout, chr, size, out_bpc=None, crop=None):
    """The whole call for one rung: (Y (h, w), UV (ch, cw, 2) or None) as stored (u8 codes at 8
    bits, else MSB-aligned 16-bit words). size: (w, h) luma; crop: (x, y, w, h) luma pixels."""
    out_bpc = bpc if out_bpc is None else out_bpc
    h, w = np.asarray(planes[0]).shape
    (x, y, cw, ch), (ux, uy, ucw, uch) = crops(w, h, layout, crop)
    ow, oh = size
    res = [resize_plane(np.asarray(planes[0], dtype=np.int64)[y:y + ch, x:x + cw], ow, oh)]
    if layout:
        px, py = phases(layout, chr)
        ocw, och = R.chroma_size(ow, oh, layout)
        for p in (1, 2):
            res.append(resize_plane(np.asarray(planes[p], dtype=np.int64)[uy:uy + uch, ux:ux + ucw], ocw, och, px, py))
    return R.semiplanar([depth(r, bpc, out_bpc) for r in res], out_bpc, layout)


def triangle_float(x, n_out, axis, phase=CENTRED):
    """float64 triangle filter, widened by the downscale ratio, edges clamped, with the samples of
    both grids at (i + 1 / phase) of their pitch: half-pixel centres, or a quarter for co-sited."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    n_in = x.shape[-1]
    ratio = max(n_in / n_out, 1.0)
    off = 1.0 / phase
    out = np.empty(x.shape[:-1] + (n_out,), dtype=np.float64)
    for o in range(n_out):
        centre = (o + off) * n_in / n_out
        i = np.arange(int(np.floor(centre - ratio)) - 2, int(np.ceil(centre + ratio)) + 2)
        wt = np.maximum(0.0, 1.0 - np.abs(centre - (i + off)) / ratio)
        out[..., o] = (x[..., np.clip(i, 0, n_in - 1)] * (wt / wt.sum())).sum(axis=-1)
    return np.moveaxis(out, -1, axis)
