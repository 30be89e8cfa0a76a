"""Reference model of the scaled semi-planar output (include/mi_av1out.h, mi_display_scaled),
written from the arithmetic the header states: the integer taps of the triangle filter in both
sitings (centred: (2o+1) / (2i+1); co-sited: (4o+1) / (4i+1)), the separable resize of every plane
on its own (horizontal pass first), the depth conversion and the semi-planar packing. It builds on
tests/resize_ref.py (the taps, the pass over one axis, the float64 triangle filter that bounds it)
and tests/display_ref.py (plane sizes, packing)."""
import numpy as np

from tests import display_ref as R
from tests.resize_ref import CENTRED, COSITED, S, resize_axis, triangle_float, weights  # noqa: F401 (the tests call them as Z.*)


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

