"""Reference model of the tone-mapped YUV outputs (include/mi_av1out.h, "the picture Q":
mi_display_yuv_tm, mi_display_scaled_tm), written from the arithmetic the header states: the 14-bit
forward matrix to the target's Y'CbCr, the 2-D chroma decimation with the siting in the taps, and Q
itself on top of tests/display_ref.py's integer R'G'B' and tests/tonemap_ref.py's float32 stage. The
scaled entry is tests/scaled_ref.py (tests/cubic_ref.py with a cubic) run on Q."""
import math

import numpy as np

from tests import display_ref as R
from tests import tonemap_ref as TM

S = 14
TARGET_MATRICES = (1, 4, 5, 6, 7, 9)


def _round(v):
    return int(math.floor(v * (1 << S) + 0.5))


def scaling(rng, d):
    """(Yo, sy, sc) of range `rng` (0 limited, 1 full) at depth d."""
    md = (1 << d) - 1
    if rng:
        return 0, 1.0, 1.0
    return 16 << (d - 8), (219 << (d - 8)) / md, (224 << (d - 8)) / md


def coefficients(mtrx, rng, d):
    """((yr, yg, yb), (ur, ug, ub), (vr, vg, vb), Yo): the fixed-point forward matrix."""
    kr, kb = R.MATRICES[mtrx]
    kg = 1.0 - kr - kb
    yo, sy, sc = scaling(rng, d)
    yr, yb = _round(kr * sy), _round(kb * sy)
    yg = _round(sy) - yr - yb
    ur, ug = -_round(sc * kr / (2.0 * (1.0 - kb))), -_round(sc * kg / (2.0 * (1.0 - kb)))
    vg, vb = -_round(sc * kg / (2.0 * (1.0 - kr))), -_round(sc * kb / (2.0 * (1.0 - kr)))
    return (yr, yg, yb), (ur, ug, -(ur + ug)), (-(vg + vb), vg, vb), yo


def forward_sums(rgb, mtrx, rng, d):
    """(Y, U4, V4) before the clip: the shifted sums with their offsets, int64."""
    r, g, b = (np.asarray(rgb[c], dtype=np.int64) for c in range(3))
    ky, ku, kv, yo = coefficients(mtrx, rng, d)
    half = 1 << (S - 1)
    out = []
    for (cr, cg, cb), off in ((ky, yo), (ku, 1 << (d - 1)), (kv, 1 << (d - 1))):
        s = cr * r + cg * g + cb * b + half
        assert np.abs(s).max() < 1 << 31
        out.append((s >> S) + off)
    return out


def forward(rgb, mtrx, rng, d):
    """(3, ...) R'G'B' integers at depth d -> (Y, U4, V4), clipped to [0, Md]."""
    return [np.clip(p, 0, (1 << d) - 1) for p in forward_sums(rgb, mtrx, rng, d)]


def forward_float(rgb, mtrx, rng, d):
    """float64: the defining equations, rounded to nearest, clipped."""
    r, g, b = (np.asarray(rgb[c], dtype=np.float64) for c in range(3))
    kr, kb = R.MATRICES[mtrx]
    kg = 1.0 - kr - kb
    yo, sy, sc = scaling(rng, d)
    yl = kr * r + kg * g + kb * b
    y = sy * yl + yo
    u = sc * (b - yl) / (2.0 * (1.0 - kb)) + (1 << (d - 1))
    v = sc * (r - yl) / (2.0 * (1.0 - kr)) + (1 << (d - 1))
    return [np.clip(np.floor(p + 0.5), 0, (1 << d) - 1).astype(np.int64) for p in (y, u, v)]


def _taps(n, kind):
    """Per output index: (indices (n_out, taps), weights (taps,)) of one axis of n samples.
    kind: "cosited" (1, 2, 1) on 2i-1, 2i, 2i+1; "centred" (1, 1) on 2i, 2i+1; "none"."""
    if kind == "none":
        return np.arange(n)[:, None], np.array([1])
    o = np.arange((n + 1) >> 1)
    if kind == "cosited":
        return np.stack([np.maximum(2 * o - 1, 0), 2 * o, np.minimum(2 * o + 1, n - 1)], axis=1), np.array([1, 2, 1])
    return np.stack([2 * o, np.minimum(2 * o + 1, n - 1)], axis=1), np.array([1, 1])


def decimate(c, layout, chr):
    """A full-resolution chroma plane (h, w) at the subsampling of `layout` with siting `chr`: one
    2-D filter per output sample, rounded once."""
    c = np.asarray(c, dtype=np.int64)
    h, w = c.shape
    ix, wx = _taps(w, "cosited" if layout in (1, 2) else "none")
    iy, wy = _taps(h, ("cosited" if chr == 2 else "centred") if layout == 1 else "none")
    acc = np.zeros((iy.shape[0], ix.shape[0]), dtype=np.int64)
    for a in range(len(wy)):
        for b in range(len(wx)):
            acc += wy[a] * wx[b] * c[iy[:, a]][:, ix[:, b]]
    total = int(wy.sum() * wx.sum())
    assert total in (1, 2, 4, 8, 16)
    return (acc + total // 2) >> (total.bit_length() - 1)


def picture_q(planes, bpc, layout, color, tables, target, d):
    """Q as planes [Y] or [Y, U, V] at depth d (LSB-aligned int64). planes: the (grained) source;
    color: (mtrx, full, chr) of the source; tables: (lut_in, m, lut_out) of the stage; target:
    (mtrx, range)."""
    mtrx, full, chr = color
    rgb = TM.apply(R.to_rgb(planes, bpc, layout, mtrx, full, chr), *tables)
    y, u4, v4 = forward(rgb, target[0], target[1], d)
    if layout == 0:
        return [y]
    return [y, decimate(u4, layout, chr), decimate(v4, layout, chr)]


def semiplanar_q(planes, bpc, layout, color, tables, target, d):
    """Q as mi_display_yuv_tm stores it: (Y, UV or None), 10 / 12-bit samples MSB-aligned."""
    return R.semiplanar(picture_q(planes, bpc, layout, color, tables, target, d), d, layout)
