"""Reference models of the display conversion (include/mi_av1out.h, mi_display_picture), written
from the arithmetic the header states: the integer chroma upsampler, the 14-bit fixed-point
matrix the kernel must reproduce bit for bit, a float64 model of the same conversion (the ITU
equations on the integer-upsampled chroma) that bounds the fixed-point error, and the
semi-planar re-interleave."""
import math

import numpy as np

S = 14
# Dav1dMatrixCoefficients -> (Kr, Kb)
MATRICES = {1: (0.2126, 0.0722), 4: (0.30, 0.11), 5: (0.299, 0.114), 6: (0.299, 0.114), 7: (0.212, 0.087),
            9: (0.2627, 0.0593)}


def chroma_size(w, h, layout):
    ss_hor, ss_ver = int(layout in (1, 2)), int(layout == 1)
    return (w + ss_hor) >> ss_hor, (h + ss_ver) >> ss_ver


def upsample(c, layout, chr, w, h):
    """A chroma plane (ch, cw) at luma resolution (h, w): the vertical pass gives integer rows,
    the horizontal pass runs over those rows; indices clamp."""
    c = np.asarray(c, dtype=np.int64)
    ch, cw = c.shape
    if layout == 1:
        j = np.arange(ch)
        up, dn = c[np.maximum(j - 1, 0)], c[np.minimum(j + 1, ch - 1)]
        v = np.empty((2 * ch, cw), dtype=np.int64)
        if chr == 2:      # co-located
            v[0::2] = c
            v[1::2] = (c + dn + 1) >> 1
        else:             # centred (and unknown)
            v[0::2] = (up + 3 * c + 2) >> 2
            v[1::2] = (3 * c + dn + 2) >> 2
        c = v[:h]
    if layout in (1, 2):
        i = np.arange(cw)
        right = c[:, np.minimum(i + 1, cw - 1)]
        o = np.empty((c.shape[0], 2 * cw), dtype=np.int64)
        o[:, 0::2] = c
        o[:, 1::2] = (c + right + 1) >> 1
        c = o[:, :w]
    return c


def _round(v):
    return int(math.floor(v * (1 << S) + 0.5))


def scaling(bpc, full):
    """(Yo, ky as a real, kc)"""
    m = (1 << bpc) - 1
    if full:
        return 0, 1.0, 1.0
    return 16 << (bpc - 8), m / (219 << (bpc - 8)), m / (224 << (bpc - 8))


def coefficients(mtrx, full, bpc):
    """The fixed-point (Yo, ky, crv, cbu, cgu, cgv)."""
    kr, kb = MATRICES[mtrx]
    kg = 1.0 - kr - kb
    yo, ky, kc = scaling(bpc, full)
    return (yo, (1 << S) if full else _round(ky), _round(2.0 * (1.0 - kr) * kc), _round(2.0 * (1.0 - kb) * kc),
            _round(2.0 * kb * (1.0 - kb) / kg * kc), _round(2.0 * kr * (1.0 - kr) / kg * kc))


def _planes_up(planes, layout, chr):
    y = np.asarray(planes[0], dtype=np.int64)
    h, w = y.shape
    if layout == 0:
        return y, None, None
    return y, upsample(planes[1], layout, chr, w, h), upsample(planes[2], layout, chr, w, h)


def to_rgb(planes, bpc, layout, mtrx, full, chr=0):
    """The integer model: (3, h, w) R, G, B."""
    y, u, v = _planes_up(planes, layout, chr)
    m, half = (1 << bpc) - 1, 1 << (bpc - 1)
    if mtrx == 0:
        assert layout == 3
        return np.stack([v, y, u])
    yo, ky, crv, cbu, cgu, cgv = coefficients(mtrx, full, bpc)
    luma = ky * (y - yo) + (1 << (S - 1))
    if layout == 0:
        r = g = b = luma
    else:
        cb, cr = u - half, v - half
        r, g, b = luma + crv * cr, luma - cgu * cb - cgv * cr, luma + cbu * cb
    assert max(np.abs(r).max(), np.abs(g).max(), np.abs(b).max()) < 1 << 31
    return np.stack([np.clip(p >> S, 0, m) for p in (r, g, b)])


def to_rgb_float(planes, bpc, layout, mtrx, full, chr=0):
    """float64: the ITU equations on the integer-upsampled chroma, rounded to nearest, clipped."""
    y, u, v = _planes_up(planes, layout, chr)
    m, half = (1 << bpc) - 1, 1 << (bpc - 1)
    kr, kb = MATRICES[mtrx]
    kg = 1.0 - kr - kb
    yo, ky, kc = scaling(bpc, full)
    luma = ky * (y - yo).astype(np.float64)
    if layout == 0:
        r = g = b = luma
    else:
        cb, cr = kc * (u - half), kc * (v - half)
        r = luma + 2.0 * (1.0 - kr) * cr
        b = luma + 2.0 * (1.0 - kb) * cb
        g = luma - 2.0 * kb * (1.0 - kb) / kg * cb - 2.0 * kr * (1.0 - kr) / kg * cr
    return np.stack([np.clip(np.floor(p + 0.5), 0, m).astype(np.int64) for p in (r, g, b)])


def to_rgba(planes, bpc, layout, mtrx, full, chr=0):
    """(h, w, 4) with A = 2^bpc - 1."""
    rgb = to_rgb(planes, bpc, layout, mtrx, full, chr)
    a = np.full(rgb.shape[1:], (1 << bpc) - 1, dtype=np.int64)
    return np.stack([rgb[0], rgb[1], rgb[2], a], axis=-1)


def semiplanar(planes, bpc, layout):
    """(Y, UV): Y (h, w) and UV (ch, cw, 2) at the layout's own subsampling (None for 4:0:0);
    10 / 12-bit samples MSB-aligned."""
    sh = 16 - bpc if bpc > 8 else 0
    y = np.asarray(planes[0], dtype=np.int64) << sh
    if layout == 0:
        return y, None
    return y, np.stack([np.asarray(planes[1], dtype=np.int64), np.asarray(planes[2], dtype=np.int64)], axis=-1) << sh
