"""Reference model of HLG sources in the colour-volume stage (include/mi_av1out.h, "HLG sources"),
written from the formulas the header states, on top of tests/tonemap_ref.py (the primaries, the
matrix in float64, the destination's OETF): tables, the five tables as the library rounds them (the scalar
transcendentals through Python's math module, one entry at a time, in double precision); gain, the
table lookup with linear interpolation on the bits of Y; apply, the exact float32 stage the kernels
must reproduce bit for bit from given tables; apply_f64, the whole conversion in float64 without
tables, which bounds the tables' quantisation."""
import math

import numpy as np

from tests.tonemap_ref import PRIMARIES, WHITE, matrix_f64, oetf_f64, rgb_to_xyz

A = 0.17883277
B = 1.0 - 4.0 * A
C = 0.5 - A * math.log(4.0 * A)
U0, U1 = 103 << 23, 127 << 23      # the float32 bits of 2^-24 and of 1.0
NODES = 1538
F32_TINY = float(np.finfo(np.float32).tiny)


def inv_oetf_branches(x):
    """(the square branch, the exponential branch before the min) of the HLG inverse OETF at x."""
    return x * x / 3.0, (math.exp((x - C) / A) + B) / 12.0


def inv_oetf(x):
    """The scene-linear signal in [0, 1] of the HLG signal x in [0, 1] (a Python float)."""
    lo, hi = inv_oetf_branches(x)
    return lo if x <= 0.5 else min(hi, 1.0)


def inv_oetf_f64(x):
    """inv_oetf over an array (numpy float64)."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x <= 0.5, x * x / 3.0, np.minimum((np.exp((x - C) / A) + B) / 12.0, 1.0))


def gamma(lw):
    """The system gamma at a nominal peak of lw nits (BT.2100-2 note 5, the extended range)."""
    return 1.2 * math.pow(1.111, math.log2(lw / 1000.0))


def nodes():
    """y_k, k = 0 .. 1537, as float32: the bit patterns min(U0 + (k << 17), U1)."""
    return np.minimum(U0 + (np.arange(NODES, dtype=np.int64) << 17), U1).astype(np.uint32).view(np.float32)


def _det3(a):
    return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
            a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))


def rgb_to_xyz_cramer(pri):
    """RGB -> XYZ of the primaries as nested Python floats, the white point's scales by Cramer's
    rule: the order of operations of the library, so that entries that cancel to nothing (1e-17)
    and the last bit of the others are the library's. tests/tonemap_ref.py's rgb_to_xyz (numpy's
    solver) is the independent evaluation; the two agree within 2^-23 after rounding."""
    p = [[x / y for x, y in PRIMARIES[pri]], [1.0, 1.0, 1.0], [(1.0 - x - y) / y for x, y in PRIMARIES[pri]]]
    w = [WHITE[0] / WHITE[1], 1.0, (1.0 - WHITE[0] - WHITE[1]) / WHITE[1]]
    det = _det3(p)
    m = [[0.0] * 3 for _ in range(3)]
    for c in range(3):
        q = [[w[r] if k == c else p[r][k] for k in range(3)] for r in range(3)]
        dc = _det3(q)
        for r in range(3):
            m[r][c] = p[r][c] * dc / det
    return m


def matrix_f32(pri, dst_pri):
    """m: float32 of inv(RGB -> XYZ of dst_pri) (RGB -> XYZ of pri) through the cofactor inverse,
    the exact identity for equal values."""
    if pri == dst_pri:
        return np.eye(3, dtype=np.float32)
    s, d = rgb_to_xyz_cramer(pri), rgb_to_xyz_cramer(dst_pri)
    det = _det3(d)
    di = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (c + 1) % 3, (c + 2) % 3, (r + 1) % 3, (r + 2) % 3
            di[r][c] = (d[r1][c1] * d[r2][c2] - d[r1][c2] * d[r2][c1]) / det
    m = [[di[r][0] * s[0][c] + di[r][1] * s[1][c] + di[r][2] * s[2][c] for c in range(3)] for r in range(3)]
    out = np.array(m, dtype=np.float64).astype(np.float32)
    assert np.abs(out.astype(np.float64) - matrix_f64(pri, dst_pri)).max() <= 2.0 ** -23
    return out


def luminance_row(pri):
    """yw: the Y row of RGB -> XYZ of the primaries, float32."""
    out = np.array(rgb_to_xyz_cramer(pri)[1], dtype=np.float64).astype(np.float32)
    assert np.abs(out.astype(np.float64) - rgb_to_xyz(pri)[1]).max() <= 2.0 ** -24
    return out


def table_in(src_bpc):
    ms = (1 << src_bpc) - 1
    vals, top = [], 0.0
    for v in range(ms + 1):
        top = 0.0 if v == 0 else max(top, inv_oetf(v / ms))
        vals.append(top)
    lut = np.array(vals, dtype=np.float64).astype(np.float32)
    lut[(lut != 0) & (np.abs(lut) < F32_TINY)] = 0.0
    return lut


def table_gain(dst_peak):
    e = gamma(float(np.float32(dst_peak))) - 1.0
    return np.array([math.pow(float(y), e) for y in nodes()], dtype=np.float64).astype(np.float32)


def tables(pri, src_bpc, dst_pri=1, dst_trc=13, dst_bpc=8, dst_peak=1000.0):
    """(lut_in float32, m float32 (3, 3), lut_out uint16, yw float32 [3], lut_gain float32 [1538])
    of an HLG source with primaries `pri` at src_bpc bits, rendered for a display of dst_peak nits."""
    md = (1 << dst_bpc) - 1
    lut_out = np.floor(oetf_f64(np.arange(65536) / 65535.0, dst_trc) * md + 0.5).astype(np.uint16)
    return (table_in(src_bpc), matrix_f32(pri, dst_pri), lut_out, luminance_row(pri),
            table_gain(dst_peak))


def gain(y, lut_gain):
    """The interpolated gain at float32 luminances y: node and fraction from the bits of y, every
    float32 operation rounded on its own."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    lut_gain = np.asarray(lut_gain, dtype=np.float32)
    u = np.clip(y.view(np.uint32).astype(np.int64), U0, U1)
    d = u - U0
    k = d >> 17
    assert k.min() >= 0 and k.max() + 1 < len(lut_gain)
    f = (d & 0x1FFFF).astype(np.float32) * np.float32(2.0 ** -17)
    g0, g1 = lut_gain[k], lut_gain[k + 1]
    out = g0 + (f * (g1 - g0))
    assert out.dtype == np.float32
    return out


def apply(rgb, lut_in, m, lut_out, yw, lut_gain):
    """The device stage on (3, ...) integers: float32 throughout, every operation rounded on its
    own, the index conversion truncating."""
    lut_in = np.asarray(lut_in, dtype=np.float32)
    m = np.asarray(m, dtype=np.float32).reshape(3, 3)
    yw = np.asarray(yw, dtype=np.float32)
    rgb = np.asarray(rgb)
    r, g, b = (lut_in[np.minimum(rgb[c], len(lut_in) - 1)] for c in range(3))
    y = (yw[0] * r + yw[1] * g).astype(np.float32) + yw[2] * b
    assert y.dtype == np.float32
    gn = gain(y, lut_gain).reshape(y.shape)
    r, g, b = r * gn, g * gn, b * gn
    out = []
    for k in range(3):
        t = (m[k, 0] * r + m[k, 1] * g).astype(np.float32) + m[k, 2] * b
        assert t.dtype == np.float32
        t = np.minimum(np.maximum(t, np.float32(0.0)), np.float32(1.0))
        i = (t * np.float32(65535.0) + np.float32(0.5)).astype(np.float32)
        out.append(np.asarray(lut_out)[i.astype(np.int64)].astype(np.int64))
    return np.stack(out)


def apply_rgba(rgb, lut_in, m, lut_out, yw, lut_gain, dst_bpc):
    """apply, as (h, w, 4) with A = 2^dst_bpc - 1."""
    o = apply(rgb, lut_in, m, lut_out, yw, lut_gain)
    return np.stack([o[0], o[1], o[2], np.full(o.shape[1:], (1 << dst_bpc) - 1, dtype=np.int64)], axis=-1)


def apply_f64(rgb, src_bpc, pri, dst_pri=1, dst_trc=13, dst_bpc=8, dst_peak=1000.0):
    """The whole conversion in float64, no tables: (3, ...) destination codes."""
    ms, md = (1 << src_bpc) - 1, (1 << dst_bpc) - 1
    lin = inv_oetf_f64(np.asarray(rgb, dtype=np.float64) / ms)
    y = np.einsum("c,c...->...", rgb_to_xyz(pri)[1], lin)
    lin = lin * np.power(np.maximum(y, 2.0 ** -60), gamma(dst_peak) - 1.0)
    t = np.clip(np.einsum("kc,c...->k...", matrix_f64(pri, dst_pri), lin), 0.0, 1.0)
    return np.floor(oetf_f64(t, dst_trc) * md + 0.5).astype(np.int64)
