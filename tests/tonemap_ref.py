"""Reference model of the colour-volume stage (include/mi_av1out.h, MiToneMap), written from the
formulas the header states: tables_f64, an independent float64 evaluation of the three tables
(numpy throughout, the matrix through numpy.linalg); apply, the exact float32 stage the kernel must
reproduce bit for bit from given tables; apply_f64, the whole conversion in float64 without tables,
which bounds the tables' quantisation. The stage runs on the (3, h, w) integers of
tests/display_ref.py's to_rgb, and tests/tensor_ref.py's resize and finish run on its result."""
import numpy as np

CURVE = {1: "709", 6: "709", 14: "709", 15: "709", 13: "srgb", 16: "pq"}
# H.273 chromaticities (R, G, B), D65 white
PRIMARIES = {1: ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060)),
             5: ((0.64, 0.33), (0.29, 0.60), (0.15, 0.06)),
             6: ((0.630, 0.340), (0.310, 0.595), (0.155, 0.070)),
             7: ((0.630, 0.340), (0.310, 0.595), (0.155, 0.070)),
             9: ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046)),
             12: ((0.680, 0.320), (0.265, 0.690), (0.150, 0.060))}
WHITE = (0.3127, 0.3290)
M1, M2, C1, C2, C3 = 2610 / 16384, 2523 / 32, 3424 / 4096, 2413 / 128, 2392 / 128


def pq_inv_eotf(nits):
    y = np.power(np.asarray(nits, dtype=np.float64) / 10000.0, M1)
    return np.power((C1 + C2 * y) / (1.0 + C3 * y), M2)


def pq_eotf(e):
    p = np.power(np.asarray(e, dtype=np.float64), 1.0 / M2)
    return 10000.0 * np.power(np.maximum(p - C1, 0.0) / (C2 - C3 * p), 1.0 / M1)


def eetf(e1, max_lum):
    """The BT.2390 EETF with black level 0 on the normalised signal."""
    e1 = np.asarray(e1, dtype=np.float64)
    ks = 1.5 * max_lum - 0.5
    if ks >= 1.0:
        return e1
    t = (e1 - ks) / (1.0 - ks)
    spline = ((2 * t**3 - 3 * t**2 + 1) * ks + (t**3 - 2 * t**2 + t) * (1.0 - ks) + (-2 * t**3 + 3 * t**2) * max_lum)
    return np.where(e1 < ks, e1, spline)


def linear_f64(x, trc, src_peak=1000.0, dst_peak=100.0):
    """Linear light in [0, 1] of source code values x in [0, 1] (float64)."""
    x = np.asarray(x, dtype=np.float64)
    curve = CURVE[trc]
    if curve == "709":
        return np.where(x < 0.081, x / 4.5, np.power((x + 0.099) / 1.099, 1.0 / 0.45))
    if curve == "srgb":
        return np.where(x <= 0.04045, x / 12.92, np.power((x + 0.055) / 1.055, 2.4))
    ns, nd = float(pq_inv_eotf(src_peak)), float(pq_inv_eotf(dst_peak))
    e2 = eetf(np.minimum(x / ns, 1.0), min(nd / ns, 1.0))
    return np.minimum(pq_eotf(e2 * ns) / dst_peak, 1.0)


def oetf_f64(l, dst_trc):
    l = np.asarray(l, dtype=np.float64)
    if dst_trc == 1:
        return np.where(l < 0.018, 4.5 * l, 1.099 * np.power(l, 0.45) - 0.099)
    return np.where(l <= 0.0031308, 12.92 * l, 1.055 * np.power(l, 1.0 / 2.4) - 0.055)


def rgb_to_xyz(pri):
    p = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in PRIMARIES[pri]], dtype=np.float64).T
    w = np.array([WHITE[0] / WHITE[1], 1.0, (1.0 - WHITE[0] - WHITE[1]) / WHITE[1]])
    return p * np.linalg.solve(p, w)


def matrix_f64(pri, dst_pri):
    if pri == dst_pri:
        return np.eye(3)
    return np.linalg.solve(rgb_to_xyz(dst_pri), rgb_to_xyz(pri))


def tables_f64(pri, trc, src_bpc, dst_pri=1, dst_trc=13, dst_bpc=8, src_peak=1000.0, dst_peak=100.0):
    """(lut_in, m, lut_out) in float64, before the one rounding the library applies: lut_in the
    linear light per source code (entry 0 exactly 0, then the running maximum), m (3, 3), lut_out OETF(i / 65535) Md (the
    library stores floor(that + 0.5))."""
    ms, md = (1 << src_bpc) - 1, (1 << dst_bpc) - 1
    lut_in = linear_f64(np.arange(ms + 1) / ms, trc, src_peak, dst_peak)
    lut_in[0] = 0.0
    lut_in = np.maximum.accumulate(lut_in)      # the table never decreases (the BT.709 knee at 12 bits)
    return lut_in, matrix_f64(pri, dst_pri), oetf_f64(np.arange(65536) / 65535.0, dst_trc) * md


def apply(rgb, lut_in, m, lut_out):
    """The device stage on (3, ...) integers: float32 throughout, every operation rounded on its
    own, the index conversion truncating."""
    lut_in = np.asarray(lut_in, dtype=np.float32)
    m = np.asarray(m, dtype=np.float32).reshape(3, 3)
    rgb = np.asarray(rgb)
    r, g, b = (lut_in[np.minimum(rgb[c], len(lut_in) - 1)] for c in range(3))
    out = []
    for k in range(3):
        t = (m[k, 0] * r + m[k, 1] * g).astype(np.float32) + m[k, 2] * b
        assert t.dtype == np.float32
        t = np.minimum(np.maximum(t, np.float32(0.0)), np.float32(1.0))
        i = (t * np.float32(65535.0) + np.float32(0.5)).astype(np.float32)
        out.append(np.asarray(lut_out)[i.astype(np.int64)].astype(np.int64))
    return np.stack(out)


def apply_rgba(rgb, lut_in, m, lut_out, dst_bpc):
    """apply, as (h, w, 4) with A = 2^dst_bpc - 1."""
    o = apply(rgb, lut_in, m, lut_out)
    return np.stack([o[0], o[1], o[2], np.full(o.shape[1:], (1 << dst_bpc) - 1, dtype=np.int64)], axis=-1)


def apply_f64(rgb, src_bpc, pri, trc, dst_pri=1, dst_trc=13, dst_bpc=8, src_peak=1000.0, dst_peak=100.0):
    """The whole conversion in float64, no tables: (3, ...) destination codes."""
    ms, md = (1 << src_bpc) - 1, (1 << dst_bpc) - 1
    lin = linear_f64(np.asarray(rgb, dtype=np.float64) / ms, trc, src_peak, dst_peak)
    lin = np.where(np.asarray(rgb) == 0, 0.0, lin)
    t = np.clip(np.einsum("kc,c...->k...", matrix_f64(pri, dst_pri), lin), 0.0, 1.0)
    return np.floor(oetf_f64(t, dst_trc) * md + 0.5).astype(np.int64)
