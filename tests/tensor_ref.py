"""Reference model of the tensor output (include/mi_av1out.h, mi_display_tensor), written from the
arithmetic the header states: the integer taps of the triangle filter, the separable resize
(horizontal pass first), the finish of the four dtypes, and the whole call on top of
tests/display_ref.py's integer R'G'B' picture. A float64 triangle filter bounds the integer one."""
import numpy as np

from tests import display_ref as R

S = 18
U8, F16, BF16, F32 = 0, 1, 2, 3


def weights(n_in, n_out):
    """Per output position: (first tap index i0, [k_0, k_1, ...]); tap j reads sample
    clamp(i0 + j, 0, n_in - 1). Python integers throughout."""
    rr = 2 * max(n_in, n_out)
    out = []
    for o in range(n_out):
        c = (2 * o + 1) * n_in
        # every i with wt_i > 0 satisfies |c - (2i+1) n_out| < rr: scan a range that contains them
        lo = (c - rr) // (2 * n_out) - 2
        hi = (c + rr) // (2 * n_out) + 2
        taps = [(i, rr - abs(c - (2 * i + 1) * n_out)) for i in range(lo, hi + 1)]
        assert taps[0][1] <= 0 and taps[-1][1] <= 0
        taps = [(i, wt) for i, wt in taps if wt > 0]
        assert [i for i, _ in taps] == list(range(taps[0][0], taps[0][0] + len(taps)))
        total = sum(wt for _, wt in taps)
        k = [(wt * (1 << S) + total // 2) // total for _, wt in taps]
        wts = [wt for _, wt in taps]
        k[wts.index(max(wts))] += (1 << S) - sum(k)      # the first tap with the largest weight
        out.append((taps[0][0], k))
    return out


def resize_axis(x, n_out, axis):
    """One pass over `axis` of an integer array."""
    x = np.moveaxis(np.asarray(x, dtype=np.int64), axis, -1)
    n_in = x.shape[-1]
    out = np.empty(x.shape[:-1] + (n_out,), dtype=np.int64)
    for o, (i0, k) in enumerate(weights(n_in, n_out)):
        idx = np.clip(np.arange(i0, i0 + len(k)), 0, n_in - 1)
        out[..., o] = ((x[..., idx] * np.asarray(k, dtype=np.int64)).sum(axis=-1) + (1 << (S - 1))) >> S
    return np.moveaxis(out, -1, axis)


def resize(x, out_w, out_h):
    """(..., h, w) -> (..., out_h, out_w): the horizontal pass, then the vertical pass over its integers."""
    return resize_axis(resize_axis(x, out_w, -1), out_h, -2)


def bfloat16_bits(f):
    """float32 array -> the bfloat16 bit patterns (uint16), round to nearest-even."""
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def finish(v, bpc, dtype, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """(3, h, w) integers -> the stored elements: uint8, float16, bfloat16 as its uint16 bit
    patterns, or float32. scale and bias are rounded to float32 here."""
    v = np.asarray(v, dtype=np.int64)
    if dtype == U8:
        return (v if bpc == 8 else np.minimum(255, (v + (1 << (bpc - 9))) >> (bpc - 8))).astype(np.uint8)
    s = np.asarray(scale, dtype=np.float32).reshape(3, 1, 1)
    b = np.asarray(bias, dtype=np.float32).reshape(3, 1, 1)
    f = v.astype(np.float32) * s       # float32 product, rounded
    f = (f + b).astype(np.float32)     # float32 sum, rounded
    assert f.dtype == np.float32
    if dtype == F32:
        return f
    if dtype == F16:
        return f.astype(np.float16)
    return bfloat16_bits(f)


def scale_bias(bpc, mean=None, std=None):
    """display_tensor's scale and bias: Python floats, rounded once to float32."""
    mean = (0.0, 0.0, 0.0) if mean is None else mean
    std = (1.0, 1.0, 1.0) if std is None else std
    m = float((1 << bpc) - 1)
    return ([np.float32(1.0 / (m * float(s))) for s in std], [np.float32(-float(a) / float(s)) for a, s in zip(mean, std)])


def tensor(planes, bpc, layout, color, crop, size, dtype, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """The whole call. color: (mtrx, full range, chr); crop: (x, y, w, h) or None; size: (w, h).
    Returns the (3, h, w) stored elements (finish)."""
    mtrx, full, chr = color
    rgb = R.to_rgb(planes, bpc, layout, mtrx, full, chr)
    if crop is not None:
        x, y, w, h = crop
        rgb = rgb[:, y:y + h, x:x + w]
    return finish(resize(rgb, size[0], size[1]), bpc, dtype, scale, bias)


def triangle_float(x, n_out, axis):
    """float64 triangle filter on half-pixel centres, widened by the downscale ratio, edges clamped."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    n_in = x.shape[-1]
    ratio = max(n_in / n_out, 1.0)
    out = np.empty(x.shape[:-1] + (n_out,), dtype=np.float64)
    for o in range(n_out):
        centre = (o + 0.5) * n_in / n_out
        i = np.arange(int(np.floor(centre - ratio)) - 1, int(np.ceil(centre + ratio)) + 2)
        wt = np.maximum(0.0, 1.0 - np.abs(centre - (i + 0.5)) / ratio)
        out[..., o] = (x[..., np.clip(i, 0, n_in - 1)] * (wt / wt.sum())).sum(axis=-1)
    return np.moveaxis(out, -1, axis)
