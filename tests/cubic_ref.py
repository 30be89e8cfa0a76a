"""Reference model of the cubic resampling filters of the tensor and scaled outputs
(include/mi_av1out.h, MI_RS_CUBIC), written from the arithmetic the header states: the taps of a
Mitchell-Netravali (B, C) in both sitings, in Python integers and floats (a Python float is an IEEE
double and every operation on one is rounded on its own, which is the header's rule), and one pass
over an axis with the clamp. A float64 filter of the same shape (clamp between the passes, no
rounding) bounds the integer one. What surrounds the resize (the upsampler, the matrix, the tone
stage, the finish, the depth conversion, the siting per plane axis) is composed from
tests/tensor_ref.py and tests/scaled_ref.py, which stay as they are."""
import math

import numpy as np

from tests import display_ref as R
from tests import scaled_ref as Z
from tests import tensor_ref as T

S = 18
ONE = 1 << S
CENTRED, COSITED = 2, 4

# the (B, C) pairs the tests run: Catmull-Rom, Mitchell, swscale's bicubic, Keys -0.75, and the two
# corners of [0, 1]^2 with the most and the least negative lobes
BC = [(0.0, 0.5), (1.0 / 3.0, 1.0 / 3.0), (0.0, 0.6), (0.0, 0.75), (0.0, 1.0), (1.0, 0.0)]


def f32(x):
    """x as the float32 member of MiResample holds it, widened back to a double."""
    return float(np.float32(x))


def kernel6(d, rr, b, c):
    """w of the header: six times the (b, c) cubic at t = d / rr, Horner, left to right."""
    t = d / rr
    if d < rr:
        p3 = 12.0 - 9.0 * b - 6.0 * c
        p2 = -18.0 + 12.0 * b + 6.0 * c
        p1 = 0.0
        p0 = 6.0 - 2.0 * b
    else:
        p3 = -b - 6.0 * c
        p2 = 6.0 * b + 30.0 * c
        p1 = -12.0 * b - 48.0 * c
        p0 = 8.0 * b + 24.0 * c
    return ((p3 * t + p2) * t + p1) * t + p0


def weights(n_in, n_out, phase=CENTRED, b=0.0, c=0.5):
    """Per output position: (first tap index i0, [k_0, k_1, ...]); tap j reads sample
    clamp(i0 + j, 0, n_in - 1)."""
    if n_in == n_out:
        return [(o, [ONE]) for o in range(n_out)]
    b, c = f32(b), f32(c)
    rr = phase * max(n_in, n_out)
    out = []
    for o in range(n_out):
        cc = (phase * o + 1) * n_in
        lo = (cc - 2 * rr) // (phase * n_out) - 2
        hi = (cc + 2 * rr) // (phase * n_out) + 2
        dist = [(i, abs(cc - (phase * i + 1) * n_out)) for i in range(lo, hi + 1)]
        assert dist[0][1] >= 2 * rr and dist[-1][1] >= 2 * rr
        taps = [(i, d) for i, d in dist if d < 2 * rr]
        assert [i for i, _ in taps] == list(range(taps[0][0], taps[0][0] + len(taps)))
        assert len(taps) <= 4 * -(-max(n_in, n_out) // n_out) + 1
        w = [kernel6(d, rr, b, c) for _, d in taps]
        total = 0.0
        for v in w:                       # ascending i
            total = total + v
        k = [math.floor(v / total * 262144.0 + 0.5) for v in w]
        k[w.index(max(w))] += ONE - sum(k)    # the first tap with the largest weight
        out.append((taps[0][0], k))
    return out


def table(n_in, n_out, phase, b, c, cap):
    """The table mi_resample_taps gives: (start [n_out], count [n_out], k [cap, n_out])."""
    start = np.zeros(n_out, dtype=np.int32)
    count = np.zeros(n_out, dtype=np.int32)
    k = np.zeros((cap, n_out), dtype=np.int32)
    for o, (i0, ks) in enumerate(weights(n_in, n_out, phase, b, c)):
        start[o], count[o] = i0, len(ks)
        k[:len(ks), o] = ks
    return start, count, k


def resize_axis(x, n_out, axis, maxv, phase=CENTRED, b=0.0, c=0.5, clamp=True):
    """One pass over `axis` of an integer array: the signed sum, the arithmetic shift, the clamp to
    [0, maxv] (clamp=False leaves it out: what the clamp test compares with)."""
    x = np.moveaxis(np.asarray(x, dtype=np.int64), axis, -1)
    n_in = x.shape[-1]
    out = np.empty(x.shape[:-1] + (n_out,), dtype=np.int64)
    for o, (i0, k) in enumerate(weights(n_in, n_out, phase, b, c)):
        idx = np.clip(np.arange(i0, i0 + len(k)), 0, n_in - 1)
        out[..., o] = ((x[..., idx] * np.asarray(k, dtype=np.int64)).sum(axis=-1) + (1 << (S - 1))) >> S
    if clamp:
        out = np.clip(out, 0, maxv)
    return np.moveaxis(out, -1, axis)


def resize(x, out_w, out_h, maxv, phase_x=CENTRED, phase_y=CENTRED, b=0.0, c=0.5, clamp=True):
    """(..., h, w) -> (..., out_h, out_w): the horizontal pass, then the vertical pass over its
    clamped integers."""
    return resize_axis(resize_axis(x, out_w, -1, maxv, phase_x, b, c, clamp), out_h, -2, maxv, phase_y, b, c, clamp)


def cubic_float(x, n_out, axis, maxv, phase=CENTRED, b=0.0, c=0.5):
    """float64 filter of the same shape: the (b, c) cubic widened by the downscale ratio, edges
    clamped, samples of both grids at (i + 1 / phase) of their pitch, weights normalised, the
    result clamped to [0, maxv] and not rounded."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    n_in = x.shape[-1]
    if n_in == n_out:
        return np.moveaxis(x.copy(), -1, axis)
    b, c = f32(b), f32(c)
    ratio = max(n_in / n_out, 1.0)
    off = 1.0 / phase
    out = np.empty(x.shape[:-1] + (n_out,), dtype=np.float64)
    for o in range(n_out):
        centre = (o + off) * n_in / n_out
        i = np.arange(int(np.floor(centre - 2 * ratio)) - 2, int(np.ceil(centre + 2 * ratio)) + 2)
        t = np.abs(centre - (i + off)) / ratio
        near = (12 - 9 * b - 6 * c) * t ** 3 + (-18 + 12 * b + 6 * c) * t ** 2 + (6 - 2 * b)
        far = (-b - 6 * c) * t ** 3 + (6 * b + 30 * c) * t ** 2 + (-12 * b - 48 * c) * t + (8 * b + 24 * c)
        wt = np.where(t < 1, near, np.where(t < 2, far, 0.0))
        out[..., o] = (x[..., np.clip(i, 0, n_in - 1)] * (wt / wt.sum())).sum(axis=-1)
    return np.moveaxis(np.clip(out, 0.0, float(maxv)), -1, axis)


def float_bound(n_in, n_out, phase, b, c, maxv):
    """(e, A) of one pass: its rounding error against the float64 filter is at most
    e = 0.5 + n_taps 2^-19 M (the shift's half, and half a unit of 2^-18 per tap times a sample of at
    most M; the clamp never widens a distance), and an error of its input grows by at most
    A = max sum |k| / 2^18. Two passes: e_v + A_v e_h."""
    ws = weights(n_in, n_out, phase, b, c)
    n = max(len(k) for _, k in ws)
    return 0.5 + n * 2.0 ** -19 * maxv, max(sum(abs(v) for v in k) for _, k in ws) / ONE


# ---- the calls ----
def tensor(planes, bpc, layout, color, crop, size, dtype, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0), b=0.0, c=0.5,
           rgb=None, out_bpc=None):
    """mi_display_tensor_rs with MI_RS_CUBIC: tests/tensor_ref.py's call with the cubic resize.
    rgb: the (3, h, w) picture the passes resize when it is not display_ref's (a tone-mapped one,
    with out_bpc its depth)."""
    mtrx, full, chr = color
    if rgb is None:
        rgb = R.to_rgb(planes, bpc, layout, mtrx, full, chr)
    depth = bpc if out_bpc is None else out_bpc
    if crop is not None:
        x, y, w, h = crop
        rgb = rgb[:, y:y + h, x:x + w]
    return T.finish(resize(rgb, size[0], size[1], (1 << depth) - 1, b=b, c=c), depth, dtype, scale, bias)


def scaled(planes, bpc, layout, chr, size, out_bpc=None, crop=None, b=0.0, c=0.5):
    """mi_display_scaled_rs with MI_RS_CUBIC for one rung: tests/scaled_ref.py's call with the
    cubic resize."""
    out_bpc = bpc if out_bpc is None else out_bpc
    h, w = np.asarray(planes[0]).shape
    (x, y, cw, ch), (ux, uy, ucw, uch) = Z.crops(w, h, layout, crop)
    ow, oh = size
    ms = (1 << bpc) - 1
    res = [resize(np.asarray(planes[0], dtype=np.int64)[y:y + ch, x:x + cw], ow, oh, ms, b=b, c=c)]
    if layout:
        px, py = Z.phases(layout, chr)
        ocw, och = R.chroma_size(ow, oh, layout)
        for p in (1, 2):
            res.append(resize(np.asarray(planes[p], dtype=np.int64)[uy:uy + uch, ux:ux + ucw], ocw, och, ms, px, py, b, c))
    return R.semiplanar([Z.depth(r, bpc, out_bpc) for r in res], out_bpc, layout)


def field(w=64, h=48, seed=20):
    """The 0 / 255 field of the clamp test and of the GPU cases that share it."""
    return (np.random.default_rng(seed).integers(0, 2, size=(h, w)) * 255).astype(np.int64)
