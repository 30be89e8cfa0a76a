"""Reference model of the separable triangle resize the tensor and the scaled outputs share
(include/mi_av1out.h), written from the arithmetic the header states: the integer taps in both
sitings (centred: (2o+1) / (2i+1); co-sited: (4o+1) / (4i+1)) and one pass over an axis. A float64
triangle filter evaluated at the same sited positions bounds the integer one."""
import numpy as np

S = 18
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
