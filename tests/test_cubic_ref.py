"""CPU, no device: the cubic tap tables the device builds (mi_resample_taps runs the generator of
csrc/resize.h on the host, the source the table kernel runs) against tests/cubic_ref.py bit for bit,
the sizes of the passes (mi_resample_plan) against the LDS tile, the 32-bit headroom of the sums,
and the integer model against a float64 filter and against torch's antialiased bicubic."""
import functools

import numpy as np
import pytest

from rav1d_amd.display import Resample, resample_plan, resample_taps
from tests import cubic_ref as C

SIZES = [(1, 7), (7, 1), (5, 17), (17, 5), (33, 32), (32, 33), (64, 40), (300, 1100), (640, 10), (1920, 30),
         (3840, 224), (65536, 1024)]
PHASES = [C.CENTRED, C.COSITED]
SEG = 2048            # kTensorSeg: the source columns a workgroup of the horizontal pass holds
ids_bc = [f"b{b:.3g}-c{c:.3g}" for b, c in C.BC]
ids_size = [f"{a}to{b}" for a, b in SIZES]


@functools.lru_cache(maxsize=None)
def library(n_in, n_out, phase, b, c):
    """(start, count, k, cap, seg_outputs) from the library, once per axis."""
    rs = Resample("cubic", b, c)
    cap, seg = resample_plan(rs, n_in, n_out)
    return resample_taps(rs, n_in, n_out, phase) + (cap, seg)


@pytest.mark.parametrize("size", SIZES, ids=ids_size)
@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("bc", C.BC, ids=ids_bc)
def test_taps_equal_the_model(bc, phase, size):
    """start, count and k bit for bit; the taps sum to 2^18; slots past count hold zero; the
    32-bit sums of both passes hold at 12 bits."""
    n_in, n_out = size
    start, count, k, cap, _ = library(n_in, n_out, phase, *bc)
    assert cap == 4 * -(-max(n_in, n_out) // n_out) + 1 and k.shape == (cap, n_out)
    want = C.table(n_in, n_out, phase, bc[0], bc[1], cap)
    assert np.array_equal(start, want[0])
    assert np.array_equal(count, want[1])
    assert np.array_equal(k, want[2]), np.argwhere(k != want[2])[:4].tolist()
    assert np.all(k.sum(axis=0, dtype=np.int64) == C.ONE)
    assert np.all(count >= 1) and np.all(count <= cap) and count.max() <= 256
    assert not np.any(k[np.arange(cap)[:, None] >= count[None, :]])
    worst = int(np.abs(k).sum(axis=0, dtype=np.int64).max())
    print(f"max sum|k| / 2^18 = {worst / C.ONE:.4f}")
    assert worst / C.ONE <= 1.54
    assert worst * 4095 + (1 << 17) < 1 << 31


def test_identity_for_every_filter():
    """n_in == n_out: start = o, one tap of 2^18, whatever B is, in both phases."""
    for b, c in C.BC:
        for phase in PHASES:
            start, count, k = resample_taps(Resample("cubic", b, c), 9, 9, phase)
            assert np.array_equal(start, np.arange(9)) and np.all(count == 1)
            assert np.all(k[0] == C.ONE) and not np.any(k[1:])


def test_presets():
    for name, (b, c) in (("catmull_rom", (0.0, 0.5)), ("mitchell", (1 / 3, 1 / 3)), ("cubic_075", (0.0, 0.75))):
        got, want = resample_taps(Resample(name), 17, 5), resample_taps(Resample("cubic", b, c), 17, 5)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    with pytest.raises(ValueError):
        Resample("lanczos")


def test_triangle_taps_equal_the_triangle_model():
    """The triangle through the same entry: tests/resize_ref.py's tables (NULL and "triangle")."""
    from tests import resize_ref as Z
    for n_in, n_out in ((7, 1), (5, 17), (64, 40), (640, 10), (9, 9)):
        for phase in PHASES:
            for rs in (None, Resample("triangle")):
                start, count, k = resample_taps(rs, n_in, n_out, phase)
                assert k.shape[0] == 2 * -(-max(n_in, n_out) // n_out) + 1
                for o, (i0, ks) in enumerate(Z.weights(n_in, n_out, phase)):
                    assert start[o] == i0 and count[o] == len(ks)
                    assert k[:len(ks), o].tolist() == ks and not np.any(k[len(ks):, o])


@pytest.mark.parametrize("size", SIZES, ids=ids_size)
@pytest.mark.parametrize("phase", PHASES)
def test_plan_fits_the_tile(phase, size):
    """Consecutive segments of seg_outputs outputs: the source columns their taps reach (as the
    horizontal pass stages them: clamped to the crop), plus the 15 the 8-column runs spend, fit the
    tile, and no output has more taps than slots. Cubic (the widest of the (B, C)) and triangle."""
    n_in, n_out = size
    tables = [library(n_in, n_out, phase, *bc) for bc in C.BC]
    tables.append(resample_taps(None, n_in, n_out, phase) + resample_plan(None, n_in, n_out))
    for start, count, k, cap, seg in tables:
        assert 1 <= seg <= 1024 and count.max() <= cap
        worst = 0
        for o0 in range(0, n_out, seg):
            o1 = min(o0 + seg, n_out) - 1
            lo = min(max(int(start[o0]), 0), n_in - 1)
            hi = min(max(int(start[o1] + count[o1]), 1), n_in)
            # every output of the segment reads inside [lo, hi)
            first = np.clip(start[o0:o1 + 1], 0, n_in - 1)
            last = np.clip(start[o0:o1 + 1] + count[o0:o1 + 1] - 1, 0, n_in - 1)
            assert first.min() >= lo and last.max() < hi
            worst = max(worst, hi - lo)
        print(f"{n_in} -> {n_out} phase {phase} cap {cap}: {seg} outputs reach {worst} columns")
        assert worst + 15 <= SEG


# ---- the integer model against float64 ----
def total_bound(axes, b, c, maxv):
    """e (1 + A): e the largest per-pass 0.5 + n_taps 2^-19 M, A the largest sum |k| / 2^18."""
    ea = [C.float_bound(n_in, n_out, phase, b, c, maxv) for n_in, n_out, phase in axes]
    return max(e for e, _ in ea) * (1 + max(a for _, a in ea))


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("bc", C.BC, ids=ids_bc)
def test_integer_model_within_the_float_filter(bc, bpc):
    """Ratios up to 8, both phases, random samples and the 0 / M field (which drives both clamps)."""
    b, c = bc
    m = (1 << bpc) - 1
    rng = np.random.default_rng(bpc)
    for (w, h), (ow, oh) in (((64, 48), (40, 30)), ((64, 48), (96, 80)), ((40, 33), (5, 9)), ((9, 7), (72, 50))):
        for px, py in ((C.CENTRED, C.CENTRED), (C.COSITED, C.COSITED)):
            for x in (rng.integers(0, m + 1, size=(h, w)), rng.integers(0, 2, size=(h, w)) * m):
                got = C.resize(x, ow, oh, m, px, py, b, c)
                ref = C.cubic_float(C.cubic_float(x, ow, -1, m, px, b, c), oh, -2, m, py, b, c)
                bound = total_bound([(w, ow, px), (h, oh, py)], b, c, m)
                err = float(np.abs(got - ref).max())
                print(f"{w}x{h} -> {ow}x{oh} phases {px}{py} {bpc} bits: max error {err:.3f}, bound {bound:.3f}")
                assert got.min() >= 0 and got.max() <= m
                assert err <= bound


def test_the_clamp_between_the_passes_matters():
    """The 64 x 48 field of 0 / 255 to 40 x 30 with Catmull-Rom: the horizontal pass overshoots, so
    the model with the intermediate clamp and the one without differ."""
    x = C.field()
    with_clamp = C.resize(x, 40, 30, 255)
    final_only = np.clip(C.resize(x, 40, 30, 255, clamp=False), 0, 255)
    n = int((with_clamp != final_only).sum())
    print(f"{n} of {with_clamp.size} samples differ")
    assert with_clamp.shape == (30, 40) and n > 0


def test_catmull_rom_interior_equals_torch_bicubic_antialias():
    """Interior outputs (every tap inside the samples) of (0, 0.5) centred against
    torch.nn.functional.interpolate(mode="bicubic", antialias=True) on float64 CPU tensors, within
    the float bound. One axis at a time (torch's result clamped to [0, M], as the pass clamps:
    clamping both sides never widens their distance), then both axes on samples in the middle half
    of the range, where neither pass clamps. Edges differ by design: this project clamps indices,
    torch renormalises."""
    import torch
    import torch.nn.functional as F
    m = 255
    rng = np.random.default_rng(5)

    def interior(n_in, n_out):
        ws = C.weights(n_in, n_out)
        return np.array([i0 >= 0 and i0 + len(k) <= n_in for i0, k in ws])

    def bicubic(x, oh, ow):
        t = torch.from_numpy(np.asarray(x, dtype=np.float64))[None, None]
        return F.interpolate(t, size=(oh, ow), mode="bicubic", antialias=True, align_corners=False)[0, 0].numpy()

    for n_in, n_out in ((64, 40), (48, 30), (33, 80), (200, 26), (37, 36)):
        x = rng.integers(0, m + 1, size=(6, n_in))
        inner = interior(n_in, n_out)
        assert inner.sum() >= n_out // 2
        e, _ = C.float_bound(n_in, n_out, C.CENTRED, 0.0, 0.5, m)
        got = C.resize_axis(x, n_out, -1, m)
        err = np.abs(got - np.clip(bicubic(x, 6, n_out), 0, m))[:, inner].max()
        print(f"x {n_in} -> {n_out}: max interior error {err:.3f}, bound {e:.3f}")
        assert err <= e
        got = C.resize_axis(x.T, n_out, -2, m)
        err = np.abs(got - np.clip(bicubic(x.T, n_out, 6), 0, m))[inner, :].max()
        print(f"y {n_in} -> {n_out}: max interior error {err:.3f}, bound {e:.3f}")
        assert err <= e
    for (w, h), (ow, oh) in (((64, 48), (40, 30)), ((30, 20), (77, 45))):
        x = rng.integers(64, 192, size=(h, w))
        got = C.resize(x, ow, oh, m)
        bound = total_bound([(w, ow, C.CENTRED), (h, oh, C.CENTRED)], 0.0, 0.5, m)
        err = np.abs(got - bicubic(x, oh, ow))[np.ix_(interior(h, oh), interior(w, ow))].max()
        print(f"{w}x{h} -> {ow}x{oh}: max interior error {err:.3f}, bound {bound:.3f}")
        assert err <= bound
