"""CPU: tests/tensor_ref.py, the model the GPU tests of mi_display_tensor compare with, pinned
before the GPU uses it: the integer taps, the identity, the flat picture in every dtype, and the
distance from a float64 triangle filter, bounded by the two passes' rounding."""
import math

import numpy as np
import pytest

from tests import display_ref as R
from tests import tensor_ref as T

PAIRS = [(1, 1), (2, 4), (4, 2), (7, 64), (67, 10), (35, 6), (512, 8), (40, 5), (136, 1), (64, 1), (5, 33), (3840, 224),
         (2160, 224), (1100, 64), (129, 2), (6, 33)]


def tap_bound(n_in, n_out):
    return 2 * math.ceil(max(n_in / n_out, 1)) + 1


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_weights(n_in, n_out):
    wts = T.weights(n_in, n_out)
    assert len(wts) == n_out
    for i0, k in wts:
        assert all(isinstance(v, int) and v >= 0 for v in k)
        assert sum(k) == 1 << T.S
        assert 1 <= len(k) <= tap_bound(n_in, n_out)
        # the support reaches at most one sample past either edge of the ratio-wide window
        assert i0 + len(k) - 1 >= 0 and i0 <= n_in - 1


def test_tap_counts_of_the_extremes():
    assert tap_bound(3840, 224) == 37 and max(len(k) for _, k in T.weights(3840, 224)) <= 35
    assert max(len(k) for _, k in T.weights(512, 8)) == 128


def test_identity_and_two_to_four():
    for n in (1, 2, 7, 64):
        assert T.weights(n, n) == [(o, [1 << T.S]) for o in range(n)]
    w = T.weights(2, 4)
    assert w[0] == (-1, [65536, 196608]) and w[1] == (0, [196608, 65536])
    assert w[2] == (0, [65536, 196608]) and w[3] == (1, [196608, 65536])
    x = np.arange(3 * 5 * 7).reshape(3, 5, 7) * 37 % 1024
    assert np.array_equal(T.resize(x, 7, 5), x)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_flat_stays_flat(bpc):
    m = (1 << bpc) - 1
    for value in (0, 1, m // 3, m):
        x = np.full((3, 35, 67), value, dtype=np.int64)
        for size in ((10, 6), (64, 70), (2, 1)):
            y = T.resize(x, *size)
            assert y.shape == (3, size[1], size[0]) and np.all(y == value)
            assert np.all(T.finish(y, bpc, T.U8) == min(255, (value + ((1 << (bpc - 9)) if bpc > 8 else 0)) >> (bpc - 8)))
            scale, bias = T.scale_bias(bpc, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
            for dtype in (T.F16, T.BF16, T.F32):
                out = T.finish(y, bpc, dtype, scale, bias)
                for c in range(3):
                    assert np.all(out[c] == out[c, 0, 0])
    # defaults: [0, 1], exactly 0 and (to float32 rounding) 1 at the ends
    ends = T.finish(np.array([0, m]).reshape(1, 1, 2).repeat(3, 0), bpc, T.F32, *T.scale_bias(bpc))
    assert np.all(ends[:, 0, 0] == 0.0) and np.all(np.abs(ends[:, 0, 1] - 1.0) <= 2.0 ** -23)


def test_finish_dtypes():
    v = np.arange(3 * 4 * 5).reshape(3, 4, 5) * 17 % 1024
    scale, bias = T.scale_bias(10, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    f32 = T.finish(v, 10, T.F32, scale, bias)
    assert f32.dtype == np.float32
    want = (v / 1023.0 - np.array([0.485, 0.456, 0.406]).reshape(3, 1, 1)) / np.array([0.229, 0.224, 0.225]).reshape(3, 1, 1)
    assert np.max(np.abs(f32 - want)) < 1e-5
    f16 = T.finish(v, 10, T.F16, scale, bias)
    assert f16.dtype == np.float16 and np.array_equal(f16, f32.astype(np.float16))
    bf = T.finish(v, 10, T.BF16, scale, bias)
    assert bf.dtype == np.uint16
    back = (bf.astype(np.uint32) << 16).view(np.float32)
    assert np.all(np.abs(back - f32) <= np.abs(f32) * 2.0 ** -8)
    # nearest-even at the halfway points: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6 (bits 0x3f80, 0x3f82)
    half = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=np.float32)
    assert list(T.bfloat16_bits(half)) == [0x3f80, 0x3f82, 0x3f81]
    assert T.finish(np.full((3, 1, 1), 4095), 12, T.U8)[0, 0, 0] == 255      # (4095 + 8) >> 4 = 256 clips
    assert T.finish(np.full((3, 1, 1), 1023), 10, T.U8)[0, 0, 0] == 255
    assert T.finish(np.full((3, 1, 1), 6), 10, T.U8)[0, 0, 0] == 2


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("src,dst", [((67, 35), (10, 6)), ((512, 40), (8, 5)), ((7, 5), (64, 33))],
                         ids=["67x35-10x6", "512x40-8x5", "7x5-64x33"])
def test_within_bound_of_float_triangle(bpc, src, dst):
    (w, h), (ow, oh) = src, dst
    rng = np.random.default_rng(bpc * 100 + w)
    m = (1 << bpc) - 1
    cw, ch = R.chroma_size(w, h, 1)
    dt = np.uint8 if bpc == 8 else np.uint16
    planes = [rng.integers(0, m + 1, s).astype(dt) for s in ((h, w), (ch, cw), (ch, cw))]
    rgb = R.to_rgb(planes, bpc, 1, 1, 0, 0)
    got = T.resize(rgb, ow, oh)
    want = T.triangle_float(T.triangle_float(rgb, ow, -1), oh, -2)
    t_h = max(len(k) for _, k in T.weights(w, ow))
    t_v = max(len(k) for _, k in T.weights(h, oh))
    bound = (0.5 + t_h * m * 2.0 ** -19) + (0.5 + t_v * m * 2.0 ** -19)
    err = np.max(np.abs(got - want))
    print(f"bpc {bpc} {w}x{h} -> {ow}x{oh}: taps {t_h}, {t_v}; error {err:.4f}, bound {bound:.4f}")
    assert got.min() >= 0 and got.max() <= m
    assert err <= bound


def test_fit_crop():
    """decode_to_batches's crop rule (rav1d_amd/stream.py): the largest centred rectangle of the target's aspect."""
    from rav1d_amd.stream import fit_crop
    assert fit_crop(18, 16, 8, 8, "stretch") == (0, 0, 18, 16)
    assert fit_crop(18, 16, 8, 8, "crop") == (1, 0, 16, 16)
    assert fit_crop(16, 18, 8, 8, "crop") == (0, 1, 16, 16)
    assert fit_crop(352, 288, 224, 224, "crop") == (32, 0, 288, 288)
    assert fit_crop(3840, 2160, 320, 240, "crop") == (480, 0, 2880, 2160)
    assert fit_crop(100, 3, 1, 100, "crop") == (49, 0, 1, 3)
    with pytest.raises(ValueError):
        fit_crop(18, 16, 8, 8, "pad")
