"""CPU: tests/scaled_ref.py, the model the GPU tests of mi_display_scaled compare with, pinned
before the GPU uses it: the taps of both sitings, the identity, the flat picture, the distance from
a float64 triangle filter at the same sited positions, the depth conversion and the packing."""
import numpy as np
import pytest

from tests import display_ref as R
from tests import scaled_ref as Z
from tests import tensor_ref as T
from tests.test_tensor_ref import PAIRS


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_centred_taps_are_the_tensor_taps(n_in, n_out):
    assert Z.weights(n_in, n_out, Z.CENTRED) == T.weights(n_in, n_out)
    assert Z.weights(n_in, n_out) == T.weights(n_in, n_out)


def test_cosited_identity_and_two_to_one():
    for n in (1, 2, 7, 64, 69):
        assert Z.weights(n, n, Z.COSITED) == [(o, [1 << Z.S]) for o in range(n)]
    # 2:1: the interior outputs are [3, 7, 5, 1] / 16 from sample 2o - 1
    for n in (4, 9, 32):
        w = Z.weights(2 * n, n, Z.COSITED)
        unit = (1 << Z.S) // 16
        for o in range(1, n - 1):
            assert w[o] == (2 * o - 1, [3 * unit, 7 * unit, 5 * unit, unit])
    x = np.arange(5 * 7).reshape(5, 7) * 37 % 1024
    assert np.array_equal(Z.resize_plane(x, 7, 5, Z.COSITED, Z.COSITED), x)


@pytest.mark.parametrize("phase", [Z.CENTRED, Z.COSITED])
def test_taps_are_positive_and_sum_to_one(phase):
    """Every extent pair 1..69 x 1..39 inside the 64:1 bound: every tap is positive, an output's
    taps sum to 2^18, and there are at most 2 ceil(max(ratio, 1)) + 1 of them."""
    n = 0
    for n_in in range(1, 70):
        for n_out in range(1, 40):
            if n_in > 64 * n_out:
                continue
            wts = Z.weights(n_in, n_out, phase)
            assert len(wts) == n_out
            cap = 2 * -(-max(n_in, n_out) // n_out) + 1
            for i0, k in wts:
                assert all(isinstance(v, int) and v > 0 for v in k), (n_in, n_out)
                assert sum(k) == 1 << Z.S
                assert 1 <= len(k) <= cap
                assert i0 + len(k) - 1 >= 0 and i0 <= n_in - 1
            n += 1
    assert n > 2600


def test_tap_count_at_64_to_1():
    for phase in (Z.CENTRED, Z.COSITED):
        assert max(len(k) for _, k in Z.weights(512, 8, phase)) == 128
        assert max(len(k) for _, k in Z.weights(128, 2, phase)) <= 128


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_flat_stays_flat(layout, bpc):
    """A constant plane stays constant through any resize, crop and siting."""
    m = (1 << bpc) - 1
    w, h = 67, 35
    cw, ch = R.chroma_size(w, h, layout)
    for vy, vu, vv in ((0, m, 1), (m, 0, m // 3), (1 << (bpc - 1), m // 3, m)):
        planes = [np.full((h, w), vy)] + ([np.full((ch, cw), vu), np.full((ch, cw), vv)] if layout else [])
        for size, crop in (((10, 6), None), ((64, 70), None), ((2, 1), None), ((9, 5), (2, 4, 40, 22)), ((80, 40), (66, 34, 1, 1))):
            for chr in (0, 2):
                y, uv = Z.scaled(planes, bpc, layout, chr, size, crop=crop)
                sh = 16 - bpc if bpc > 8 else 0
                assert y.shape == (size[1], size[0]) and np.all(y == vy << sh)
                if layout:
                    assert uv.shape == R.chroma_size(size[0], size[1], layout)[::-1] + (2,)
                    assert np.all(uv[..., 0] == vu << sh) and np.all(uv[..., 1] == vv << sh)
                else:
                    assert uv is None


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("src,dst", [((67, 35), (10, 6)), ((136, 70), (64, 33)), ((7, 5), (64, 33)), ((65, 33), (30, 40))],
                         ids=["67x35-10x6", "136x70-64x33", "7x5-64x33", "65x33-30x40"])
def test_within_one_code_of_float_triangle(bpc, src, dst):
    """Both sitings on both axes: the integer result is within 1 code of the float64 filter
    evaluated at the same sited positions, the bound the call promises. Each pass rounds once, by
    at most half a code, and the 18-bit taps add at most t M 2^-19 per pass (below 0.02 code at
    these tap counts), so the provable worst case is a little above 1 and needs both roundings at
    their extreme on one sample; over these seeded planes the largest distance is 0.9957."""
    (w, h), (ow, oh) = src, dst
    rng = np.random.default_rng(bpc * 100 + w)
    m = (1 << bpc) - 1
    x = rng.integers(0, m + 1, (h, w))
    for px in (Z.CENTRED, Z.COSITED):
        for py in (Z.CENTRED, Z.COSITED):
            got = Z.resize_plane(x, ow, oh, px, py)
            want = Z.triangle_float(Z.triangle_float(x, ow, -1, px), oh, -2, py)
            err = np.max(np.abs(got - want))
            print(f"bpc {bpc} {w}x{h} -> {ow}x{oh} phases {px}, {py}: error {err:.4f}")
            assert got.min() >= 0 and got.max() <= m
            assert err <= 1.0


def test_sited_positions_differ():
    """The co-sited taps are not the centred ones wherever the extents differ: a ramp resized 2:1
    lands a quarter of an output sample apart."""
    x = np.arange(64)[None, :] * 16
    a = Z.resize_axis(x, 32, -1, Z.CENTRED)[0, 4:-4]
    b = Z.resize_axis(x, 32, -1, Z.COSITED)[0, 4:-4]
    assert np.all(a - b == 4)      # centres at 2o + 0.5 against 2o + 0.25, in input samples of 16 codes


def test_depth_conversion():
    """16 << k, 235 << k, 240 << k map to the corresponding codes in both directions, and no
    result exceeds Md."""
    for s in (8, 10, 12):
        for d in (8, 10, 12):
            for code in (16, 235, 240, 0, 128):
                assert Z.depth(np.array([code << (s - 8)]), s, d)[0] == code << (d - 8)
            every = Z.depth(np.arange(1 << s), s, d)
            assert every.min() == 0 and every.max() <= (1 << d) - 1
            assert np.all(np.diff(every) >= 0)
            if d >= s:
                assert np.array_equal(every, np.arange(1 << s) << (d - s))
    assert Z.depth(np.array([4095]), 12, 8)[0] == 255       # (4095 + 8) >> 4 = 256 clips
    assert Z.depth(np.array([1023]), 10, 8)[0] == 255
    assert Z.depth(np.array([4094]), 12, 10)[0] == 1023     # (4094 + 2) >> 2 = 1024 clips
    assert Z.depth(np.array([6]), 10, 8)[0] == 2


def test_packing_and_crops():
    """1:1 at the source depth is display_ref.semiplanar of the planes; a crop is the crop of it;
    the chroma crop follows the header's extents."""
    rng = np.random.default_rng(3)
    for layout in range(4):
        w, h, bpc = 17, 9, 10
        cw, ch = R.chroma_size(w, h, layout)
        planes = [rng.integers(0, 1024, s) for s in [(h, w)] + ([(ch, cw)] * 2 if layout else [])]
        y, uv = Z.scaled(planes, bpc, layout, 2, (w, h))
        ry, ruv = R.semiplanar(planes, bpc, layout)
        assert np.array_equal(y, ry) and (uv is None if not layout else np.array_equal(uv, ruv))
        # an even-origin crop reaching the odd right and bottom edges, 1:1
        y, uv = Z.scaled(planes, bpc, layout, 0, (13, 5), crop=(4, 4, 13, 5))
        assert np.array_equal(y, ry[4:, 4:])
        if layout:
            sh, sv = int(layout in (1, 2)), int(layout == 1)
            assert np.array_equal(uv, ruv[4 >> sv:, 4 >> sh:])
    assert Z.crops(17, 9, 1, (4, 2, 13, 7)) == ((4, 2, 13, 7), (2, 1, 7, 4))
    assert Z.crops(17, 9, 2, (4, 3, 12, 5)) == ((4, 3, 12, 5), (2, 3, 6, 5))
    assert Z.crops(17, 9, 1, None) == ((0, 0, 17, 9), (0, 0, 9, 5))


def test_even_crop():
    """rav1d_amd.display.even_crop moves a crop onto the chroma grid inside the picture."""
    from rav1d_amd.display import even_crop
    assert even_crop((1, 0, 16, 16), 18, 16, 1) == (0, 0, 18, 16)      # odd origin: one left, then even extent
    assert even_crop((3, 5, 10, 6), 179, 120, 1) == (2, 4, 12, 8)
    assert even_crop((3, 5, 10, 6), 179, 120, 2) == (2, 5, 12, 6)
    assert even_crop((3, 5, 10, 6), 179, 120, 3) == (3, 5, 10, 6)
    assert even_crop((170, 0, 9, 120), 179, 120, 1) == (170, 0, 9, 120)    # reaches the odd right edge
    assert even_crop((0, 0, 9, 5), 179, 120, 1) == (0, 0, 10, 6)
