"""CPU: the reference models of the display conversion (tests/display_ref.py) against each other
and against hand-computed values. The integer model is what the gfx950 kernel is compared with
bit for bit (tests/test_display_gpu.py), so it is pinned here first."""
import numpy as np
import pytest

from tests import display_ref as R

MATRICES = sorted(R.MATRICES)


def _planes(rng, w, h, bpc, layout, kind):
    m, half = (1 << bpc) - 1, 1 << (bpc - 1)
    cw, ch = R.chroma_size(w, h, layout)
    shapes = [(h, w)] + ([(ch, cw)] * 2 if layout else [])
    if kind == "random":
        return [rng.integers(0, m + 1, s) for s in shapes]
    # blocks of 0, M and H, independently per plane: every clip fires somewhere
    return [rng.choice([0, m, half], size=((s[0] + 3) // 4, (s[1] + 3) // 4)).repeat(4, 0).repeat(4, 1)[:s[0], :s[1]]
            for s in shapes]


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("mtrx", MATRICES)
def test_integer_model_within_one_of_float(mtrx, full, bpc):
    """Each coefficient is off by at most 0.5 / 2^14, so the sum by at most
    (4095 + 2048 + 2048) / 2^15 = 0.25, plus 0.5 of final rounding: below 1 code value."""
    rng = np.random.default_rng(mtrx * 100 + full * 10 + bpc)
    m, half = (1 << bpc) - 1, 1 << (bpc - 1)
    for layout, chr in ((1, 0), (1, 2), (2, 0), (3, 0), (0, 0)):
        cases = [_planes(rng, 37, 22, bpc, layout, k) for k in ("random", "blocks")]
        cases += [[np.full(p.shape, v) for p in cases[0]] for v in (0, m, half)]
        for planes in cases:
            a = R.to_rgb(planes, bpc, layout, mtrx, full, chr)
            b = R.to_rgb_float(planes, bpc, layout, mtrx, full, chr)
            assert np.abs(a - b).max() <= 1, (layout, chr)
            assert a.min() >= 0 and a.max() <= m


def test_upsampler_hits_every_clamp():
    """cw and ch of 1 and 2, by hand."""
    # 1 x 1 chroma (2 x 2 luma): every neighbour clamps to the sample itself
    for chr in (0, 1, 2):
        assert np.array_equal(R.upsample([[7]], 1, chr, 2, 2), [[7, 7], [7, 7]])
        assert np.array_equal(R.upsample([[7]], 1, chr, 1, 1), [[7]])
    # horizontal, cw 2: column 1 = (c0 + c1 + 1) >> 1, column 3 clamps to c1
    assert np.array_equal(R.upsample([[10, 21]], 2, 0, 4, 1), [[10, 16, 21, 21]])
    assert np.array_equal(R.upsample([[10, 21]], 2, 0, 3, 1), [[10, 16, 21]])
    # vertical, ch 2, co-located: rows c0, (c0 + c1 + 1) >> 1, c1, c1
    assert np.array_equal(R.upsample([[10], [21]], 1, 2, 1, 4), [[10], [16], [21], [21]])
    # vertical, ch 2, centred: (c0 + 3 c0 + 2) >> 2, (3 c0 + c1 + 2) >> 2, (c0 + 3 c1 + 2) >> 2, (3 c1 + c1 + 2) >> 2
    for chr in (0, 1):
        assert np.array_equal(R.upsample([[10], [21]], 1, chr, 1, 4), [[10], [13], [18], [21]])
        assert np.array_equal(R.upsample([[10], [21]], 1, chr, 1, 3), [[10], [13], [18]])
    # both passes, 2 x 2 chroma, centred: the horizontal pass runs over the integer rows
    got = R.upsample([[0, 100], [200, 40]], 1, 0, 4, 4)
    rows = [[0, 100], [50, 85], [150, 55], [200, 40]]
    want = [[a, (a + b + 1) >> 1, b, b] for a, b in rows]
    assert np.array_equal(got, want)
    # 4:4:4 and 4:0:0 have nothing to upsample
    c = np.arange(6).reshape(2, 3)
    assert np.array_equal(R.upsample(c, 3, 0, 3, 2), c)


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("mtrx", MATRICES)
def test_grey_black_and_white(mtrx, bpc):
    m, half = (1 << bpc) - 1, 1 << (bpc - 1)
    k = bpc - 8

    def px(y, full, layout=3):
        planes = [np.full((2, 2), y)] + [np.full((2, 2), half)] * (2 if layout else 0)
        return R.to_rgb(planes, bpc, layout, mtrx, full)

    # full range: mid-grey in, mid-grey out; the ends stay
    for layout in (3, 0):
        assert np.all(px(half, 1, layout) == half)
        assert np.all(px(0, 1, layout) == 0) and np.all(px(m, 1, layout) == m)
    # limited range: black and white map to 0 and M, below / above clip, grey stays neutral
    assert np.all(px(16 << k, 0) == 0) and np.all(px(235 << k, 0) == m)
    assert np.all(px(0, 0) == 0) and np.all(px(m, 0) == m)
    grey = px((16 << k) + (219 << k) // 2, 0)
    assert np.all(grey == grey[0, 0, 0]) and abs(int(grey[0, 0, 0]) - m / 2) <= 1.5


def test_identity_and_layouts():
    rng = np.random.default_rng(5)
    planes = [rng.integers(0, 1024, (5, 7)) for _ in range(3)]
    rgb = R.to_rgb(planes, 10, 3, 0, 1)
    assert np.array_equal(rgb[1], planes[0]) and np.array_equal(rgb[2], planes[1]) and np.array_equal(rgb[0], planes[2])
    rgba = R.to_rgba(planes, 10, 3, 0, 1)
    assert rgba.shape == (5, 7, 4) and np.all(rgba[..., 3] == 1023) and np.array_equal(rgba[..., 0], planes[2])
    y, uv = R.semiplanar(planes, 10, 3)
    assert np.array_equal(y, planes[0] << 6) and np.array_equal(uv[..., 1], planes[2] << 6)
    assert R.semiplanar(planes[:1], 8, 0)[1] is None


def test_coefficients_bt709_8bit():
    """The limited-range BT.709 coefficients at 8 bits, computed by hand from the definitions:
    ky = 2^14 255/219, crv = 2^14 1.5748 255/224, cbu = 2^14 1.8556 255/224."""
    yo, ky, crv, cbu, cgu, cgv = R.coefficients(1, 0, 8)
    assert (yo, ky, crv, cbu) == (16, 19077, 29372, 34610)
    assert (cgu, cgv) == (3494, 8731)
    assert R.coefficients(1, 1, 8)[:2] == (0, 16384)
