"""GPU parity of the inverse transforms on the directed inputs of tests/itx_cases.py:
coefficients at the ends of their range for every (size, type) pair, every packed corner shape,
through every route that runs an inverse transform (mi_itx_frame plain / banded / runs, dense and
packed arenas, mi_dsp_itxfm_add per call, the fused intra reconstruction). Expectations come
from the oracle (the 64-bit exact restatement); every comparison is bit-exact and covers the
whole allocated planes, so a write outside a block shows too. tests/test_itx_cases.py shows
without a GPU which slips these inputs notice."""
import functools

import numpy as np
import pytest
import torch

from rav1d_amd import ITX_KEEP_COEFS, lib
from rav1d_amd.frame import Frame, _stream_ptr, itx_frame
from rav1d_amd.synth import TX_DIMS, itx_band_order, itx_dc_runs
from tests import itx_cases as C
from tests import oracle_lib
from tests.oracle_lib import ptr

pytestmark = pytest.mark.gpu

ROUTES = ("plain", "banded", "runs")


def run_frame(gpu, fr, route="plain", flags=0):
    """The frame through one route; returns (whole allocated planes, arena afterwards)."""
    f = Frame(fr["w"], fr["h"], fr["bpc"], fr["layout"])
    for p, arr in enumerate(fr["planes"]):
        f.set_buffer_np(p, arr)
    blk, bands, dc_end = fr["blocks"], None, None
    if route != "plain":
        ah = (fr["h"] + 127) & ~127
        ch = ah >> (1 if fr["layout"] == 1 else 0)
        blk, _, bands = itx_band_order(blk, [ah, ch, ch])
        if route == "runs":
            dc_end = itx_dc_runs(blk, bands)
            assert (dc_end > bands[:, :-1]).any(), "no DC run"
    blocks = torch.from_numpy(blk.view(np.uint8).copy()).cuda()
    coef = torch.from_numpy(fr["coef"].copy()).cuda()
    itx_frame(gpu, f, blocks, fr["size_start"], coef, flags, band_start=bands, dc_end=dc_end)
    torch.cuda.synchronize()
    assert lib().mi_ctx_device_status(gpu.h, _stream_ptr(None)) == 0, "a descriptor was rejected"
    return [f.buffer_np(p) for p in range(len(fr["planes"]))], coef.cpu().numpy()


@functools.lru_cache(maxsize=4)
def expected(bpc, base, layout, kind):
    """(dense frame, packed frame, the oracle's planes): computed once per frame, left unchanged."""
    dense = C.directed_frame(bpc, base, layout, kind)
    packed = C.directed_frame(bpc, base, layout, kind, packed=True)
    coef = dense["coef"].copy()
    ref = oracle_lib.itx_frame([p.copy() for p in dense["planes"]], dense["blocks"], coef, bpc)
    assert not coef.any()
    pcoef = packed["coef"].copy()
    pref = oracle_lib.itx_frame([p.copy() for p in packed["planes"]], packed["blocks"], pcoef, bpc)
    assert not pcoef.any() and all(np.array_equal(a, b) for a, b in zip(ref, pref)), "the oracle expands a packed corner"
    for p in ref:
        p.setflags(write=False)
    return dense, packed, ref


def assert_planes(got, ref, fr, what):
    for p in range(len(ref)):
        if not np.array_equal(got[p], ref[p]):
            bad = np.argwhere(got[p] != ref[p])
            y, x = (int(v) for v in bad[0])
            b = fr["blocks"]
            dims = np.array(TX_DIMS)
            hit = np.nonzero((b["plane"] == p) & (b["x"] <= x) & (x < b["x"] + dims[b["tx"], 0]) &
                             (b["y"] <= y) & (y < b["y"] + dims[b["tx"], 1]))[0]
            who = [(int(b["tx"][k]), int(b["txtp"][k]), fr["cases"][fr["case_of_block"][k]][4]) for k in hit]
            raise AssertionError(f"{what}: plane {p}: {len(bad)} pixels differ, first at x {x} y {y}: got "
                                 f"{got[p][y, x]} expected {ref[p][y, x]}, block (tx, txtp, pattern) {who or 'none'}")


@pytest.mark.parametrize("base", C.PIXEL_BASES)
@pytest.mark.parametrize("layout", [1, 3])
@pytest.mark.parametrize("bpc", C.BPCS)
def test_frame_routes_at_extremes(gpu, bpc, layout, base):
    """One block per (size, type, pattern) and DC-only blocks at max / min, through the plain,
    banded and runs routes, from the dense arena and from the arena pack_coefs packs; the
    consumed coefficients are zeroed."""
    dense, packed, ref = expected(bpc, base, layout, "pairs")
    fl = packed["blocks"]["flags"]
    assert (fl & 0x80).any() and packed["coef"].size < dense["coef"].size
    if bpc > 8:
        assert (fl & 0x40).any() and ((fl & 0xc0) == 0x80).any(), "both arena forms: MI_TX_I16 and int32 corners"
    for route in ROUTES:
        for name, fr in (("dense", dense), ("packed", packed)):
            got, coef_after = run_frame(gpu, fr, route)
            assert_planes(got, ref, fr, f"{route} {name}")
            assert not coef_after.any(), f"{route} {name}: coefficients not zeroed"


@pytest.mark.parametrize("layout", [0, 2])
@pytest.mark.parametrize("bpc", C.BPCS)
def test_plain_route_monochrome_and_422(gpu, bpc, layout):
    for base in C.PIXEL_BASES:
        dense, packed, ref = expected(bpc, base, layout, "pairs")
        for name, fr in (("dense", dense), ("packed", packed)):
            got, coef_after = run_frame(gpu, fr)
            assert_planes(got, ref, fr, f"{base} {name}")
            assert not coef_after.any()


@pytest.mark.parametrize("layout", [1, 3])
@pytest.mark.parametrize("bpc", C.BPCS)
def test_keep_coefs_at_extremes(gpu, bpc, layout):
    """MI_ITX_KEEP_COEFS: the same pixels, the arena (dense and packed) untouched."""
    dense, packed, ref = expected(bpc, "rand", layout, "pairs")
    for route in ROUTES:
        for name, fr in (("dense", dense), ("packed", packed)):
            got, coef_after = run_frame(gpu, fr, route, flags=ITX_KEEP_COEFS)
            assert_planes(got, ref, fr, f"{route} {name}")
            assert np.array_equal(coef_after, fr["coef"]), f"{route} {name}: arena changed"


@pytest.mark.parametrize("layout", [1, 3])
@pytest.mark.parametrize("bpc", C.BPCS)
def test_every_corner_shape(gpu, bpc, layout):
    """Every packed corner shape (cw, ch) of every size, as int16 pairs and (10 / 12 bits) as
    int32 entries, through the plain and the banded route."""
    for base in C.PIXEL_BASES:
        dense, packed, ref = expected(bpc, base, layout, "corners")
        fl = packed["blocks"]["flags"]
        shapes = {(int(t), int(f) & 0x3f, bool(f & 0x40)) for t, f in zip(packed["blocks"]["tx"], fl) if f & 0x80}
        for tx in range(1, 19):
            forms = (True, False) if bpc > 8 else (False,)
            want = {(tx, ((cw // 4 - 1) << 3) | (ch // 4 - 1), i16) for (cw, ch) in C.corner_shapes(tx) for i16 in forms}
            assert want <= shapes, tx
        for route in ("plain", "banded"):
            for name, fr in (("dense", dense), ("packed", packed)):
                got, coef_after = run_frame(gpu, fr, route)
                assert_planes(got, ref, fr, f"{base} {route} {name}")
                assert not coef_after.any()


@pytest.mark.parametrize("bpc", C.BPCS)
def test_per_call_at_extremes(gpu, bpc):
    """mi_dsp_itxfm_add on host buffers: max, min and the two matched patterns of widest reach of
    every pair (624 calls)."""
    L = lib()
    o = oracle_lib.load_oracle()
    cdt = np.int16 if bpc == 8 else np.int32
    dt = np.uint8 if bpc == 8 else np.uint16
    rng = np.random.default_rng(0x17C0 + bpc)
    calls = 0
    for tx, txtp in C.PAIRS:
        w, h = TX_DIMS[tx]
        for name in ("max", "min") + C.widest_matches(tx, txtp):
            c, eob = C.pattern(tx, txtp, bpc, name)
            c = c.astype(cdt)
            d = rng.integers(0, 1 << bpc, size=(h + 2, w + 16)).astype(dt)
            c_ref, d_ref = c.copy(), d.copy()
            o.oracle_itxfm_add(tx, txtp, ptr(d_ref[1:]), d_ref.strides[0], ptr(c_ref), eob, (1 << bpc) - 1)
            assert L.mi_dsp_itxfm_add(tx, txtp, ptr(d[1:]), d.strides[0], ptr(c), eob, (1 << bpc) - 1) == 0
            assert np.array_equal(d, d_ref), (tx, txtp, name)
            assert not c.any() and not c_ref.any()
            calls += 1
    assert calls < 2000


def test_lossless_10bit_all_max(gpu):
    """Sixteen coefficients of 131071 through WHT_WHT at 10 bits: the row pass gives 65534 and
    the column pass 131068, both inside the 18 bits a 10-bit stream may use and both beyond
    int16. All of it lands on the first pixel: on pixels of 511 it becomes 1023 exactly (507 if
    the hand-off were cut to int16), the others stay."""
    c = np.full(16, 131071, np.int32)
    d = np.full((4, 4), 511, np.uint16)
    c_ref, d_ref = c.copy(), d.copy()
    oracle_lib.load_oracle().oracle_itxfm_add(0, C.WHT, ptr(d_ref), d_ref.strides[0], ptr(c_ref), 15, 1023)
    want = np.full((4, 4), 511, np.uint16)
    want[0, 0] = 1023
    assert np.array_equal(d_ref, want)
    assert lib().mi_dsp_itxfm_add(0, C.WHT, ptr(d), d.strides[0], ptr(c), 15, 1023) == 0
    assert np.array_equal(d, want), d
    assert not c.any()


@pytest.mark.parametrize("granules", [False, True])
@pytest.mark.parametrize("bpc", C.BPCS)
def test_fused_intra_recon_at_extremes(gpu, bpc, granules):
    """The fused intra reconstruction with every transform block's type, eob and coefficients
    replaced by the directed patterns: all 19 sizes, every legal type (WHT_WHT on 4x4 too) with a
    pattern of every class."""
    from rav1d_amd.intra import IntraFrame, device_status
    frames = C.intra_frames(bpc)
    dealt = set().union(*[d for _, _, d in frames])
    assert {tx for tx, _, _ in dealt} == set(range(19))
    for pr in C.PAIRS:
        assert {C.pattern_class(n) for tx, t, n in dealt if (tx, t) == pr} == set(C.CLASSES), pr
    for k, (fr, init_name, _) in enumerate(frames):
        w, h, layout = C.INTRA_FRAMES[k][:3]
        init = C.intra_init(w, h, layout, bpc, init_name)
        exp, arena = _intra_expected(bpc, k)
        cur = Frame(w, h, bpc, layout)
        for p in range(len(cur.planes)):
            cur.set_buffer_np(p, init[p])
        intra = IntraFrame(gpu, fr)
        intra.recon(cur.picture(), keep_coefs=False, granules=granules)
        device_status(gpu)
        for p in range(len(cur.planes)):
            got = cur.buffer_np(p)
            if not np.array_equal(got, exp[p]):
                bad = np.argwhere(got != exp[p])
                raise AssertionError(f"{w}x{h} layout {layout} plane {p}: {len(bad)} mismatches, first at {bad[0]}: "
                                     f"got {got[tuple(bad[0])]} exp {exp[p][tuple(bad[0])]}")
        assert not arena.any() and int(torch.count_nonzero(intra.coef)) == 0, "coefficients not zeroed"


@functools.lru_cache(maxsize=None)
def _intra_expected(bpc, k):
    """The oracle's reconstruction of fused frame k (shared by both granule settings)."""
    w, h, layout = C.INTRA_FRAMES[k][:3]
    fr, init_name, _ = C.intra_frames(bpc)[k]
    init = C.intra_init(w, h, layout, bpc, init_name)
    return oracle_lib.intra_recon(init, bpc, fr["blocks"], fr["tx_blocks"][fr["tx_of_block"]], fr["ac"], fr["idx"],
                                  fr["pal"], fr["coef"])


@pytest.mark.parametrize("granules", [False, True])
def test_intra_recon_12bit_identity32_saturates(gpu, granules):
    """12 bpc identity transforms on 32-point columns with every coefficient at the row clip:
    the column pass's identity32 (x4, unclipped, itx_1d.rs:1106-1121) drives (c + 8) >> 4 to
    +32768, one past int16. The fused kernel keeps the residual in int16 LDS,
    so it must saturate rather than wrap (a wrapped +32768 turns a pixel that clips to 4095
    into 0: Argon 12-bit test15549_5522_4902). Negative blocks reach -32768 exactly."""
    from rav1d_amd.intra import IntraFrame, device_status, make_intra_residuals
    from rav1d_amd.ipred_synth import make_intra_frame
    w, h, bpc, layout = 256, 192, 12, 3
    rng = np.random.default_rng(0x12B1D)
    fr = make_intra_residuals(make_intra_frame(w, h, bpc, layout, rng, sb=64, min_bs=8, tx_split=0.2), bpc, rng)
    cf_max = (128 << bpc) - 1
    tb, coef = fr["tx_blocks"], fr["coef"]
    hit = set()
    for k in range(len(tb)):
        tw, th = TX_DIMS[int(tb[k]["tx"])]
        if th != 32 or tw < 8 or tw > 32:   # (64-wide sizes take DCT_DCT only)
            continue
        n = min(tw, 32) * 32
        off = int(tb[k]["coef_off"])
        sign = 1 if k % 3 else -1
        coef[off:off + n] = sign * cf_max
        tb[k]["txtp"] = 9          # IDTX
        tb[k]["eob"] = n - 1
        hit.add((tw, th))
    assert {(32, 32), (8, 32), (16, 32)} <= hit, f"sizes covered: {sorted(hit)}"
    cur = Frame(w, h, bpc, layout)
    for p in range(len(cur.planes)):
        cur.set_buffer_np(p, rng.integers(0, 1 << bpc, size=cur.buffer_np(p).shape))
    init = [cur.buffer_np(p) for p in range(len(cur.planes))]
    IntraFrame(gpu, fr).recon(cur.picture(), granules=granules)
    device_status(gpu)
    exp, _ = oracle_lib.intra_recon(init, bpc, fr["blocks"], fr["tx_blocks"][fr["tx_of_block"]], fr["ac"], fr["idx"],
                                    fr["pal"], fr["coef"])
    for p in range(len(cur.planes)):
        got = cur.buffer_np(p)
        if not np.array_equal(got, exp[p]):
            bad = np.argwhere(got != exp[p])
            raise AssertionError(f"plane {p}: {len(bad)} mismatches, first at {bad[0]}: got {got[tuple(bad[0])]} "
                                 f"exp {exp[p][tuple(bad[0])]}")
