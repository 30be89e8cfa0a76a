"""CPU: the plain DC-only reference (tests/dc_ref.py, Python integers from the specification of
the path) against the oracle's itxfm_add (oracle/itx.c) for every transform size, bit depth,
flat destination {0, bdmax/2, bdmax} and the directed DC list. The two then judge the device
DC paths together (tests/test_itx_dc_paths_gpu.py)."""
import numpy as np
import pytest

from rav1d_amd.synth import TX_DIMS
from tests import dc_ref
from tests.oracle_lib import load_oracle, ptr


def test_directed_list_shape():
    for bpc in (8, 10, 12):
        lo, hi = dc_ref.legal_range(bpc)
        dcs = dc_ref.directed_dcs(bpc)
        assert sorted(dcs) == sorted(dc_ref.directed_dcs(bpc, edges_first=True))
        assert {0, 1, -1, 2, -2, 3, -3, 5, -5, hi, lo, hi // 2, -(hi // 2)} <= set(dcs)
        inside = [d for d in dcs if lo <= d <= hi]
        assert len(inside) == 13 + dc_ref.N_DRAWS
        outside = sorted(set(dcs) - set(inside))
        if bpc == 8:
            assert not outside and lo == -32768 and hi == 32767      # the int16 arena bounds the list
        else:
            assert outside == [-(1 << 23), -(1 << 20), 1 << 20, (1 << 23) - 1]
        assert max(abs(d) for d in dcs) * 181 + 128 < 1 << 31       # every step stays in 32-bit int


def test_dc_block_counts_mirror_the_kernel_header():
    """itx_dc_blocks restates rav1d_amd/csrc/common.h; the constants it mirrors must still read so"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rav1d_amd", "csrc", "common.h")).read()
    assert int(re.search(r"constexpr int kItxDcItems = (\d+);", src).group(1)) == dc_ref.ITX_DC_ITEMS
    assert "imax_c(1, imin_c(128, 64 * kItxDcItems / (tx_dim(tx).h * (tx_dim(tx).w < 8 ? 1 : tx_dim(tx).w / 8))))" in src
    assert [dc_ref.itx_dc_blocks(t) for t in (0, 1, 2, 3, 4, 12, 18)] == [128, 128, 32, 8, 2, 4, 8]


@pytest.mark.parametrize("layout", [1, 0, 3])
def test_directed_frames_hold_the_runs_they_promise(layout):
    """dc_frame asserts its run lengths and that the plain reference and the oracle agree on
    every DC-only block; here also: runs inside one band, chroma runs, out-of-range DCs."""
    cases = [c for c in dc_ref.FRAME_CASES if c[2] == layout]
    assert len(cases) == (57 if layout == 1 else 12)
    for tx, bpc, _ in cases:
        fr = dc_ref.dc_frame(tx, bpc, layout)
        w, h = TX_DIMS[tx]
        blk, bs, de = fr["band_blocks"], fr["band_start"], fr["dc_end"]
        assert [int(de[tx, q] - bs[tx, q]) for q in fr["bands"]] == dc_ref.run_lengths(tx)
        dcb = fr["blocks"][fr["dc"]]
        assert len(dcb) == sum(dc_ref.run_lengths(tx)) and (~fr["dc"]).sum() >= 3
        if layout == 1:
            assert fr["chroma"] == (h <= 16)
        if fr["chroma"]:
            assert (dcb["plane"] == 1).any() and (dcb["plane"] == 2).any()
        if bpc > 8:   # the values past the legal range reach every frame
            assert set(dc_ref.out_of_range_dcs(bpc)) <= set(int(v) for v in fr["coef"][dcb["coef_off"]])
        # no two blocks overlap
        for p, (pw, ph) in enumerate(dc_ref.plane_dims(layout)):
            cover = np.zeros((ph, pw), np.int32)
            for b in fr["blocks"][fr["blocks"]["plane"] == p]:
                cover[b["y"]:b["y"] + h, b["x"]:b["x"] + w] += 1
            assert cover.max() <= 1


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_dc_ref_matches_oracle(bpc):
    o = load_oracle()
    bdmax = (1 << bpc) - 1
    cdt = np.int16 if bpc == 8 else np.int32
    dt = np.uint8 if bpc == 8 else np.uint16
    n = 0
    for tx, (w, h) in enumerate(TX_DIMS):
        for px in (0, bdmax // 2, bdmax):
            for dc in dc_ref.directed_dcs(bpc):
                c = np.zeros(min(w, 32) * min(h, 32), cdt)
                c[0] = dc
                assert int(c[0]) == dc
                d = np.full((h, w + 8), px, dt)
                o.oracle_itxfm_add(tx, 0, ptr(d), d.strides[0], ptr(c), 0, bdmax)
                want = int(dc_ref.dc_add(px, tx, dc, bpc))
                assert (d[:, :w] == want).all() and (d[:, w:] == px).all(), (tx, px, dc, want, int(d[0, 0]))
                assert not c.any()
                n += 1
    assert n == 19 * 3 * len(dc_ref.directed_dcs(bpc))
