"""CPU: the directed intra frames of tests/intra_cases.py hold the blocks they are meant to hold.

For every frame the GPU tests of tests/test_intra_frame_gpu.py run (intra_cases.CASES), in luma
and, where the layout has chroma, in chroma: a block without left at an interior tile column
start, without top at an interior tile row start, without either at an interior tile corner; a
top-right and a bottom-left cut by an interior tile end on a mode that reads them; blocks
straddling the right and the bottom end of the coded area; a top-right whose available run is
shorter than the block (where the frame's geometry allows one, intra_cases.FRAMES); a CfL block
with device-computed AC and padding; and each mode remap of rav1d_prepare_intra_edges taken
because an edge is missing. The oracle must also see the tiling: the same blocks as one tile
give another picture."""
import numpy as np
import pytest

from rav1d_amd import INTRA_BOTTOM_LEFT, INTRA_TOP_RIGHT
from rav1d_amd.frame import plane_geometry
from tests import intra_cases as C
from tests import oracle_lib


def plane_shapes(w, h, bpc, layout):
    (yr, ys), (cr, cs), _ = plane_geometry(w, h, layout, bpc)
    pxb = 1 if bpc == 8 else 2
    return [(yr, ys // pxb)] + ([(cr, cs // pxb)] * 2 if layout else [])


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_case_holds_every_directed_kind(case):
    name, bpc, layout, extreme, _ = case
    w, h, sb, tcols, trows = C.FRAMES[name][:5]
    fr = C.case_frame(case)
    got = C.census(fr, layout, tcols, trows)
    missing = [k for k in C.required_kinds(name, layout) if not got.get(k)]
    assert not missing, missing


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_case_geometry(case):
    """The records say what the generator promises: blocks start inside the coded area and
    their tile, end inside the allocation, overlap nowhere, and claim a top-right or
    bottom-left only inside their tile; every dependency is an earlier block of the same tile."""
    name, bpc, layout, extreme, _ = case
    w, h, sb, tcols, trows = C.FRAMES[name][:5]
    fr = C.case_frame(case)
    b = fr["blocks"]
    ss_h, ss_v = C._subsampling(layout)
    shapes = plane_shapes(w, h, bpc, layout)
    seen = [np.zeros(s, bool) for s in shapes]
    tile_of = []
    for k, r in enumerate(b):
        p = int(r["plane"])
        sh, sv = (ss_h, ss_v) if p else (0, 0)
        x, y, bw, bh = int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])
        cw, ch = C._align(w, 8) >> sh, C._align(h, 8) >> sv
        assert x < cw and y < ch and x < r["tile_w"] <= cw and y < r["tile_h"] <= ch
        assert y + bh <= shapes[p][0] and x + bw <= (C._align(w, 128) >> sh)
        assert not seen[p][y:y + bh, x:x + bw].any()
        seen[p][y:y + bh, x:x + bw] = True
        if r["mode"] != C.MODE_IBC:
            assert r["max_w"] == cw - x and r["max_h"] == ch - y
        if r["flags"] & INTRA_TOP_RIGHT:   # (at the tile's end only as a decoder's superblock-relative flag)
            assert x + bw < r["tile_w"] or (x + bw == r["tile_w"] < cw and y % (sb >> sv) == 0)
        if r["flags"] & INTRA_BOTTOM_LEFT:
            assert y + bh < r["tile_h"]
        tile_of.append((p > 0, max(t >> sh for t in tcols if (t >> sh) <= x),
                        max(t >> sv for t in trows if (t >> sv) <= y)))
        for d in fr["deps"][k]:
            # (a CfL block also depends on the luma of its own tile)
            assert d < k and tile_of[d][1:] == (tile_of[k][1] << (sh if not tile_of[d][0] else 0),
                                                tile_of[k][2] << (sv if not tile_of[d][0] else 0))
    for p, s in enumerate(seen):
        sh, sv = (ss_h, ss_v) if p else (0, 0)
        assert s[:C._align(h, 8) >> sv, :C._align(w, 8) >> sh].all(), "the coded area is not covered"
    if extreme:
        bdmax = (1 << bpc) - 1
        assert set(np.unique(fr["pal"])) <= {0, bdmax}
        assert fr["ac"].max() > 7 * bdmax and fr["ac"].min() < -7 * bdmax
        assert (b["mode"] == C.MODE_PAL).sum() >= 8
        assert set(np.unique(b["alpha"][b["mode"] == C.MODE_CFL])) <= {-16, -1, 1, 16}


@pytest.mark.parametrize("case", [c for c in C.CASES if c[0] != "C"], ids=C.case_id)
def test_tiling_reaches_the_oracle(case):
    name, bpc, layout, extreme, _ = case
    w, h, sb, tcols, trows = C.FRAMES[name][:5]
    fr = C.case_frame(case)
    init = C.case_init(case, plane_shapes(w, h, bpc, layout))
    tiled = oracle_lib.intra_blocks(init, bpc, fr["blocks"], fr["ac"], fr["idx"], fr["pal"])
    flat = oracle_lib.intra_blocks(init, bpc, C.without_tiles(fr["blocks"], w, h, layout), fr["ac"], fr["idx"],
                                   fr["pal"])
    assert any(not np.array_equal(a, f) for a, f in zip(tiled, flat))
    # and nothing outside the blocks is touched
    for p, (a, i) in enumerate(zip(tiled, init)):
        inside = np.zeros(a.shape, bool)
        for r in fr["blocks"][fr["blocks"]["plane"] == p]:
            inside[r["y"]:r["y"] + r["h"], r["x"]:r["x"] + r["w"]] = True
        assert np.array_equal(a[~inside], i[~inside])
