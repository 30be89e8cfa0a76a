"""The directed inverse-transform inputs (tests/itx_cases.py), checked without a GPU: that every
(size, type) pair holds every pattern, that the packed corner shapes are all there in both arena
forms, and, on the census flavour of the oracle (oracle/census.h), that the inputs reach every
clip and would notice a slip: which single-decision mutant of oracle/itx.c changes a pixel of
which pair is written down below (KILLS), so that a generator change that loses a kill shows.

The kill analysis runs the pair patterns on flat pictures of 0, bdmax and mid grey (one block
per (pair, pattern), laid out by the same shelf packer the GPU frames use)."""
import ctypes
import functools

import numpy as np
import pytest

from rav1d_amd.synth import TX_DIMS, pack_coefs, tx_types
from tests import itx_cases as C
from tests import oracle_lib

MUTANTS = ("ROT_I32", "NO_CLIP", "NO_MIDCLIP", "MID_I16", "RES_I16", "WHT_MID_I16")
COUNTERS = ("ROW_CLIP_LO", "ROW_CLIP_HI", "COL_CLIP_LO", "COL_CLIP_HI", "MID_CLIP_LO", "MID_CLIP_HI",
            "PX_CLIP_0", "PX_CLIP_MAX", "RES_GT_I16", "WHT_MID_GT_I16", "ROT_GE_2P31")
IDTX = 9

# KILLS[bpc][mutant][tx]: bit t set when the mutant changes a pixel of a pattern of (tx, type t)
# (bit 16: WHT_WHT). Measured by analysis() below; a pair that is missing cannot be told from the
# oracle through pixels by these inputs (often by no input: at 8 bits the hand-off clip re-applies
# the bound NO_CLIP removes on 4x4, ROT_I32 and MID_I16 change nothing below 12 bits).
KILLS = {
    8: {
        "ROT_I32": (0,) * 19,
        "NO_CLIP": (0x0000, 0xfdff, 0x0dff, 0x0001, 0x0001, 0x55ff, 0xa9ff, 0xfdff, 0xfdff, 0x0001,
                    0x0001, 0x0001, 0x0001, 0x55ff, 0xa9ff, 0x0001, 0x0001, 0x0001, 0x0001),
        "NO_MIDCLIP": (0x55ec, 0x0000, 0x0000, 0x0000, 0x0000, 0x01ec, 0x55ec, 0x0000, 0x0000, 0x0000,
                       0x0000, 0x0000, 0x0000, 0x01ec, 0x5400, 0x0000, 0x0000, 0x0000, 0x0000),
        "MID_I16": (0,) * 19,
        "RES_I16": (0,) * 19,
        "WHT_MID_I16": (0,) * 19,
    },
    10: {
        "ROT_I32": (0,) * 19,
        "NO_CLIP": (0x0000, 0xfdff, 0x0dff, 0x0001, 0x0001, 0x55ff, 0xa9ff, 0xfdff, 0xfdff, 0x0001,
                    0x0001, 0x0001, 0x0001, 0x55ff, 0xa9ff, 0x0001, 0x0001, 0x0001, 0x0001),
        "NO_MIDCLIP": (0x55ff, 0x55ff, 0x05ff, 0x0001, 0x0001, 0x55ff, 0x55ff, 0x55ff, 0x55ff, 0x0001,
                       0x0001, 0x0001, 0x0001, 0x55ff, 0x55ff, 0x0001, 0x0001, 0x0001, 0x0001),
        "MID_I16": (0,) * 19,
        "RES_I16": (0,) * 19,
        "WHT_MID_I16": (0x10000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000,
                        0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000),
    },
    12: {
        "ROT_I32": (0xa9ff, 0xa9ff, 0x09ff, 0x0001, 0x0001, 0xa1ec, 0xa1ec, 0xa1ec, 0xa9ff, 0x0001,
                    0x0001, 0x0001, 0x0001, 0xa9ff, 0xa9ff, 0x0001, 0x0001, 0x0001, 0x0001),
        "NO_CLIP": (0x0000, 0xfdff, 0x0dff, 0x0001, 0x0001, 0x55ff, 0xa9ff, 0xfdff, 0xfdff, 0x0001,
                    0x0001, 0x0001, 0x0001, 0x55ff, 0xa9ff, 0x0001, 0x0001, 0x0001, 0x0001),
        "NO_MIDCLIP": (0x55ff, 0x55ff, 0x05ff, 0x0001, 0x0001, 0x55ff, 0x55ff, 0x55ff, 0x55ff, 0x0001,
                       0x0001, 0x0001, 0x0001, 0x55ff, 0x55ff, 0x0001, 0x0001, 0x0001, 0x0001),
        "MID_I16": (0xffff, 0xffff, 0x0fff, 0x0201, 0x0001, 0xffff, 0xffff, 0xffff, 0xffff, 0x0201,
                    0x0201, 0x0001, 0x0001, 0xffff, 0xffff, 0x0201, 0x0201, 0x0001, 0x0001),
        "RES_I16": (0x0000, 0x0000, 0x0000, 0x0200, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0200,
                    0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0200, 0x0000, 0x0000, 0x0000),
        "WHT_MID_I16": (0x10000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000,
                        0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000, 0x0000),
    },
}


def _label_map(fr):
    """Block index per pixel of plane 0 (-1: no block); asserts that no two blocks overlap."""
    label = np.full(fr["planes"][0].shape, -1, np.int32)
    b = fr["blocks"]
    for k in range(len(b)):
        w, h = TX_DIMS[b["tx"][k]]
        cell = label[b["y"][k]:b["y"][k] + h, b["x"][k]:b["x"][k] + w]
        assert cell.shape == (h, w) and (cell == -1).all()
        cell[:] = k
    return label


@functools.lru_cache(maxsize=None)
def analysis(bpc):
    """(kills: mutant -> set of pairs, counters: pair -> census counts) of one bit depth."""
    cen = oracle_lib.load_census()
    cases = C.pair_cases(bpc)
    kills = {m: set() for m in MUTANTS}
    ctr = {}
    try:
        for base in ("zero", "max", "mid"):
            fr = C.build_frame(cases, bpc, 0, C.FRAME_WIDTH[0], base)
            b = fr["blocks"]
            label = _label_map(fr)
            # the unmutated census flavour, pair by pair (every block runs once, on fresh pixels)
            ref, coef = [p.copy() for p in fr["planes"]], fr["coef"].copy()
            cen.set_mutant(0)
            key = b["tx"].astype(int) * 32 + b["txtp"]
            for pr in C.PAIRS:
                cen.reset()
                oracle_lib.itx_frame(ref, b[key == pr[0] * 32 + pr[1]], coef, bpc, cen.lib)
                ctr[pr] = ctr.get(pr, 0) + cen.read()
            assert not coef.any()
            plain = oracle_lib.itx_frame([p.copy() for p in fr["planes"]], b, fr["coef"].copy(), bpc)
            assert np.array_equal(plain[0], ref[0]), "the census flavour without a mutant is the plain oracle"
            for m in MUTANTS:
                cen.set_mutant(cen.at["MUT_ITX_" + m])
                got = oracle_lib.itx_frame([p.copy() for p in fr["planes"]], b, fr["coef"].copy(), bpc, cen.lib)
                cen.set_mutant(0)
                assert (label[got[0] != ref[0]] >= 0).all()
                for k in np.unique(label[got[0] != ref[0]]):
                    kills[m].add((int(b["tx"][k]), int(b["txtp"][k])))
    finally:
        cen.set_mutant(0)
    return kills, ctr


def kill_masks(kills):
    return {m: tuple(sum(1 << t for (x, t) in kills[m] if x == tx) for tx in range(len(TX_DIMS))) for m in MUTANTS}


def n_pairs(kills, m):
    return len(kills[m] - {(0, C.WHT)})


def test_plain_oracle_holds_no_census():
    o = oracle_lib.load_oracle()
    for sym in ("oracle_census_ctr", "oracle_census_mutant", "oracle_census_reset", "oracle_census_read",
                "oracle_census_set_mutant", "oracle_census_layout"):
        with pytest.raises(AttributeError):
            getattr(o, sym)
    assert ctypes.c_int.in_dll(oracle_lib.load_census().lib, "oracle_census_mutant").value == 0


def test_pairs_and_patterns():
    assert len(C.PAIRS) == 156 and len(set(C.PAIRS)) == 156
    assert sorted(C.PAIRS[:-1]) == sorted((tx, t) for tx in range(19) for t in tx_types(tx))
    assert set(C.BASE_PATTERNS) <= set(C.PATTERNS) and len(C.BASE_PATTERNS) == 29
    for bpc in C.BPCS:
        lo, hi = C.cf_range(bpc)
        assert (lo, hi) == (-128 * 2 ** bpc, 128 * 2 ** bpc - 1)
        for tx, t in C.PAIRS:
            sw, sh = C.coded_dims(tx)
            for n in C.PATTERNS:
                c, eob = C.pattern(tx, t, bpc, n)
                c2, eob2 = C.pattern(tx, t, bpc, n)
                assert np.array_equal(c, c2) and eob == eob2, "a pure function of its arguments"
                assert c.shape == (sw * sh,) and lo <= c.min() and c.max() <= hi and c.any()
                assert 1 <= eob < sw * sh, "no block takes the DC path"
                if not n.startswith("imp"):
                    assert eob == sw * sh - 1
            full = np.abs(np.stack([C.pattern(tx, t, bpc, n)[0] for n in ("max", "min", "altx", "alty", "altxy",
                                                                         "rsign0", "match1_1", "matchn2_0")]))
            assert (full >= hi).all()
            d = C.pattern(tx, t, bpc, "altx")[0].reshape(sw, sh)
            assert (d[0] == hi).all() and (d[1] == lo).all()      # by x: d[x, y]
            d = C.pattern(tx, t, bpc, "alty")[0].reshape(sw, sh)
            assert (d[:, 0] == hi).all() and (d[:, 1] == lo).all()
        e = C.pattern(3, 0, bpc, "i16edge")[0]
        assert set(e) == ({32767, -32768} if bpc == 8 else {32767, -32768, 32768, -32769})
        assert set(C.pattern(3, 0, bpc, "i16fit")[0]) == {32767, -32768}
    # the matched pattern of an output carries the signs of that output's basis, so no input of
    # the range drives that output further (taking min as -max: |min| = max + 1)
    for tx, t in ((1, 0), (2, 3), (7, 6), (3, 9), (0, 16)):
        w, h = TX_DIMS[tx]
        hi = C.cf_range(10)[1]
        v = np.sign(C.pattern(tx, t, 10, "match1_1")[0].reshape(w, h).T).astype(np.float64) * hi   # [y, x]
        br = np.array([oracle_lib.itx_1d(C.ROW_KIND[t], w, np.eye(w, dtype=np.int32)[i] << 14) for i in range(w)]).T
        bc = np.array([oracle_lib.itx_1d(C.COL_KIND[t], h, np.eye(h, dtype=np.int32)[i] << 14) for i in range(h)]).T
        out = bc.astype(np.float64) @ v @ br.astype(np.float64).T
        reach = hi * np.abs(bc[h // 2]).sum() * np.abs(br[w // 2]).sum()
        assert out[h // 2, w // 2] == reach > 0


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("bpc", C.BPCS)
def test_directed_frame_holds_every_case(bpc, layout):
    fr = C.directed_frame(bpc, "zero", layout)
    b, cases = fr["blocks"], fr["cases"]
    names = {}
    for k in range(len(b)):
        tx, t, _, eob, name = cases[fr["case_of_block"][k]]
        assert (tx, t, eob) == (b["tx"][k], b["txtp"][k], b["eob"][k])
        names.setdefault((tx, t), []).append(name)
    for pr in C.PAIRS:
        got = [n for n in names[pr] if n != "dc"]
        assert sorted(got) == sorted(C.PATTERNS), pr
    dc = b[(b["txtp"] == 0) & (b["eob"] < 1)]
    lo, hi = C.cf_range(bpc)
    for tx in range(19):
        assert set(fr["coef"][dc["coef_off"][dc["tx"] == tx]]) == {lo, hi}, "DC-only blocks at both extremes"
    assert 4000 <= len(b) <= 7000
    nplanes = 1 if layout == 0 else 3
    assert set(b["plane"]) == set(range(nplanes))
    # inside their planes, no two on the same pixel, some ending at a right and at a bottom edge
    ss_hor, ss_ver = C._subsampling(layout)
    for p in range(nplanes):
        pw, ph = (fr["w"], fr["h"]) if p == 0 else ((fr["w"] + ss_hor) >> ss_hor, (fr["h"] + ss_ver) >> ss_ver)
        sel = b[b["plane"] == p]
        assert (sel["x"] + np.array(TX_DIMS)[sel["tx"], 0] <= pw).all()
        assert (sel["y"] + np.array(TX_DIMS)[sel["tx"], 1] <= ph).all()
        _label_map(dict(blocks=sel, planes=[fr["planes"][p]]))
    right, bottom = C.edge_blocks(fr)
    assert right > 0 and bottom > 0
    assert fr["w"] % 128 and sum(p.size for p in fr["planes"]) < 3 << 20


@pytest.mark.parametrize("bpc", C.BPCS)
def test_corner_shapes_in_both_arena_forms(bpc):
    seen = {}
    for tx, t, c, eob, (_, cw, ch, wide) in C.corner_cases(bpc):
        assert t in tx_types(tx) and eob >= 1
        packed, flags = pack_coefs(c, tx, bpc > 8)
        sw, sh = C.coded_dims(tx)
        if sw * sh <= 16 and not (flags & 0x40):
            assert flags == 0            # a 4x4 block is packed only as int16
        else:
            assert flags & 0x80 and (((flags >> 3) & 7) * 4 + 4, (flags & 7) * 4 + 4) == (cw, ch)
        assert bool(flags & 0x40) == (bpc > 8 and not wide), "MI_TX_I16 exactly when the corner fits int16"
        seen.setdefault(tx, set()).add((cw, ch, wide))
    for tx in range(19):
        forms = (False, True) if bpc > 8 else (False,)
        assert seen[tx] == {(cw, ch, f) for (cw, ch) in C.corner_shapes(tx) for f in forms}
    fr = C.directed_frame(bpc, "rand", 1, "corners", packed=True)
    fl = fr["blocks"]["flags"]
    assert (fl & 0x80).any() and (bpc == 8 or ((fl & 0x40).any() and ((fl & 0xc0) == 0x80).any()))


@pytest.mark.parametrize("bpc", C.BPCS)
def test_mutants_killed(bpc):
    """The kill table is the one written down, and holds the floors measured when the inputs were
    designed (base patterns, sed-made variants of oracle/itx.c)."""
    kills, ctr = analysis(bpc)
    cen = oracle_lib.load_census()
    total = sum(ctr.values())
    n = {m: n_pairs(kills, m) for m in MUTANTS}
    print(bpc, n, {c: cen.itx(total, c, bpc) for c in COUNTERS})
    assert kill_masks(kills) == KILLS[bpc]
    if bpc == 12:
        assert n["ROT_I32"] >= 104 and n["MID_I16"] == 155
        assert kills["RES_I16"] == {(tx, IDTX) for tx in (3, 9, 15)}      # IDTX on 32x32, 16x32, 8x32
        assert cen.itx(total, "ROT_GE_2P31", bpc) > 0 and cen.itx(total, "RES_GT_I16", bpc) > 0
    else:
        # the claim of itx_1d.h, on adversarial inputs: at 8 and 10 bits every product and
        # pair-sum fits 32 bits; and the residual fits int16
        assert n["ROT_I32"] == 0 and not kills["ROT_I32"] and cen.itx(total, "ROT_GE_2P31", bpc) == 0
        assert not kills["RES_I16"] and cen.itx(total, "RES_GT_I16", bpc) == 0
    assert n["NO_CLIP"] >= 114
    assert n["NO_MIDCLIP"] >= (33 if bpc == 8 else 116)
    # the lossless row result needs more than int16 from 10 bits on (18 bits at 10)
    assert ((0, C.WHT) in kills["WHT_MID_I16"]) == (bpc > 8)
    assert (cen.itx(total, "WHT_MID_GT_I16", bpc) > 0) == (bpc > 8)
    assert kills["WHT_MID_I16"] <= {(0, C.WHT)}


def clip_reachable(counter, tx, bpc):
    """Whether a clip can fire at all for a size. The hand-off clip cuts (row + rnd) >> s to the
    column range. A row kernel that clips its outputs leaves them in the row range
    [-2^(bpc+7), 2^(bpc+7) - 1] (8 bits: int16); adst4 and the identities do not clip.
      * 8 bits, both ranges int16: behind a clipped row the hand-off clip cannot fire. It fires
        only where an unclipped row kernel's gain (adst4 at most 2.68, identity4 1.41, identity8
        2, identity16 2.41, identity32 4; times 181/256 in 2:1 rectangles), halved s times, still
        exceeds 1: 4x4 (2.68), 4x8 (1.89), 8x4 (1.41), 32x16 (1.41), 4x16 (1.34), 16x4 (1.21).
        8x8 and 32x32 end at exactly 1, (2 * 32767 + 1) >> 1 = 32767, the rest below;
      * 10 and 12 bits, s = 2 (column range = row range >> 2): a clipped row's upper end gives
        (2^(bpc+7) - 1 + 2) >> 2 = 2^(bpc+5), one past the column range; its lower end gives
        exactly -2^(bpc+5), inside. 64x64, 16x64 and 64x16 have s = 2 and DCT_DCT alone
        (clipped), so their hand-off never clips at the lower end; 16x16, 32x32, 8x32 and 32x8
        reach it through identity rows, every other size has s < 2."""
    if counter in ("MID_CLIP_LO", "MID_CLIP_HI") and bpc == 8:
        return tx in (0, 5, 6, 10, 13, 14)
    if counter == "MID_CLIP_LO":
        return tx not in (4, 17, 18)
    return True


@pytest.mark.parametrize("bpc", C.BPCS)
def test_every_clip_fires_for_every_size(bpc):
    _, ctr = analysis(bpc)
    cen = oracle_lib.load_census()
    for c in COUNTERS[:8]:
        for tx in range(19):
            fired = any(cen.itx(ctr[p], c, bpc) for p in C.PAIRS if p[0] == tx)
            assert fired == clip_reachable(c, tx, bpc), (c, tx)


def test_fused_intra_frames_hold_every_pair_and_class():
    """The fused intra frames of the GPU test: all 19 sizes, and every (size, type) pair, WHT_WHT
    on 4x4 included, with a pattern of every class."""
    frames = C.intra_frames(10)
    dealt = set().union(*[d for _, _, d in frames])
    assert {tx for tx, _, _ in dealt} == set(range(19))
    for pr in C.PAIRS:
        assert {C.pattern_class(n) for tx, t, n in dealt if (tx, t) == pr} == set(C.CLASSES), pr
    assert {C.pattern_class(n) for n in C.PATTERNS} == set(C.CLASSES)
    for fr, _, _ in frames:
        tb = fr["tx_blocks"]
        assert ((tb["eob"] >= 1) & (tb["txtp"] <= C.WHT)).all(), "no block is left on the DC path"
