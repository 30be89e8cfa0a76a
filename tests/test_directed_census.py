"""CPU: the directed inputs of tests/directed_filters.py reach what they claim to reach.

The census flavour of the oracle (oracle/census.h) counts, over the directed frames of one bit
depth and layout, how often every decision of the three in-loop filters is taken and how often
it sits at its limit. The minimums below are conditions on the inputs; no cell is excused. The
same flavour can flip one decision at a time: every such mutant must change at least one pixel
of the directed frames, which is what makes the GPU comparisons over them worth something.
"""
import functools

import numpy as np
import pytest

from tests import directed_filters as D
from tests import oracle_lib
from tests.test_oracle_lf import pad_planes

LF_BRANCHES = ("unfiltered", "narrow_hev", "narrow", "6tap", "8tap", "13tap")
LF_CMPS = ("I_p1p0", "I_q1q0", "E", "I_p2p1", "I_q2q1", "I_p3p2", "I_q3q2", "Fo_p6", "Fo_p5", "Fo_p4", "Fo_q4",
           "Fo_q5", "Fo_q6", "Fi_p2", "Fi_p1", "Fi_q1", "Fi_q2", "Fi_p3", "Fi_q3", "H_p", "H_q")
LF_CLIPS = ("d_lo", "d_hi", "f_lo", "f_hi", "f4_max", "f3_max", "out_lo", "out_hi")
LF_WIDTHS = (4, 6, 8, 16)


def lf_reach(cls, wd):
    """Branches and comparisons the filter can reach at one plane class and width."""
    br = [0, 1, 2] + ([3] if wd == 6 else []) + ([4] if wd >= 8 else []) + ([5] if wd == 16 else [])
    cmp_ = [0, 1, 2, 19, 20]
    if wd >= 6:
        cmp_ += [3, 4, 13, 14, 15, 16]
    if wd >= 8:
        cmp_ += [5, 6, 17, 18]
    if wd == 16:
        cmp_ += [7, 8, 9, 10, 11, 12]
    return br, sorted(cmp_)


def lf_cells_of(layout):
    return [(d, cls, wd) for d in (0, 1) for cls in ((0, 1) if layout else (0,))
            for wd in ((4, 8, 16) if cls == 0 else (4, 6))]


def run_lf(bpc, layout, seed, lib=None):
    planes, lf, w, h, sb128 = D.lf_directed(bpc, layout, seed)
    out = oracle_lib.deblock_frame(pad_planes(planes, w, h, bpc, layout), bpc, layout, w, h, lf, sb128=sb128,
                                   lib=lib)
    return [o[:p.shape[0], :p.shape[1]] for o, p in zip(out, planes)]


@functools.lru_cache(maxsize=None)
def lf_census(bpc, layout):
    c = oracle_lib.load_census()
    c.set_mutant(0)
    c.reset()
    for seed in range(len(D.LF_SEEDS)):
        run_lf(bpc, layout, seed, c.lib)
    return c.lf_cells(c.read())


def lf_shortfalls(cells, layout, at):
    """Every (cell, event, count, minimum) of the deblock census below its minimum."""
    bad = []
    for d, cls, wd in lf_cells_of(layout):
        c = cells[d, cls, LF_WIDTHS.index(wd)]
        name = f"dir{d} {'chroma' if cls else 'luma'} wd{wd}"
        br, cmps = lf_reach(cls, wd)
        for b in br:
            if c[at["LF_CELL_BRANCH"] + b] < 32:
                bad.append((name, "branch " + LF_BRANCHES[b], int(c[at["LF_CELL_BRANCH"] + b]), 32))
        for k in cmps:
            for off, what in ((at["LF_CELL_AT"], "at limit"), (at["LF_CELL_AT1"], "at limit + 1")):
                if c[off + k] < 8:
                    bad.append((name, f"{LF_CMPS[k]} {what}", int(c[off + k]), 8))
        for i, x in enumerate(br):
            for y in br[i + 1:]:
                n = c[at["LF_CELL_PAIR"] + x * len(LF_BRANCHES) + y]
                if n < 4:
                    bad.append((name, f"pair {LF_BRANCHES[x]}/{LF_BRANCHES[y]}", int(n), 4))
        for b in br:
            if b >= 3:
                for off, what in ((at["LF_CELL_PIN_LO"], "pinned at 0"), (at["LF_CELL_PIN_HI"], "pinned at bdmax")):
                    if c[off + b] < 32:
                        bad.append((name, f"{LF_BRANCHES[b]} {what}", int(c[off + b]), 32))
        for k, what in enumerate(LF_CLIPS):
            if c[at["LF_CELL_CLIP"] + k] < 1:
                bad.append((name, "clip " + what, 0, 1))
    return bad


@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("bpc", D.BPCS)
def test_deblock_census_minimums(bpc, layout):
    """Per direction, plane class and width: every reachable branch on 32 lines, every deciding
    comparison 8 times at its limit and 8 times one past it, every pair of distinct branches on
    4 line pairs, every smoother 32 times on lines pinned at 0 and at bdmax, and every clip of
    the narrow filter and of its outputs at least once."""
    bad = lf_shortfalls(lf_census(bpc, layout), layout, oracle_lib.load_census().at)
    assert not bad, "\n".join(f"{n}: {e}: {v} < {m}" for n, e, v, m in bad)


# ---------------------------------------------------------------------------------------
# CDEF
# ---------------------------------------------------------------------------------------

def run_cdef(bpc, layout, seed, lib=None):
    planes, masks, cd, w, h = D.cdef_directed(bpc, layout, seed)
    out = oracle_lib.cdef_frame(pad_planes(planes, w, h, bpc, layout), bpc, layout, w, h, masks, cd, lib=lib)
    return [o[:p.shape[0], :p.shape[1]] for o, p in zip(out, planes)]


@functools.lru_cache(maxsize=None)
def cdef_census(bpc, layout):
    c = oracle_lib.load_census()
    c.set_mutant(0)
    c.reset()
    for seed in range(len(D.CDEF_SEEDS)):
        run_cdef(bpc, layout, seed, c.lib)
    return c.read()


@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("bpc", D.BPCS)
def test_cdef_census_minimums(bpc, layout):
    """64 direction searches tie a proper subset of the directions, with four distinct winners
    and not direction 0 alone; the clamp changes 1% of the pixels filtered with both strengths;
    the sentinel, the negative rounding, both output bounds and (with chroma) the cut
    pri_shift occur."""
    at = oracle_lib.load_census().at
    c = cdef_census(bpc, layout)
    ties = c[at["CDEF_TIES"]:at["CDEF_TIES"] + 9]
    sub = c[at["CDEF_WIN_SUBTIE"]:at["CDEF_WIN_SUBTIE"] + 8]
    # ties between a proper subset of the directions: there the merge order decides
    assert ties[2:8].sum() >= 64, ties
    assert np.count_nonzero(sub) >= 4 and sub[1:].sum() > 0, sub
    assert ties[8] > 0 and c[at["CDEF_VAR0"]] > 0                      # flat blocks
    assert c[at["CDEF_PX_CLAMPED"]] * 100 >= c[at["CDEF_PX_BOTH"]] > 0, (c[at["CDEF_PX_CLAMPED"]], c[at["CDEF_PX_BOTH"]])
    for name in ("CDEF_PX_SENTINEL", "CDEF_PX_NEG", "CDEF_PX_OUT0", "CDEF_PX_OUTMAX"):
        assert c[at[name]] > 0, name
    # pri_shift = max(0, damping - ulog2(pri)) is cut only on chroma: luma has damping >= 3 + (bpc - 8)
    # from the header and pri <= 15 << (bpc - 8), so the difference is never negative; chroma
    # filters with damping - 1 and reaches -1 at header damping 3 and a primary strength >= 8.
    if layout:
        assert c[at["CDEF_PX_PRISHIFT0"]] > 0
    else:
        assert c[at["CDEF_PX_PRISHIFT0"]] == 0


def test_cdef_inputs_cover_the_stated_parameters():
    pri, sec, damp, unset_edge = set(), set(), set(), False
    for seed in range(len(D.CDEF_SEEDS)):
        planes, masks, cd, w, h = D.cdef_directed(10, 1, seed)
        assert w <= 256 and h <= 192
        for s in list(cd["y_strength"]) + list(cd["uv_strength"]):
            pri.add(int(s) >> 2)
            sec.add(int(s) & 3)
        damp.add(cd["damping"])
        unset_edge |= bool((masks["cdef_idx"][0] == -1).any())
        assert (masks["cdef_idx"] == -1).any() and (masks["noskip_mask"] != 0xFFFF).any()
    assert {1, 15} <= pri and sec == {0, 1, 2, 3} and {3, 6} <= damp and unset_edge
    assert any(h % 8 and ((h + 1) >> 1) % 2 for _, h, _ in D.CDEF_SEEDS)


# ---------------------------------------------------------------------------------------
# Loop restoration
# ---------------------------------------------------------------------------------------

def run_lr(bpc, layout, seed, lib=None):
    c, d, lr, w, h = D.lr_directed(bpc, layout, seed)
    out = oracle_lib.lr_frame(pad_planes(c, w, h, bpc, layout), pad_planes(d, w, h, bpc, layout), bpc, layout,
                              w, h, lr, lib=lib)
    return [o[:p.shape[0], :p.shape[1]] for o, p in zip(out, c)]


@functools.lru_cache(maxsize=None)
def lr_census(bpc, layout):
    c = oracle_lib.load_census()
    c.set_mutant(0)
    c.reset()
    for seed in range(len(D.LR_SEEDS)):
        run_lr(bpc, layout, seed, c.lib)
    return c.read()


@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("bpc", D.BPCS)
def test_lr_census_minimums(bpc, layout):
    """All four Wiener clips, z = 0 and z >= 255 at both radii, the two u32 products past 2^31
    where arithmetic allows, both output clips, and all 16 sets and Wiener units on luma and on
    chroma."""
    at = oracle_lib.load_census().at
    c = lr_census(bpc, layout)
    for name in ("WIENER_HCLIP_LO", "WIENER_HCLIP_HI", "WIENER_VCLIP_LO", "WIENER_VCLIP_HI", "SGR_OUT_LO",
                 "SGR_OUT_HI"):
        assert c[at[name]] > 0, name
    for r in (0, 1):                                     # radius 2 (5x5, n = 25), radius 1 (3x3, n = 9)
        assert c[at["SGR_Z0"] + r] > 0 and c[at["SGR_Z255"] + r] > 0
    # p * s >= 2^31. p = a * n - b * b on samples scaled to 8 bits is largest with k of the n samples
    # at 255 and the rest at 0: 255^2 * k * (n - k). Radius 1: 255^2 * 20 * 3236 = 4.21e9, reachable at
    # every bit depth (and below 2^32). Radius 2: 255^2 * 156 * 140 = 1.42e9 < 2^31, never.
    assert c[at["SGR_PS31"] + 1] > 0 and c[at["SGR_PS31"] + 0] == 0
    # x * sum * one_by_x >= 2^31 needs 12 bits: 255 * 25 * 4095 * 164 = 4.28e9 and 255 * 9 * 4095 * 455 =
    # 4.28e9, against 255 * 25 * 1023 * 164 = 1.07e9 at 10 bits.
    for r in (0, 1):
        assert (c[at["SGR_XSUM31"] + r] > 0) == (bpc == 12), (r, c[at["SGR_XSUM31"] + r])
    sets = c[at["LR_SET"]:at["LR_SET"] + 48].reshape(3, 16)
    wien = c[at["LR_WIENER"]:at["LR_WIENER"] + 3]
    assert (sets[0] > 0).all() and wien[0] > 0
    if layout:
        assert ((sets[1] + sets[2]) > 0).all() and wien[1] + wien[2] > 0


@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_lr_inputs_cover_the_stated_parameters(layout):
    """The corners of the codable Wiener taps and both ends of the self-guided weights, on luma
    and on chroma, over the frames of one bit depth; D far from C."""
    lo, hi = (-5, -23, -17), (10, 8, 46)
    for cls in ((0, 1) if layout else (0,)):
        taps, weights = set(), {}
        for seed in range(len(D.LR_SEEDS)):
            c, d, lr, w, h = D.lr_directed(10, layout, seed)
            assert w <= 384 and h <= 256 and lr["unit_size_log2"] == (6, 5 if layout == 1 else 6)
            assert np.mean(np.abs(c[0].astype(int) - d[0].astype(int))) > 1023 / 8
            u = lr["lr_mask"]["lr"][:, :, [0] if cls == 0 else [1, 2], :].reshape(-1)
            for un in u:
                if un["type"] == 2:
                    taps.add((tuple(int(v) for v in un["filter_h"]), tuple(int(v) for v in un["filter_v"])))
                else:
                    weights.setdefault(int(un["type"]) - 3, set()).add(tuple(int(v) for v in un["sgr_weights"]))
        z = (lambda t: t) if cls == 0 else (lambda t: (0,) + t[1:])
        assert {(z(lo), z(lo)), (z(hi), z(hi)), (z(lo), z(hi)), (z(hi), z(lo))} <= taps
        assert sorted(weights) == list(range(16))
        for i, ws in weights.items():
            # sets 10-13 have no 5x5 pass and code no w0, sets 14-15 no 3x3 pass and no w1
            assert {w0 for w0, _ in ws} >= ({-96, 31} if i < 10 or i >= 14 else {0}), (i, ws)
            assert {w1 for _, w1 in ws} >= ({-32, 95} if i < 14 else {95}), (i, ws)


# ---------------------------------------------------------------------------------------
# The two flavours agree; every mutant shows
# ---------------------------------------------------------------------------------------

RUNNERS = (("deblock", run_lf, len(D.LF_SEEDS)), ("cdef", run_cdef, len(D.CDEF_SEEDS)),
           ("lr", run_lr, len(D.LR_SEEDS)))


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("bpc", D.BPCS)
def test_census_flavour_matches_plain_oracle(bpc, layout):
    """liboracle_census.so without a mutant gives liboracle.so's pixels on every directed frame."""
    c = oracle_lib.load_census()
    c.set_mutant(0)
    for name, run, n in RUNNERS:
        for seed in range(n):
            assert same(run(bpc, layout, seed), run(bpc, layout, seed, c.lib)), (name, seed)


# mutant number -> (stage, description); oracle/census.h
MUTANTS = {1 + k: ("deblock", f"{n} <= taken as <") for k, n in enumerate(LF_CMPS[:19])}
MUTANTS.update({
    20: ("deblock", "|p1 - p0| > H taken as >="), 21: ("deblock", "|q1 - q0| > H taken as >="),
    22: ("deblock", "8-tap sums cut to int16"), 23: ("deblock", "13-tap sums cut to int16"),
    24: ("cdef", "direction tie-break >="), 25: ("cdef", "clamp removed"),
    26: ("cdef", "sentinel joins the minimum"),
    27: ("lr", "Wiener horizontal lower clip removed"), 28: ("lr", "Wiener horizontal upper clip removed"),
    29: ("lr", "p * s as int32"), 30: ("lr", "x * sum * one_by_x as int32"),
})


def mutant_can_show(m, bpc):
    """Mutants that arithmetic makes equivalent to the original at some bit depth."""
    if m == 22:
        return False          # the 8-tap sums reach 8 * 4095 + 4 = 32764 < 2^15 at most: they fit
    if m == 23:
        return bpc == 12      # 16 * 1023 + 8 = 16376 fits, 16 * 4095 + 8 = 65528 does not
    if m == 30:
        return bpc == 12      # see test_lr_census_minimums
    return True


def mutant_detected(m, bpc, layout):
    stage = MUTANTS[m][0]
    c = oracle_lib.load_census()
    _, run, n = next(r for r in RUNNERS if r[0] == stage)
    try:
        for seed in range(n):
            c.set_mutant(0)
            ref = run(bpc, layout, seed, c.lib)
            c.set_mutant(m)
            if not same(ref, run(bpc, layout, seed, c.lib)):
                return True
        return False
    finally:
        c.set_mutant(0)


@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("bpc", D.BPCS)
def test_every_mutant_changes_a_pixel(bpc, layout):
    """Each single-decision mutant of the oracle differs from it in at least one pixel of the
    directed frames of this bit depth and layout, and the mutants that arithmetic makes
    equivalent (mutant_can_show) in none: the sums they cut do fit."""
    # every in-loop filter mutant: the numbers below the first inverse-transform mutant (those
    # are tests/test_itx_cases.py's)
    assert sorted(MUTANTS) == list(range(1, oracle_lib.load_census().at["MUT_ITX_ROT_I32"]))
    wrong = [(m, MUTANTS[m][1]) for m in MUTANTS if mutant_detected(m, bpc, layout) != mutant_can_show(m, bpc)]
    assert not wrong, wrong
