#!/usr/bin/env python3
"""What the in-loop filter tests reach, measured on the CPU by the census flavour of the oracle
(oracle/census.h): the random frames of tests/test_lf_gpu.py, test_cdef_gpu.py and
test_lr_gpu.py (their small cases) next to the directed frames of tests/directed_filters.py.
Nothing here is asserted; tests/test_directed_census.py asserts the directed column.

    python tools/filter_census.py > profiles/filter_census.md
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rav1d_amd.synth import add_cdef_meta, make_lr_meta  # noqa: E402
from tests import directed_filters as D  # noqa: E402
from tests import oracle_lib  # noqa: E402
from tests import test_directed_census as T  # noqa: E402
from tests.test_oracle_lf import frame, pad_planes  # noqa: E402
from tests.test_oracle_lr import planes_for  # noqa: E402


def crop(out, planes):
    return [o[:p.shape[0], :p.shape[1]] for o, p in zip(out, planes)]


# ---- the random frames, as the GPU tests build them ------------------------------------

def random_lf(bpc, layout, k, lib=None):
    w, h = ((256, 192), (200, 136))[k]
    planes, lf = frame(w, h, bpc, layout, seed=bpc * 7 + layout)
    planes = planes[:1] if layout == 0 else planes
    return crop(oracle_lib.deblock_frame(pad_planes(planes, w, h, bpc, layout), bpc, layout, w, h, lf,
                                         sb128=int(w == 256), lib=lib), planes)


def random_cdef(bpc, layout, k, lib=None):
    w, h = ((256, 192), (200, 134))[k]
    seed = bpc * 13 + layout + h
    planes, lf = frame(w, h, bpc, layout, seed)
    planes = planes[:1] if layout == 0 else planes
    cd = add_cdef_meta(lf, np.random.default_rng(seed + 99))
    return crop(oracle_lib.cdef_frame(pad_planes(planes, w, h, bpc, layout), bpc, layout, w, h, lf["masks"], cd,
                                      lib=lib), planes)


def random_lr(bpc, layout, k, lib=None):
    w, h, sb128, ul = ((256, 200, 1, None), (200, 150, 0, (6, 5)), (330, 260, 0, (7, 6)))[k]
    if ul is not None and layout != 1:
        ul = (ul[0], ul[0])
    rng = np.random.default_rng(bpc * 31 + layout + w)
    c = planes_for(w, h, bpc, layout, rng)
    d = planes_for(w, h, bpc, layout, rng)
    lr = make_lr_meta(w, h, layout, rng, sb128=sb128, unit_log2=ul)
    return crop(oracle_lib.lr_frame(pad_planes(c, w, h, bpc, layout), pad_planes(d, w, h, bpc, layout), bpc, layout,
                                    w, h, lr, lib=lib), c)


SOURCES = {
    "random": {"deblock": (random_lf, 2), "cdef": (random_cdef, 2), "lr": (random_lr, 3)},
    "directed": {"deblock": (T.run_lf, len(D.LF_SEEDS)), "cdef": (T.run_cdef, len(D.CDEF_SEEDS)),
                 "lr": (T.run_lr, len(D.LR_SEEDS))},
}


def census(run, n, bpc, layout):
    c = oracle_lib.load_census()
    c.set_mutant(0)
    c.reset()
    for k in range(n):
        run(bpc, layout, k, c.lib)
    return c.read()


def undetected(src, bpc):
    """Mutants that change no pixel of any frame of one bit depth, all layouts together."""
    c = oracle_lib.load_census()
    out = []
    for m, (stage, what) in T.MUTANTS.items():
        run, n = SOURCES[src][stage]
        hit = False
        for layout in D.LAYOUTS:
            for k in range(n):
                c.set_mutant(0)
                ref = run(bpc, layout, k, c.lib)
                c.set_mutant(m)
                hit = hit or not T.same(ref, run(bpc, layout, k, c.lib))
                if hit:
                    break
            if hit:
                break
        c.set_mutant(0)
        if not hit and T.mutant_can_show(m, bpc):
            out.append(f"{m} ({what})")
    return out


def main():
    at = oracle_lib.load_census().at
    print("# In-loop filter census: random test frames against directed frames\n")
    print("Written by `tools/filter_census.py`; counts come from the census flavour of the oracle on the CPU.")
    print("Random: the 256x192 / 200x136 deblock, 256x192 / 200x134 CDEF and three small restoration cases of")
    print("the GPU parity tests, per bit depth and layout. Directed: `tests/directed_filters.py`. Deblock counts")
    print("are lines, CDEF counts searches or pixels, restoration counts samples.\n")
    for stage in ("deblock", "cdef", "lr"):
        print(f"## {stage}\n")
        if stage == "deblock":
            print("Cells are (direction, plane class, width); `short` counts the reachable entries of a kind that stay")
            print("below the minimum of tests/test_directed_census.py (32 lines per branch, 8 per comparison at its")
            print("limit and 8 one past it, 4 line pairs per pair of branches, 32 pinned lines per smoother, 1 per clip).\n")
            print("| bpc | layout | input | branch cells short | comparisons short | branch pairs short | "
                  "pinned short | clips never hit | 13-tap lines | 8-tap lines from a 16 edge |")
            print("|---|---|---|---|---|---|---|---|---|---|")
        elif stage == "cdef":
            print("| bpc | layout | input | searches | all 8 tie | 2-7 tie | winners of 2-7 ties | clamp changed / both "
                  "strengths | sentinel px | pri_shift cut px | out 0 / bdmax px |")
            print("|---|---|---|---|---|---|---|---|---|---|---|")
        else:
            print("| bpc | layout | input | Wiener h clip lo / hi | v clip lo / hi | z = 0 (r2 / r1) | z >= 255 | "
                  "p*s >= 2^31 | x*sum*1/x >= 2^31 | sgr out clip lo / hi | sets missing luma / chroma |")
            print("|---|---|---|---|---|---|---|---|---|---|---|")
        for bpc in D.BPCS:
            for layout in D.LAYOUTS:
                for src in ("random", "directed"):
                    run, n = SOURCES[src][stage]
                    c = census(run, n, bpc, layout)
                    if stage == "deblock":
                        cells = oracle_lib.load_census().lf_cells(c)
                        bad = T.lf_shortfalls(cells, layout, at)
                        kinds = [sum(1 for b in bad if b[1].startswith(k)) for k in ("branch", ("I_", "E ", "F", "H_"), "pair")]
                        pinned = sum(1 for b in bad if "pinned" in b[1])
                        clips = sum(1 for b in bad if b[1].startswith("clip"))
                        wide = cells[:, 0, 3]
                        print(f"| {bpc} | {layout} | {src} | {kinds[0]} | {kinds[1]} | {kinds[2]} | {pinned} | {clips} | "
                              f"{int(wide[:, at['LF_CELL_BRANCH'] + 5].sum())} | {int(wide[:, at['LF_CELL_BRANCH'] + 4].sum())} |")
                    elif stage == "cdef":
                        g = lambda name, k=1: c[at[name]:at[name] + k]
                        ties = g("CDEF_TIES", 9)
                        sub = g("CDEF_WIN_SUBTIE", 8)
                        print(f"| {bpc} | {layout} | {src} | {int(ties.sum())} | {int(ties[8])} | {int(ties[2:8].sum())} | "
                              f"{[int(i) for i in np.nonzero(sub)[0]]} | {int(g('CDEF_PX_CLAMPED')[0])} / {int(g('CDEF_PX_BOTH')[0])} | "
                              f"{int(g('CDEF_PX_SENTINEL')[0])} | {int(g('CDEF_PX_PRISHIFT0')[0])} | "
                              f"{int(g('CDEF_PX_OUT0')[0])} / {int(g('CDEF_PX_OUTMAX')[0])} |")
                    else:
                        g = lambda name, k=1: [int(v) for v in c[at[name]:at[name] + k]]
                        sets = c[at["LR_SET"]:at["LR_SET"] + 48].reshape(3, 16)
                        miss_c = int(((sets[1] + sets[2]) == 0).sum()) if layout else "-"
                        print(f"| {bpc} | {layout} | {src} | {g('WIENER_HCLIP_LO')[0]} / {g('WIENER_HCLIP_HI')[0]} | "
                              f"{g('WIENER_VCLIP_LO')[0]} / {g('WIENER_VCLIP_HI')[0]} | {g('SGR_Z0', 2)} | {g('SGR_Z255', 2)} | "
                              f"{g('SGR_PS31', 2)} | {g('SGR_XSUM31', 2)} | {g('SGR_OUT_LO')[0]} / {g('SGR_OUT_HI')[0]} | "
                              f"{int((sets[0] == 0).sum())} / {miss_c} |")
        print()
    print("## mutants\n")
    print("Single-decision mutants of the oracle (oracle/census.h) that change no pixel of any frame of a bit depth.")
    print("Mutants that arithmetic makes equivalent at that depth are left out: the 8-tap sums cut to int16 (never")
    print("past 32764), the 13-tap sums cut to int16 and x*sum*one_by_x read as int32 below 12 bits.\n")
    print("| bpc | input | undetected |")
    print("|---|---|---|")
    for bpc in D.BPCS:
        for src in ("random", "directed"):
            u = undetected(src, bpc)
            print(f"| {bpc} | {src} | {'; '.join(u) if u else 'none'} |")


if __name__ == "__main__":
    main()
