"""Directed inputs for the three in-loop filters: deblock, CDEF and loop restoration.

The synthetic textures of rav1d_amd.synth feed the filters one kind of content (a sine base,
small noise, mid-grey flats). The frames here are built the other way round: from the
decisions the filters take. Every comparison is placed at its limit and one past it, flat
runs sit at 0, at bdmax and mid-range, neighbouring lines of a 4-line unit take different
branches, and the restoration units carry the corner taps and all sixteen self-guided sets
over 0/bdmax stripes. tests/test_directed_census.py holds the conditions these inputs must
meet, measured by the census flavour of the oracle; the GPU tests then ask for the same
pixels from every device route.

Each input is a pure function of (bit depth, layout, seed).
"""
import functools

import numpy as np

from rav1d_amd.synth import (AV1FILTER_DTYPE, AV1RESTORATION_DTYPE, RESTORATION_SGRPROJ, RESTORATION_WIENER,
                             SGR_PARAMS, TX_BY_DIMS, _unit_maps, calc_eih, make_lf_meta)

BPCS = (8, 10, 12)
LAYOUTS = (1, 2, 3, 0)      # 4:2:0, 4:2:2, 4:4:4, monochrome


def subsampling(layout):
    return (1 if layout in (1, 2) else 0), (1 if layout == 1 else 0)


def plane_dims(w, h, layout):
    ss_hor, ss_ver = subsampling(layout)
    dims = [(w, h)]
    if layout:
        dims += [((w + ss_hor) >> ss_hor, (h + ss_ver) >> ss_ver)] * 2
    return dims


def px_dtype(bpc):
    return np.uint16 if bpc > 8 else np.uint8


# =======================================================================================
# Deblock
# =======================================================================================
# (size, which edge direction the content is written for, sharpness). Direction 0 frames give
# every row a profile across the column edges; direction 1 frames give every column a profile
# across the row edges. Column edges are filtered first, so a direction 1 frame keeps them
# sparse (wide, flat transform blocks) and, on luma, at level 0.
LF_SEEDS = ((256, 192, 0, 0), (200, 136, 1, 0), (200, 136, 0, 7), (256, 192, 1, 7),
            (232, 168, 0, 0), (232, 168, 1, 0))
LF_LEVELS = (0, 1, 2, 3, 7, 14, 22, 31, 45, 63, 63, 16)
# transform shapes (along the edge normal, along the edge) per filter width index
_LF_SHAPES_LUMA = ((4, 16), (8, 32), (16, 64))
_LF_SHAPES_CHROMA = ((4, 16), (8, 32))


def _lf_tiling(pw, ph, direction, shapes, region, phase):
    """Regions of `region` x `region` pixels, each filled with one transform shape, narrow
    across the edges of `direction` and long along them; what does not fit becomes 4x4."""
    blocks = []
    for ry, y0 in enumerate(range(0, ph, region)):
        for rx, x0 in enumerate(range(0, pw, region)):
            a, b = shapes[(rx + 2 * ry + phase) % len(shapes)]
            a, b = min(a, region), min(b, region)
            tw, th = (a, b) if direction == 0 else (b, a)
            for y in range(y0, min(y0 + region, ph), th):
                for x in range(x0, min(x0 + region, pw), tw):
                    if x + tw <= pw and y + th <= ph:
                        blocks.append((x, y, TX_BY_DIMS[(tw, th)]))
                    else:
                        blocks += [(xx, yy, 0) for yy in range(y, min(y + th, ph), 4)
                                   for xx in range(x, min(x + tw, pw), 4)]
    return blocks


def _solve_e(target, i_lim):
    """d0 = |p0 - q0| and d1 = |p1 - q1| with 2 * d0 + (d1 >> 1) == target and |d1 - d0| within
    what the two I tests allow; the pair with the smallest |d1 - d0|."""
    best = None
    for d0 in range(target // 2 + 1):
        r = target - 2 * d0
        for d1 in (2 * r, 2 * r + 1):
            if abs(d1 - d0) <= 2 * i_lim and (best is None or abs(d1 - d0) < abs(best[1] - best[0])):
                best = (d0, d1)
    return best


@functools.lru_cache(maxsize=None)
def _lf_profiles(wd, half, level, sharp, bpc):
    """Line profiles across one edge of width `wd`: int array [K, 2 * half], each row
    p[half-1] .. p0 q0 .. q[half-1]. K is a multiple of 4 and rows (2j, 2j + 1) are meant to
    take different branches: a 4-line unit takes four consecutive rows."""
    bdm8 = bpc - 8
    bdmax = (1 << bpc) - 1
    F = 1 << bdm8
    e, i = calc_eih(sharp)
    E, I, H = int(e[level]) << bdm8, int(i[level]) << bdm8, (level >> 4) << bdm8
    mid = bdmax // 2
    rows = []
    serial = [level]

    def base():
        """Flat runs at 0, at bdmax and mid-range in turn; deltas point into the range."""
        serial[0] += 1
        return ((0, 1), (bdmax, -1), (mid, 1))[serial[0] % 3]

    def row(p0, q0, dp=(), dq=()):
        P, Q = [p0] * half, [q0] * half
        for k, v in dp:
            if k < half:
                P[k] = p0 + v
        for k, v in dq:
            if k < half:
                Q[k] = q0 + v
        rows.append(P[::-1] + Q)

    def tail(j, v):
        return tuple((k, v) for k in range(j, half))

    n_i = 1 if wd == 4 else 2 if wd == 6 else 3          # tap pairs under the I test
    n_fi = 0 if wd == 4 else 2 if wd == 6 else 3         # samples under the inner flat test

    def breaker(sg):
        """A far sample more than F from its p0/q0 with every neighbour step within I."""
        return () if wd == 4 else tail(2, sg * (F + 1))

    # --- branch makers -----------------------------------------------------------------
    def mk_none():
        d0 = min(E // 2 + 1, bdmax - mid)
        row(mid, mid + d0)

    def mk_hev():
        b, sg = base()
        d = max(H, F) + 1
        row(b, b + sg * F, dp=tail(1, sg * d))

    def mk_narrow():
        b, sg = base()
        row(b, b + sg * 2 * F, dp=breaker(sg))

    def mk_smooth(outer_break):
        b, sg = base()
        row(b, b + sg * F, dq=tail(5, sg * (F + 1)) if outer_break else ())

    makers = {"none": mk_none, "hev": mk_hev, "narrow": mk_narrow,
              "inner": lambda: mk_smooth(wd == 16), "outer": lambda: mk_smooth(False)}
    reach = ["none", "hev", "narrow"] + (["inner"] if wd >= 6 else []) + (["outer"] if wd == 16 else [])

    # --- every comparison at its limit (0) and one past it (1), next to another branch -----
    def emit_pair(fn, at):
        fn(at)
        makers[reach[(len(rows) // 2 + at) % len(reach)]]()

    for at in (0, 1):
        for j in range(n_i):                              # I tests, both sides
            for side in (0, 1):
                def f(at, j=j, side=side):
                    b, sg = base()
                    d = tail(j + 1, sg * (I + at))
                    row(b, b, dp=d if side == 0 else (), dq=d if side else ())
                emit_pair(f, at)

        def fe(at):                                       # E test
            sol = _solve_e(E + at, I)
            if sol is None:
                return mk_none()
            d0, d1 = sol
            extra = d1 - d0
            a = extra // 2
            p0 = mid + d0 // 2
            q0 = p0 - d0
            row(p0, q0, dp=tail(1, a), dq=tail(1, -(extra - a)))
        emit_pair(fe, at)

        for j in range(1, n_fi + 1):                      # inner flat tests
            for side in (0, 1):
                def f(at, j=j, side=side):
                    b, sg = base()
                    d = ((j, sg * (F + at)),)
                    step = sg * F * (len(rows) // 2 % 2)
                    row(b, b + step, dp=d if side == 0 else (), dq=d if side else ())
                emit_pair(f, at)
        if wd == 16:                                      # outer flat tests
            for j in (4, 5, 6):
                for side in (0, 1):
                    def f(at, j=j, side=side):
                        b, sg = base()
                        d = ((j, sg * (F + at)),)
                        step = sg * F * (len(rows) // 2 % 2)
                        row(b, b + step, dp=d if side == 0 else (), dq=d if side else ())
                    emit_pair(f, at)
        for side in (0, 1):                               # the two hev tests
            def f(at, side=side):
                b, sg = base()
                d = tail(1, sg * (H + at))
                brk = breaker(sg)
                step = sg * min(E // 4, 8 * F)
                row(b, b + step, dp=d if side == 0 else brk, dq=d if side else brk)
            emit_pair(f, at)

    # --- the narrow filter's clips -------------------------------------------------------
    for sg in (1, -1):
        d0 = 43 * F                                       # 3 * d0 passes 128 * F: f, f + 4, f + 3 cut
        row(mid - sg * d0 // 2, mid - sg * d0 // 2 + sg * d0, dp=breaker(1))
        makers[reach[len(rows) // 2 % len(reach)]]()
        # hev: p1 - q1 beyond +-128 * F
        d0 = 2 * F
        a = min(I, 63 * F)
        row(mid + sg * d0 // 2, mid - sg * d0 // 2, dp=tail(1, sg * a), dq=tail(1, -sg * a))
        makers[reach[len(rows) // 2 % len(reach)]]()
    d = 4 * F + 1
    row(bdmax, bdmax, dq=tail(1, -d))                     # p0 + f2 past bdmax
    row(0, 0, dp=tail(1, d))                              # q0 - f1 below 0
    row(bdmax - F, bdmax, dp=breaker(-1))                 # no hev: q0 - f1, p1 + f near bdmax
    row(F, 0, dp=breaker(1))

    # --- every unordered pair of distinct branches on lines (0, 1) or (2, 3) ------------------
    for x in range(len(reach)):
        for y in range(x + 1, len(reach)):
            makers[reach[x]]()
            makers[reach[y]]()
    while len(rows) % 4:
        makers[reach[len(rows) % len(reach)]]()
    return np.clip(np.array(rows, np.int64), 0, bdmax)


def _lf_paint(view, starts, size_log, level, cap, sharp, bpc):
    """Write profiles across every edge of one direction. view[line, along]; starts, size_log
    and level are per 4x4 unit in the same orientation."""
    n_line4, n_along4 = starts.shape
    l4, a4 = np.nonzero(starts[:, 1:])
    a4 = a4 + 1
    k = np.minimum(np.minimum(size_log[l4, a4 - 1], size_log[l4, a4]), cap)
    half = (4 << np.minimum(size_log[l4, a4 - 1], size_log[l4, a4])) // 2
    lv = np.where(level[l4, a4] > 0, level[l4, a4], level[l4, a4 - 1])
    for kk in np.unique(k):
        wd = (4, 8, 16)[kk] if cap == 2 else (4, 6)[kk]
        in_k = np.nonzero((k == kk) & (lv > 0))[0]
        serial = np.arange(len(in_k))                     # running number over units of this width
        for hh in np.unique(half[in_k]):
            hh_eff = min(int(hh), 8)
            for L in np.unique(lv[in_k]):
                sel = (half[in_k] == hh) & (lv[in_k] == L)
                tab = _lf_profiles(wd, hh_eff, int(L), sharp, bpc)
                u = in_k[sel]
                for i in range(4):
                    r = (serial[sel] * 4 + i) % len(tab)
                    lines = l4[u] * 4 + i
                    ok = lines < view.shape[0]
                    cols = a4[u][ok, None] * 4 - hh_eff + np.arange(2 * hh_eff)[None, :]
                    view[lines[ok, None], cols] = tab[r[ok]]


@functools.lru_cache(maxsize=None)
def lf_directed(bpc, layout, seed):
    """-> (planes, lf meta, w, h, sb128) for the deblock filter."""
    w, h, direction, sharp = LF_SEEDS[seed]
    ss_hor, ss_ver = subsampling(layout)
    dims = plane_dims(w, h, layout)
    til = [_lf_tiling(w, h, direction, _LF_SHAPES_LUMA, 64, seed)]
    if layout:
        shapes = _LF_SHAPES_CHROMA
        t = _lf_tiling(dims[1][0], dims[1][1], direction, shapes, 32, seed)
        til += [t, t]
    rng = np.random.default_rng(1000 * seed + 10 * bpc + layout)
    lf = make_lf_meta(til, w, h, layout, rng, sharpness=sharp)
    bdmax = (1 << bpc) - 1
    planes = []
    level = lf["level"]
    for p, (pw, ph) in enumerate(dims):
        nux, nuy = (pw + 3) >> 2, (ph + 3) >> 2
        lw, lh, sx, sy, bid = _unit_maps(til[p], nux, nuy)
        # levels per block from the list, in place of make_lf_meta's draw
        pick = np.array(LF_LEVELS, np.uint8)
        nb = len(til[p])
        lv = pick[(np.arange(nb)[:, None] * 5 + np.arange(2)[None, :] * 7 + seed + 3 * p) % len(pick)]
        if p == 0:
            level[:nuy, :nux, 0] = lv[bid, 0] if direction == 0 else 0
            level[:nuy, :nux, 1] = lv[bid, 1]
        else:
            level[:nuy, :nux, 1 + p] = lv[bid, 0]
        yy, xx = np.mgrid[0:ph, 0:pw]
        img = (bdmax // 2 + ((xx // 5 + yy // 3) % 9 - 4) * (1 << (bpc - 8))).astype(np.int64)
        if direction == 0:
            _lf_paint(img, sx, lw, level[:nuy, :nux, 0 if p == 0 else 1 + p], 2 if p == 0 else 1, sharp, bpc)
        else:
            _lf_paint(img.T, sy.T, lh.T, level[:nuy, :nux, 1 if p == 0 else 1 + p].T, 2 if p == 0 else 1,
                      sharp, bpc)
        planes.append(img.astype(px_dtype(bpc)))
    lf["tilings"] = til
    return planes, lf, w, h, int(w == 256)


def lf_call_runs(bpc, layout, seed, plane, direction):
    """The loop_filter_sb calls that cover one plane of a directed deblock frame in one
    direction: (x, y, vmask[3], level row, level column, slot) per run of up to 32 4-pixel units
    along one edge line. vmask bit k carries the filter width of unit k as the table entry
    expects it: index 0/1/2 for 4/8/16 on luma, 0/1 for 4/6 on chroma."""
    planes, lf, w, h, _ = lf_directed(bpc, layout, seed)
    ph, pw = planes[plane].shape
    nux, nuy = (pw + 3) >> 2, (ph + 3) >> 2
    lw, lh, sx, sy, _ = _unit_maps(lf["tilings"][plane], nux, nuy)
    cap = 1 if plane else 2
    slot = (0 if direction == 0 else 1) if plane == 0 else 1 + plane
    if direction == 1:
        lw, sx = lh.T, sy.T
    size = np.minimum(lw, cap)
    runs = []
    for a in range(1, sx.shape[1]):                       # the edge line: column (row) of units
        for l0 in range(0, sx.shape[0], 32):
            vm = [0, 0, 0]
            for k in range(min(32, sx.shape[0] - l0)):
                if sx[l0 + k, a]:
                    vm[min(size[l0 + k, a - 1], size[l0 + k, a])] |= 1 << k
            if any(vm):
                x, y, lr, lc = (a * 4, l0 * 4, l0, a) if direction == 0 else (l0 * 4, a * 4, a, l0)
                runs.append((x, y, vm, lr, lc, slot))
    return runs


# =======================================================================================
# CDEF
# =======================================================================================
# (w, h, damping). 134 and 150 are no multiples of 8 and give odd chroma heights at 4:2:0.
CDEF_SEEDS = ((200, 134, 3), (256, 192, 6), (184, 150, 3), (248, 190, 6), (256, 134, 4), (200, 192, 5))
# strength = primary << 2 | secondary; secondary 3 is coded for 4
_CDEF_STRENGTHS = (15 << 2 | 3, 1 << 2 | 0, 15 << 2 | 1, 7 << 2 | 2, 0 << 2 | 3, 7 << 2 | 3, 0, 4 << 2 | 2,
                   15 << 2 | 0, 1 << 2 | 3, 9 << 2 | 2, 15 << 2 | 2)

_YX = np.mgrid[0:8, 0:8]


def _dir_index(d):
    """The line index cdef_find_dir sums along for direction d (its 0..14 / 0..10 / 0..7 bins)."""
    y, x = _YX
    return (y + x, y + (x >> 1), y, 3 + y - (x >> 1), 7 + y - x, 3 - (y >> 1) + x, x, (y >> 1) + x)[d]


def _cdef_block(kind, n, bpc, rng):
    """One 8x8 block. n is the block's running number; rng is only used for pattern values."""
    bdmax = (1 << bpc) - 1
    sc = 1 << (bpc - 8)
    if kind in (0, 1):
        # a pattern constant along direction d plus its image under transposition (kind 0) or
        # under mirroring (kind 1): the two directions tie exactly, with non-zero variance
        d = ((2, 1, 3), (0, 1, 5))[kind][n % 3]
        g = rng.integers(0, bdmax // 2 + 1, size=15)
        a = g[_dir_index(d)]
        return a + (a.T if kind == 0 else a[:, ::-1])
    if kind == 2:
        # 0 / bdmax stripes and checkerboards of period 1, 2 and 4
        y, x = _YX
        per = (1, 2, 4)[n % 3]
        t = ((x // per), (y // per), (x // per + y // per))[(n // 3) % 3]
        return ((t + n // 9) % 2) * bdmax
    if kind == 3:
        return np.full((8, 8), bdmax * (n % 2))
    base, sg = ((0, 1), (bdmax, -1), (bdmax // 2, 1))[n % 3]
    if kind == 4:
        # flat with bumps no larger than the strengths on a lattice of period 3, which no tap
        # offset bridges: every tap of a bump sits on the flat, the filter overshoots it and
        # the clamp has to act. Three blocks in four are split into a half at 0 and a half at
        # bdmax, so that its variance keeps the luma primary strength up.
        y, x = _YX
        amp = np.array((1, 2, 3, 4, 2, 3, 2))[rng.integers(0, 7, size=(8, 8))] * sc
        bumps = amp * ((x % 3 == n % 3) & (y % 3 == n // 3 % 3))
        if n // 3 % 4 == 0:
            return base + sg * bumps
        hi = (x >= 4, y >= 4, x + y >= 8)[n % 3]
        return np.where(hi, bdmax - bumps, bumps)
    # a low-amplitude pattern along one direction: every tap within the thresholds
    g = rng.integers(0, 17, size=15) * sc
    return base + sg * g[_dir_index(n % 8)]


@functools.lru_cache(maxsize=None)
def cdef_directed(bpc, layout, seed):
    """-> (planes, Av1Filter masks, cdef params, w, h) for CDEF."""
    w, h, damping = CDEF_SEEDS[seed]
    rng = np.random.default_rng(7000 + 100 * seed + 10 * bpc + layout)
    planes = []
    for p, (pw, ph) in enumerate(plane_dims(w, h, layout)):
        nby, nbx = (ph + 7) // 8, (pw + 7) // 8
        img = np.zeros((nby * 8, nbx * 8), np.int64)
        for by in range(nby):
            for bx in range(nbx):
                n = by * nbx + bx + seed + p
                kind = (0, 1, 4, 2, 4, 4, 5, 3, 4, 1, 4, 0, 4)[(bx + 3 * by + seed + p) % 13]
                img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = _cdef_block(kind, n, bpc, rng)
        planes.append(np.clip(img[:ph, :pw], 0, (1 << bpc) - 1).astype(px_dtype(bpc)))
    sbh, sbw = (h + 127) >> 7, (w + 127) >> 7
    masks = np.zeros((sbh, sbw), AV1FILTER_DTYPE)
    k = np.arange(4)
    idx = ((np.arange(sbh)[:, None, None] * 5 + np.arange(sbw)[None, :, None] * 3 + k[None, None, :] + seed) % 8)
    idx = idx.astype(np.int8)
    # unset indices: one 64x64 in the frame's first row or column, one inside
    idx[0, (seed // 2) % sbw, seed % 2] = -1
    idx[sbh - 1, sbw - 1, 0 if seed % 2 else 3] = -1
    masks["cdef_idx"] = idx
    # two mask bits per 8x8 block; a fifth of the blocks skipped, the rest with 01, 10 or 11
    by, bx = np.mgrid[0:sbh * 16, 0:sbw * 16]
    sel = (by * 7 + bx * 3 + (by * bx) % 5 + seed) % 11
    bits = np.where(sel < 2, 0, sel % 3 + 1).astype(np.uint32)
    rows = (bits << (2 * (bx % 16))).reshape(sbh, 16, sbw, 16).sum(-1)          # [sbh, 16, sbw]
    rows = rows.transpose(0, 2, 1)
    masks["noskip_mask"] = np.stack([rows & 0xFFFF, rows >> 16], -1).astype(np.uint16)
    st = np.array(_CDEF_STRENGTHS, np.uint8)
    cd = dict(damping=damping, y_strength=st[(np.arange(8) + seed) % len(st)],
              uv_strength=st[(np.arange(8) * 5 + seed + 1) % len(st)])
    return planes, masks, cd, w, h


# =======================================================================================
# Loop restoration
# =======================================================================================
LR_SEEDS = ((384, 256), (330, 200), (256, 200), (384, 232), (320, 256), (296, 248))
_WIENER_LO, _WIENER_HI = (-5, -23, -17), (10, 8, 46)      # the corners of the codable tap ranges
_WIENER_MIX = (-5, 8, -17)
_WIENER_UNITS = ((_WIENER_LO, _WIENER_LO), (_WIENER_HI, _WIENER_HI), (_WIENER_LO, _WIENER_HI),
                 (_WIENER_HI, _WIENER_LO), (_WIENER_MIX, _WIENER_LO), (_WIENER_LO, _WIENER_MIX))
_SGR_W0 = (-96, 31, -96, 31)                               # both ends of each coded weight
_SGR_W1 = (-32, 95, 95, -32)


def _lr_content(pw, ph, bpc, seed, plane):
    """Patches of 48x40 pixels, so that every kind straddles unit, stripe and tile borders."""
    bdmax = (1 << bpc) - 1
    y, x = np.mgrid[0:ph, 0:pw]
    cell = (x // 48) * 5 + (y // 40) * 3 + seed + plane
    kind = cell % 12
    dots = ((x % 4 == 0) & (y % 4 == 0))
    pats = [
        (x % 4 == 0) * bdmax,                  # lines one pixel wide, three apart: the centre tap alone
        (x % 4 != 0) * bdmax,                  # and the opposite: every tap but the centre
        (y % 4 == 0) * bdmax,
        (y % 4 != 0) * bdmax,
        dots * bdmax,
        (~dots) * bdmax,
        ((x + y) % 2) * bdmax,                 # checkerboard
        ((x // 2 + y // 2) % 2) * bdmax,
        np.full_like(x, bdmax),                # flat at the ends of the range
        np.zeros_like(x),
        (x + 2 * y) // 3 % (bdmax + 1),        # shallow ramps
        bdmax - (2 * x + y) // 5 % (bdmax + 1),
    ]
    return np.choose(kind, pats).astype(px_dtype(bpc))


@functools.lru_cache(maxsize=None)
def lr_directed(bpc, layout, seed):
    """-> (CDEF picture C, deblocked picture D, lr meta, w, h) for loop restoration."""
    w, h = LR_SEEDS[seed]
    bdmax = (1 << bpc) - 1
    dims = plane_dims(w, h, layout)
    c = [_lr_content(pw, ph, bpc, seed, p) for p, (pw, ph) in enumerate(dims)]
    # D is C turned upside down in value and shifted: a row taken from the wrong picture shows
    d = [np.roll(bdmax - a, 3, axis=1) for a in c]
    sbh, sbw = (h + 127) >> 7, (w + 127) >> 7
    m = np.zeros((sbh, sbw), AV1RESTORATION_DTYPE)
    u = m["lr"]                                            # [sbh, sbw, 3, 4]
    n_types = len(_WIENER_UNITS) + 16
    for sy in range(sbh):
        for sx in range(sbw):
            for p in range(3):
                for k in range(4):
                    # 4:2:2 chroma units of 64 pixels span 128 luma pixels: only even ones are read
                    step = 2 if p and layout == 2 else 1
                    n = ((sy * 2 + k // 2) * (2 * sbw // step) + (sx * 2 + k % 2) // step) * 7 + seed * 5 + p * 3
                    t = n % n_types
                    un = u[sy, sx, p, k]
                    if t < len(_WIENER_UNITS):
                        fh, fv = _WIENER_UNITS[t]
                        un["type"] = RESTORATION_WIENER
                        un["filter_h"] = fh if p == 0 else (0,) + fh[1:]     # chroma is 5-tap
                        un["filter_v"] = fv if p == 0 else (0,) + fv[1:]
                    else:
                        i = t - len(_WIENER_UNITS)
                        s0, s1 = SGR_PARAMS[i]
                        un["type"] = RESTORATION_SGRPROJ + i
                        j = (n // n_types) % 4
                        un["sgr_weights"] = (0 if s0 == 0 else _SGR_W0[j], 95 if s1 == 0 else _SGR_W1[j])
                    u[sy, sx, p, k] = un
    m["lr"] = u
    lr = dict(lr_mask=m, unit_size_log2=(6, 5 if layout == 1 else 6), restore_planes=7 if layout else 1,
              sb128=0)
    return c, d, lr, w, h


def lr_call_units(bpc, layout, seed, plane):
    """One lr.wiener / lr.sgr call per restoration unit and stripe of one plane of a directed
    frame: (x, y, w, h, edges, unit record). Stripes start 8 luma rows above the multiples of
    64, units are 64 pixels wide (32 on 4:2:0 chroma) and the last one takes the remainder."""
    c, d, lr, w, h = lr_directed(bpc, layout, seed)
    ss_hor, ss_ver = subsampling(layout) if plane else (0, 0)
    ph, pw = c[plane].shape
    unit = 1 << lr["unit_size_log2"][1 if plane else 0]
    units = []
    y = 0
    while y < ph:
        sh = min((64 - (8 if y == 0 else 0)) >> ss_ver, ph - y)
        x = 0
        while x < pw:
            uw = unit if pw - x >= unit + unit // 2 else pw - x
            ly, lx = min((y << ss_ver) + 8, h - 1), x << ss_hor
            rec = lr["lr_mask"]["lr"][ly >> 7, lx >> 7, plane, ((ly >> 6) & 1) * 2 + ((lx >> 6) & 1)]
            edges = (1 if x else 0) | (2 if x + uw < pw else 0) | (4 if y else 0) | (8 if y + sh < ph else 0)
            units.append((x, y, uw, sh, edges, rec))
            x += uw
        y += sh
    return units
