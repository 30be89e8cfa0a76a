"""Directed inverse-transform inputs: coefficients at the limits of their range, for every
transform size and every type the size allows.

Every input is a pure function of (tx, txtp, bpc, pattern name). The coefficients live in the
coded min(w, 32) x min(h, 32) area and span the whole range a conformant stream can hold:
CF_MAX = 128 * 2^bpc - 1 and CF_MIN = -CF_MAX - 1 (the dequantiser's clamp). make_coefs draws
sigma = 4 * 2^bpc with a steep decay, so with it the intermediate clips of the 1-D kernels, the
clip between the two passes and the pixel clip fire by accident or not at all.

PATTERNS (one block of each per (size, type) pair, WHT_WHT on 4x4 included):
  max, min            every coefficient at one end of the range
  altx, alty, altxy   max / min alternating by x, by y, by x + y (asymmetric: a transposed
                      residual shows)
  rsign0..2           random signs at full magnitude
  runi0..2            uniform over the whole range
  match{a}_{b}, matchn{a}_{b}
                      the sign pattern that peaks output (ox, oy), ox = (0, w/2, w-1)[a] and
                      oy = (0, h/2, h-1)[b]: max where sign(B_row[ox, x]) * sign(B_col[oy, y]) > 0,
                      else min (matchn: negated), with the basis signs taken from the oracle's
                      1-D kernels on unit vectors. Drives the intermediate and the final clips
  imp{max,min}{0..3}  one coefficient, at (0, 0), (sw-1, 0), (0, sh-1), (sw-1, sh-1)
  row0, col0          the first row / the first column at max
  i16fit, i16edge     32767 / -32768 alone, and together with 32768 / -32769: the int16 boundary
                      of the packed arena (pack_coefs picks MI_TX_I16 exactly when the corner
                      fits int16). At 8 bits the range ends at the boundary and both are equal

corner_cases(): every packed corner shape (cw, ch) in steps of 4 of every size, filled with
int16 values and non-zero at its far element, once as it is and (10 / 12 bits) once with one
value outside int16, so that both arena forms occur for every shape.

build_frame() lays a list of cases out with a shelf packer over the planes of a picture, so
that one launch runs thousands of them; DC-only DCT_DCT blocks at max / min are mixed in so
that mi_itx_frame_runs has runs. tests/test_itx_cases.py shows without a GPU, on the census
flavour of the oracle, which single-decision slips these inputs notice."""
import functools
import zlib

import numpy as np

from rav1d_amd import TXBLOCK_DTYPE
from rav1d_amd.frame import plane_geometry
from rav1d_amd.synth import TX_DIMS, itx_device_order, pack_coefs, tx_types
from tests import oracle_lib

BPCS = (8, 10, 12)
WHT = 16
K_DCT, K_ADST, K_FLIPADST, K_IDENTITY, K_WHT = range(5)
# TxfmType -> 1-D kind of the column (vertical) and the row (horizontal) pass; oracle/itx.c
COL_KIND = (K_DCT, K_ADST, K_DCT, K_ADST, K_FLIPADST, K_DCT, K_FLIPADST, K_ADST, K_FLIPADST, K_IDENTITY,
            K_DCT, K_IDENTITY, K_ADST, K_IDENTITY, K_FLIPADST, K_IDENTITY, K_WHT)
ROW_KIND = (K_DCT, K_DCT, K_ADST, K_ADST, K_DCT, K_FLIPADST, K_FLIPADST, K_FLIPADST, K_ADST, K_IDENTITY,
            K_IDENTITY, K_DCT, K_IDENTITY, K_ADST, K_IDENTITY, K_FLIPADST, K_WHT)

# the 155 (size, type) pairs of tx_types, then WHT_WHT on 4x4
PAIRS = tuple((tx, t) for tx in range(len(TX_DIMS)) for t in tx_types(tx)) + ((0, WHT),)

BASE_PATTERNS = (("max", "min", "altx", "alty", "altxy") + tuple(f"rsign{k}" for k in range(3)) +
                 tuple(f"runi{k}" for k in range(3)) +
                 tuple(f"match{n}{a}_{b}" for n in ("", "n") for a in range(3) for b in range(3)))
EXTRA_PATTERNS = (tuple(f"imp{s}{k}" for s in ("max", "min") for k in range(4)) +
                  ("row0", "col0", "i16fit", "i16edge"))
PATTERNS = BASE_PATTERNS + EXTRA_PATTERNS
CLASSES = ("flat", "alt", "rsign", "runi", "match", "imp", "line", "i16")


def pattern_class(name):
    if name in ("max", "min"):
        return "flat"
    if name in ("row0", "col0"):
        return "line"
    return next(c for c in CLASSES if name.startswith(c))


# one pattern of every class first, then the others: the order the fused intra frames deal them in
_LEAD = ("max", "altxy", "rsign0", "runi0", "match1_1", "impmax3", "row0", "i16edge")
DEAL_ORDER = _LEAD + tuple(n for n in PATTERNS if n not in _LEAD)
PIXEL_BASES = ("zero", "max", "rand")


def cf_range(bpc):
    """(CF_MIN, CF_MAX): the dequantiser's clamp (rav1d src/recon.rs decode_coefs)."""
    return -(128 << bpc), (128 << bpc) - 1


def coded_dims(tx):
    w, h = TX_DIMS[tx]
    return min(w, 32), min(h, 32)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def basis(kind, n):
    """B[o, i] << 14 of the n-point 1-D kernel: output o's response to input i (i < min(n, 32)),
    from the oracle's kernel on a unit vector large enough for its rounding not to hide a sign."""
    s = np.zeros((n, min(n, 32)), np.int64)
    for i in range(min(n, 32)):
        v = np.zeros(n, np.int32)
        v[i] = 1 << 14
        s[:, i] = oracle_lib.itx_1d(kind, n, v)
    return s


def basis_signs(kind, n):
    return np.sign(basis(kind, n))


def widest_matches(tx, txtp):
    """The two matched patterns of a pair whose output has the largest reach (sum of |basis|
    over the coded inputs): the first as it is, the second negated."""
    w, h = TX_DIMS[tx]
    br, bc = np.abs(basis(ROW_KIND[txtp], w)).sum(1), np.abs(basis(COL_KIND[txtp], h)).sum(1)
    reach = sorted(((-int(br[(0, w // 2, w - 1)[a]] * bc[(0, h // 2, h - 1)[b]]), a, b)
                    for a in range(3) for b in range(3)))
    (_, a0, b0), (_, a1, b1) = reach[:2]
    return f"match{a0}_{b0}", f"matchn{a1}_{b1}"


def pattern(tx, txtp, bpc, name):
    """(coefficients in the dense arena order y + x * sh as int64, eob) of one directed block."""
    w, h = TX_DIMS[tx]
    sw, sh = coded_dims(tx)
    lo, hi = cf_range(bpc)
    xs, ys = np.arange(sw)[:, None], np.arange(sh)[None, :]
    eob = sw * sh - 1
    pick = lambda m: np.where(m, hi, lo).astype(np.int64)   # noqa: E731
    if name == "max":
        c = np.full((sw, sh), hi, np.int64)
    elif name == "min":
        c = np.full((sw, sh), lo, np.int64)
    elif name == "altx":
        c = pick((xs + 0 * ys) % 2 == 0)
    elif name == "alty":
        c = pick((0 * xs + ys) % 2 == 0)
    elif name == "altxy":
        c = pick((xs + ys) % 2 == 0)
    elif name.startswith("rsign"):
        c = pick(_rng(tx, txtp, bpc, name).random((sw, sh)) < 0.5)
    elif name.startswith("runi"):
        c = _rng(tx, txtp, bpc, name).integers(lo, hi + 1, size=(sw, sh))
    elif name.startswith("match"):
        neg = name.startswith("matchn")
        a, b = (int(v) for v in name[6 if neg else 5:].split("_"))
        ox, oy = (0, w // 2, w - 1)[a], (0, h // 2, h - 1)[b]
        sr = basis_signs(ROW_KIND[txtp], w)[ox, :sw]
        sc = basis_signs(COL_KIND[txtp], h)[oy, :sh]
        c = pick((sr[:, None] * sc[None, :] > 0) != neg)
    elif name.startswith("imp"):
        k = int(name[-1])
        x, y = (0, sw - 1)[k & 1], (0, sh - 1)[k >> 1]
        c = np.zeros((sw, sh), np.int64)
        c[x, y] = hi if name.startswith("impmax") else lo
        eob = max(1, y + x * sh)      # never the DC path: these blocks carry their type's transform
    elif name == "row0":
        c = np.zeros((sw, sh), np.int64)
        c[:, 0] = hi
    elif name == "col0":
        c = np.zeros((sw, sh), np.int64)
        c[0, :] = hi
    elif name == "i16fit":
        c = pick((xs + 2 * ys) % 2 == 0).clip(-32768, 32767)
    elif name == "i16edge":
        c = np.array([32767, -32768, 32768, -32769], np.int64)[(xs + 2 * ys) % 4].clip(lo, hi)
    else:
        raise KeyError(name)
    return c.reshape(-1), eob


def pair_cases(bpc, patterns=PATTERNS, pairs=PAIRS):
    """[(tx, txtp, coefficients, eob, name)] of every pattern of every pair."""
    return [(tx, t) + pattern(tx, t, bpc, n) + (n,) for (tx, t) in pairs for n in patterns]


def corner_shapes(tx):
    sw, sh = coded_dims(tx)
    return [(cw, ch) for cw in range(4, sw + 1, 4) for ch in range(4, sh + 1, 4)]


def corner_cases(bpc):
    """[(tx, txtp, coefficients, eob, name)]: every packed corner shape of every size; the types
    of the size in turn. `name` is ("corner", cw, ch, wide)."""
    out = []
    lo, hi = cf_range(bpc)
    for tx in range(len(TX_DIMS)):
        sw, sh = coded_dims(tx)
        types = tx_types(tx)
        for k, (cw, ch) in enumerate(corner_shapes(tx)):
            for wide in ((False, True) if bpc > 8 else (False,)):
                rng = _rng("corner", tx, cw, ch, bpc, wide)
                c = np.zeros((sw, sh), np.int64)
                c[:cw, :ch] = rng.integers(-32768, 32768, size=(cw, ch))
                c[cw - 1, ch - 1] = 32767 if k % 2 else -32768        # the far element: never zero
                if wide:
                    c[cw // 2, ch // 2] = (32768, -32769, hi, lo)[k % 4]
                txtp = types[k % len(types)]
                out.append((tx, txtp, c.reshape(-1), sw * sh - 1, ("corner", cw, ch, wide)))
    return out


def dc_cases(bpc, per_sign=3):
    """DC-only DCT_DCT blocks (eob 0, one stored coefficient) at max and min, every size."""
    lo, hi = cf_range(bpc)
    return [(tx, 0, np.array([v], np.int64), 0, "dc") for tx in range(len(TX_DIMS))
            for v in (hi, lo) for _ in range(per_sign)]


def _subsampling(layout):
    return (1 if layout in (1, 2) else 0), (1 if layout == 1 else 0)


def shelf_pack(cases, layout, width):
    """Places the cases' blocks on the planes of a picture `width` luma pixels wide: blocks
    sorted by height then width (so shelves of one height fill their plane's width exactly while
    blocks of that height last), each shelf on the plane that is least full. Returns
    ([(plane, x, y)] per case, luma height): the smallest picture height that holds them all."""
    ss_hor, ss_ver = _subsampling(layout)
    pws = [width] if layout == 0 else [width, width >> ss_hor, width >> ss_hor]
    vscale = [1] if layout == 0 else [1, 1 << ss_ver, 1 << ss_ver]
    order = sorted(range(len(cases)), key=lambda i: (-TX_DIMS[cases[i][0]][1], -TX_DIMS[cases[i][0]][0], i))
    used = [0] * len(pws)          # rows taken per plane
    pos = [None] * len(cases)
    shelf = None                   # (plane, y, height, x)
    for i in order:
        w, h = TX_DIMS[cases[i][0]]
        if shelf is None or shelf[2] != h or shelf[3] + w > pws[shelf[0]]:
            p = min(range(len(pws)), key=lambda q: (used[q] * vscale[q], q))
            shelf = [p, used[p], h, 0]
            used[p] += h
        pos[i] = (shelf[0], shelf[3], shelf[1])
        shelf[3] += w
    height = max(u * s for u, s in zip(used, vscale))
    return pos, height


def build_frame(cases, bpc, layout, width, base="rand", packed=False):
    """One itx frame of the given cases: dict(blocks (device order), size_start, coef, planes
    (whole allocated buffers, rows x stride in pixels), w, h, bpc, layout, case_of_block (index
    into cases per block of `blocks`))."""
    pos, height = shelf_pack(cases, layout, width)
    recs, chunks, off = [], [], 0
    for (tx, txtp, c, eob, _), (p, x, y) in zip(cases, pos):
        flags = 0
        if packed and not (txtp == 0 and eob < 1):
            c, flags = pack_coefs(c, tx, bpc > 8)
            if flags and off % 4:
                chunks.append(np.zeros(4 - off % 4, np.int64))
                off += 4 - off % 4
        recs.append((off, x, y, p, tx, txtp, flags, eob))
        chunks.append(np.asarray(c, np.int64))
        off += len(c)
    blocks = np.array(recs, dtype=TXBLOCK_DTYPE)
    coef = np.concatenate(chunks)
    cdt = np.int16 if bpc == 8 else np.int32
    assert coef.min() >= np.iinfo(cdt).min and coef.max() <= np.iinfo(cdt).max
    # device order, remembering which case each block is
    tag = np.arange(len(blocks))
    dc = (blocks["txtp"] == 0) & (blocks["eob"] < 1)
    order = np.lexsort((blocks["x"], blocks["y"], blocks["plane"], ~dc, blocks["tx"]))
    sorted_blocks, size_start = itx_device_order(blocks)
    assert np.array_equal(sorted_blocks, blocks[order])
    (yr, ys), (cr, cs), _ = plane_geometry(width, height, layout, bpc)
    pxb = 1 if bpc == 8 else 2
    shapes = [(yr, ys // pxb)] + ([] if layout == 0 else [(cr, cs // pxb)] * 2)
    dt = np.uint8 if bpc == 8 else np.uint16
    bdmax = (1 << bpc) - 1
    if base == "zero":
        planes = [np.zeros(s, dt) for s in shapes]
    elif base == "max":
        planes = [np.full(s, bdmax, dt) for s in shapes]
    elif base == "mid":
        planes = [np.full(s, (bdmax + 1) >> 1, dt) for s in shapes]
    else:
        rng = _rng("pixels", bpc, layout, width, len(cases))
        planes = [rng.integers(0, bdmax + 1, size=s).astype(dt) for s in shapes]
    return dict(blocks=sorted_blocks, size_start=size_start, coef=coef.astype(cdt), planes=planes, w=width,
                h=height, bpc=bpc, layout=layout, case_of_block=tag[order])


# luma width per layout: a multiple of 64 and not of 128, so that shelves fill it exactly and the
# allocated planes (128-aligned) are wider than the picture
FRAME_WIDTH = {0: 1088, 1: 1216, 2: 1088, 3: 704}


@functools.lru_cache(maxsize=None)
def _frame_cases(bpc, kind):
    if kind == "pairs":
        return pair_cases(bpc) + dc_cases(bpc)
    if kind == "corners":
        return corner_cases(bpc) + dc_cases(bpc, 1)
    raise KeyError(kind)


def directed_frame(bpc, base, layout, kind="pairs", packed=False):
    """The directed frame of one bit depth, pixel base and layout: kind "pairs" holds one block
    per (size, type, pattern), "corners" one per packed corner shape and arena form."""
    cases = _frame_cases(bpc, kind)
    fr = build_frame(cases, bpc, layout, FRAME_WIDTH[layout], base, packed)
    fr["cases"] = cases
    return fr


def edge_blocks(fr):
    """(blocks ending at their plane's right edge, at its bottom edge)."""
    ss_hor, ss_ver = _subsampling(fr["layout"])
    b = fr["blocks"]
    dims = np.array(TX_DIMS)
    pw = np.where(b["plane"] == 0, fr["w"], (fr["w"] + ss_hor) >> ss_hor)
    ph = np.where(b["plane"] == 0, fr["h"], (fr["h"] + ss_ver) >> ss_ver)
    return (int((b["x"] + dims[b["tx"], 0] == pw).sum()), int((b["y"] + dims[b["tx"], 1] == ph).sum()))


# ---- fused intra reconstruction: generated intra frames whose residuals are the patterns ----

# (w, h, layout, seed, make_intra_frame settings, initial picture): together these frames hold
# all 19 transform sizes often enough for every (size, type) to get a pattern of every class
INTRA_FRAMES = ((512, 384, 3, 0x17C1, dict(sb=64, min_bs=4, tx_split=0.5), "rand"),
                (512, 384, 3, 0x17C2, dict(sb=64, min_bs=4, tx_split=0.5), "zero"),
                (512, 384, 1, 0x17C3, dict(sb=64, min_bs=8, tx_split=0.5), "max"))


@functools.lru_cache(maxsize=None)
def intra_frames(bpc):
    """[(frame dict of make_intra_residuals, initial picture name, dealt)]: the k-th transform
    block of a size, counted through all frames, takes type k mod (types of the size) and
    pattern DEAL_ORDER[k div types]; 4x4 blocks take WHT_WHT as a 17th type. dealt: the set of
    (tx, txtp, pattern) in the frame."""
    from rav1d_amd.intra import make_intra_residuals
    from rav1d_amd.ipred_synth import make_intra_frame
    count = [0] * len(TX_DIMS)
    out = []
    for (w, h, layout, seed, kw, init) in INTRA_FRAMES:
        rng = np.random.default_rng(seed)
        fr = make_intra_residuals(make_intra_frame(w, h, bpc, layout, rng, **kw), bpc, rng)
        tb, coef = fr["tx_blocks"], fr["coef"]
        dealt = set()
        for k in range(len(tb)):
            tx = int(tb[k]["tx"])
            types = tx_types(tx) + ([WHT] if tx == 0 else [])
            txtp = types[count[tx] % len(types)]
            name = DEAL_ORDER[count[tx] // len(types) % len(DEAL_ORDER)]
            count[tx] += 1
            c, eob = pattern(tx, txtp, bpc, name)
            off = int(tb[k]["coef_off"])
            coef[off:off + len(c)] = c
            tb[k]["txtp"], tb[k]["eob"] = txtp, eob
            dealt.add((tx, txtp, name))
        out.append((fr, init, dealt))
    return out


def intra_init(fr_w, fr_h, layout, bpc, init):
    """The picture a fused intra frame starts from: whole allocated planes."""
    (yr, ys), (cr, cs), _ = plane_geometry(fr_w, fr_h, layout, bpc)
    pxb = 1 if bpc == 8 else 2
    shapes = [(yr, ys // pxb)] + ([] if layout == 0 else [(cr, cs // pxb)] * 2)
    dt, bdmax = (np.uint8 if bpc == 8 else np.uint16), (1 << bpc) - 1
    if init == "rand":
        rng = _rng("intra init", fr_w, fr_h, layout, bpc)
        return [rng.integers(0, bdmax + 1, size=s).astype(dt) for s in shapes]
    return [np.full(s, 0 if init == "zero" else bdmax, dt) for s in shapes]
