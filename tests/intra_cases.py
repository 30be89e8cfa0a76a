"""Directed intra frames: pictures of any size, cut into several tiles, optionally with extreme
pixels, as MiIntraBlock records (the dict ipred_synth.make_intra_frame returns, so
make_intra_residuals, IntraFrame, run_intra_frame and the oracle helpers take them unchanged).

What make_intra_frame cannot produce and this does:
  * a picture whose size is no multiple of the block sizes. The coded area is the luma size
    rounded up to 8, shifted per plane (the reference's 4 * bw >> ss). Transform blocks starting
    at or beyond it are dropped, blocks straddling it are kept whole (they write into the
    picture's padding), max_w / max_h are the distance to its end;
  * tiles. Blocks come tile by tile in raster tile order; HAVE_LEFT / HAVE_TOP are relative to
    the block's tile, tile_w / tile_h are the tile's end in plane pixels (the coded area's end
    for the last tile), TOP_RIGHT / BOTTOM_LEFT need the pixels written and inside the tile,
    and dependencies, intra block copy sources and CfL luma stay inside the tile. One exception,
    as a decoder makes it: its edge flags are relative to the superblock and know no tiles, so a
    block in the top row of a superblock below its tile's first carries TOP_RIGHT even where it
    ends at its tile's end, and x + w >= tile_w is what cuts that top-right. Such blocks carry
    the flag here too; nothing depends on the pixels beyond the tile, which are not yet written;
  * blocks that lack an edge, straddle the coded area's end or end at their tile's end take in
    turn the modes whose edge preparation that changes (DC, PAETH, V, H, SMOOTH, Z1, Z3), so
    that every fallback of rav1d_prepare_intra_edges is present whatever the seed;
  * extreme: palettes of {0, bdmax} on about 0.3 of the blocks (they write exact extremes
    whatever their edges, and so seed extreme neighbours for the blocks after them), stored CfL
    AC over the full +-(bdmax << 3), alpha from {-16, -1, 1, 16}.

census() counts the directed kinds of block in such a frame; CASES are the frames the GPU tests
run, and tests/test_intra_cases.py asserts the census for each of them without a GPU."""
import functools

import numpy as np

from rav1d_amd import (INTRA_BOTTOM_LEFT, INTRA_CFL_AC, INTRA_DTYPE, INTRA_EDGE_FILTER, INTRA_HAVE_LEFT,
                       INTRA_HAVE_TOP, INTRA_SMOOTH_NB, INTRA_TOP_RIGHT)
from rav1d_amd.ipred_synth import BASE_ANGLES
from rav1d_amd.synth import partition_blocks

MODE_DC, MODE_V, MODE_H, MODE_D45, MODE_D203, MODE_D67, MODE_PAETH = 0, 1, 2, 3, 7, 8, 12
MODE_SMOOTH, MODE_FILTER, MODE_CFL, MODE_PAL, MODE_IBC = 9, 13, 32, 64, 96
# edges each final mode reads: LEFT 1, TOP 2, TOP_LEFT 4, TOP_RIGHT 8, BOTTOM_LEFT 16
NEEDS = (3, 2, 1, 1, 2, 0, 14, 7, 21, 3, 3, 3, 7, 7)


def _align(v, a):
    return (v + a - 1) // a * a


def _subsampling(layout):
    return (1 if layout in (1, 2) else 0), (1 if layout == 1 else 0)


def _z1(rng):
    """A mode and angle delta below 90 degrees (Z1 when the top row is there, else V)."""
    m = (MODE_D45, MODE_D67, MODE_V)[int(rng.integers(0, 3))]
    return m, int(rng.integers(-3, 0)) if m == MODE_V else int(rng.integers(-3, 4))


def _z3(rng):
    """A mode and angle delta above 180 degrees (Z3 when the left column is there, else H)."""
    m = (MODE_D203, MODE_H)[int(rng.integers(0, 2))]
    return m, int(rng.integers(1, 4)) if m == MODE_H else int(rng.integers(-3, 4))


# the modes that blocks of one situation take in turn (None: the ordinary random draw)
_TURNS = {
    "no_left": ("z3", MODE_DC, MODE_PAETH, None, None),
    "no_top": ("z1", MODE_DC, MODE_PAETH, None, None),
    "neither": (MODE_DC, MODE_PAETH, None),
    "straddle_right": (MODE_V, "z1", MODE_SMOOTH, None),
    "straddle_bottom": (MODE_H, "z3", MODE_SMOOTH, None),
    "straddle_both": (MODE_SMOOTH, MODE_PAETH, None),
    "cut_top_right": ("z1_36",),
    "right_end": ("z1", None),
    "bottom_end": ("z3", None),
    "both_ends": ("z1", "z3", None),
}


def make_directed_intra_frame(w, h, bpc, layout, rng, sb=64, tile_cols=(0,), tile_rows=(0,), extreme=False,
                              min_bs=8, p_split=0.7, tx_split=0.5, cfl_frac=0.4, filter_frac=0.1,
                              edge_filter=None, cfl_dev_frac=0.5, ibc_frac=0.05):
    """A w x h intra frame in tiles starting at the luma columns tile_cols and rows tile_rows
    (multiples of sb). Returns make_intra_frame's dict."""
    ss_h, ss_v = _subsampling(layout)
    nplanes = 3 if layout else 1
    bdmax = (1 << bpc) - 1
    cw0, ch0 = _align(w, 8), _align(h, 8)                       # coded area, luma
    assert tile_cols[0] == 0 and tile_rows[0] == 0
    assert all(c % sb == 0 and c < cw0 for c in tile_cols) and all(r % sb == 0 and r < ch0 for r in tile_rows)
    cols, rows = list(tile_cols) + [cw0], list(tile_rows) + [ch0]
    aw, ah = _align(w, 128), _align(h, 128)                     # the picture allocation (frame.plane_geometry)
    owner = [np.full((ah >> (ss_v if p else 0), aw >> (ss_h if p else 0)), -1, np.int64) for p in range(nplanes)]
    pal_frac = 0.3 if extreme else 0.05
    if extreme:
        cfl_frac = 0.3
    if edge_filter is None:
        edge_filter = int(rng.integers(0, 2))
    dt = np.uint8 if bpc == 8 else np.uint16
    level_of, dep_lists, recs, ac, idx, pal = [], [], [], [], [], []
    n_ac = n_idx = n_pal = 0
    turn = {}

    for tr in range(len(rows) - 1):
        for tc in range(len(cols) - 1):
            X0, X1, Y0, Y1 = cols[tc], cols[tc + 1], rows[tr], rows[tr + 1]
            for (bx, by, bw, bh) in partition_blocks(X1 - X0, Y1 - Y0, rng, sb=sb, min_bs=min_bs, p_split=p_split):
                bx, by = bx + X0, by + Y0
                for pl in range(nplanes):
                    sh, sv = (ss_h, ss_v) if pl else (0, 0)
                    cw, ch = cw0 >> sh, ch0 >> sv               # coded area, this plane
                    x0, x1, y0, y1 = X0 >> sh, X1 >> sh, Y0 >> sv, Y1 >> sv   # the tile, this plane
                    own = owner[pl]
                    px, py, pbw, pbh = bx >> sh, by >> sv, bw >> sh, bh >> sv
                    tw = pbw // 2 if pbw >= 8 and rng.random() < tx_split else pbw
                    th = pbh // 2 if pbh >= 8 and rng.random() < tx_split else pbh
                    tw, th = min(tw, 64), min(th, 64)
                    if tw * 4 < th:
                        th = tw * 4
                    if th * 4 < tw:
                        tw = th * 4
                    for ty in range(py, py + pbh, th):
                        for tx in range(px, px + pbw, tw):
                            if tx >= cw or ty >= ch:
                                continue
                            hl, ht = tx > x0, ty > y0
                            flags = (INTRA_HAVE_LEFT if hl else 0) | (INTRA_HAVE_TOP if ht else 0)
                            flags |= INTRA_EDGE_FILTER if edge_filter else 0
                            flags |= INTRA_SMOOTH_NB if rng.random() < 0.3 else 0
                            if ht and tx + tw < x1 and (own[ty - 1, tx + tw:min(tx + 2 * tw, x1)] >= 0).all() \
                                    and rng.random() < 0.85:
                                flags |= INTRA_TOP_RIGHT
                            if hl and ty + th < y1 and (own[ty + th:min(ty + 2 * th, y1), tx - 1] >= 0).all() \
                                    and rng.random() < 0.85:
                                flags |= INTRA_BOTTOM_LEFT
                            # (a decoder's superblock-relative flag at an interior tile end)
                            if ht and tx + tw == x1 and x1 < cw and ty % (sb >> sv) == 0 and rng.random() < 0.85:
                                flags |= INTRA_TOP_RIGHT
                            # a flagged top-right that the tile's end cuts or shortens: rare, always Z1
                            cut_tr = bool(flags & INTRA_TOP_RIGHT) and x1 - tx - tw < tw
                            # the block's situation, and whether it is its turn to take a directed mode
                            over_r, over_b = ht and tx + tw > x1, hl and ty + th > y1
                            right_end = ht and (tx + tw == x1 or ((flags & INTRA_TOP_RIGHT) and x1 - tx - tw < tw))
                            bottom_end = hl and (ty + th == y1 or ((flags & INTRA_BOTTOM_LEFT) and y1 - ty - th < th))
                            # (a block in several situations takes the one served least so far)
                            sits = []
                            if cut_tr:
                                sits = ["cut_top_right"]
                            elif not hl or not ht:
                                sits = ["neither" if not hl and not ht else "no_left" if not hl else "no_top"]
                            else:
                                if over_r or over_b:
                                    sits.append("straddle_both" if over_r and over_b else
                                                "straddle_right" if over_r else "straddle_bottom")
                                if right_end or bottom_end:
                                    sits.append("both_ends" if right_end and bottom_end else
                                                "right_end" if right_end else "bottom_end")
                            sit = min(sits, key=lambda s_: turn.get((pl > 0, s_), 0)) if sits else None
                            directed = None
                            if sit is not None:
                                key = (pl > 0, sit)
                                directed = _TURNS[sit][turn.get(key, 0) % len(_TURNS[sit])]
                                turn[key] = turn.get(key, 0) + 1
                            r = rng.random()
                            is_pal = directed is None and r < pal_frac
                            is_cfl = directed is None and pl > 0 and pal_frac <= r < pal_frac + cfl_frac
                            # CfL with the AC from the reconstructed luma. The luma under a chroma
                            # block that straddles the coded area was never decoded there: those
                            # 4-pixel groups are padding (w_pad / h_pad), as in the reference
                            cfl_dev = bool(is_cfl and tw <= 32 and th <= 32 and rng.random() < cfl_dev_frac)
                            reserved = 0
                            deps = []
                            # intra block copy from pixels of this tile that are already written
                            # (half-pel in subsampled chroma for odd displacements; the tap past a
                            # source that ends at the coded area's end replicates it, as emu_edge)
                            ibc = None
                            if directed is None and not cfl_dev and rng.random() < ibc_frac:
                                for t_ in range(8):
                                    lx, lyd = -int(rng.integers(0, 65)), -int(rng.integers(0, 65))
                                    if t_ & 1:
                                        lx, lyd = (-int(rng.integers(0, 2)), lyd) if t_ & 2 else \
                                            (lx, -int(rng.integers(0, 2)))
                                    mvx, mvy = 8 * lx, 8 * lyd
                                    sx, sy = tx + (mvx >> (3 + sh)), ty + (mvy >> (3 + sv))
                                    mxp = (mvx & (15 >> (1 - sh))) << (1 - sh)
                                    myp = (mvy & (15 >> (1 - sv))) << (1 - sv)
                                    ex, ey = min(sx + tw + (mxp > 0), cw), min(sy + th + (myp > 0), ch)
                                    if sx >= x0 and sy >= y0 and sx + tw <= x1 and sy + th <= y1 and ex <= x1 and \
                                            ey <= y1 and (own[sy:ey, sx:ex] >= 0).all():
                                        ibc = (mvx, mvy)
                                        deps.append(own[sy:ey, sx:ex].ravel())
                                        break
                            if cfl_dev:
                                wp = int(rng.integers(0, tw // 4)) if rng.random() < 0.3 else 0
                                hp = int(rng.integers(0, th // 4)) if rng.random() < 0.3 else 0
                                wp, hp = max(wp, (tx + tw - cw + 3) // 4, 0), max(hp, (ty + th - ch + 3) // 4, 0)
                                reserved = wp | (hp << 8) | (ss_h << 16) | (ss_v << 17)
                                flags |= INTRA_CFL_AC
                                ly0, lx0 = ty << ss_v, tx << ss_h
                                luma = owner[0][ly0:ly0 + ((th - 4 * hp) << ss_v), lx0:lx0 + ((tw - 4 * wp) << ss_h)]
                                assert (luma >= 0).all()
                                deps.append(luma.ravel())
                            # every pixel of the tile that the edge may read
                            if hl:
                                deps.append(own[ty:min(ty + 2 * th, y1), tx - 1])
                            if ht:
                                deps.append(own[ty - 1, max(tx - 1, x0):min(tx + 2 * tw, x1)])
                            dep_ids = np.unique(np.concatenate(deps)) if deps else np.zeros(0, np.int64)
                            dep_ids = dep_ids[dep_ids >= 0]
                            lv = 1 + max(level_of[i] for i in dep_ids) if dep_ids.size else 0
                            dep_lists.append(dep_ids)
                            mode, angle, filt, alpha, aux, poff = 0, 0, 0, 0, 0, 0
                            if directed == "z1_36":
                                # 36 degrees: the flattest Z1, whose last rows read the far end of the top-right
                                mode, angle = MODE_D45, -3
                            elif directed == "z1":
                                mode, angle = _z1(rng)
                            elif directed == "z3":
                                mode, angle = _z3(rng)
                            elif directed is not None:
                                mode = directed
                            elif ibc is not None:
                                mode, filt = MODE_IBC, sh | (sv << 1)
                                reserved = (ibc[0] & 0xFFFF) | ((ibc[1] & 0xFFFF) << 16)
                            elif is_pal:
                                mode = MODE_PAL
                                if extreme:
                                    pal.append((rng.integers(0, 2, size=8) * bdmax).astype(dt))
                                else:
                                    pal.append(rng.integers(0, 1 << bpc, size=8).astype(dt))
                                poff, n_pal = n_pal, n_pal + 8
                                idx.append(rng.integers(0, 8, size=tw * th).astype(np.uint8))
                                aux, n_idx = n_idx, n_idx + tw * th
                            elif is_cfl:
                                mode = MODE_CFL
                                alpha = int(rng.choice([-16, -1, 1, 16])) if extreme else int(rng.integers(-16, 17))
                                lim = bdmax << 3 if extreme else 400
                                ac.append(rng.integers(-lim, lim + 1, size=tw * th).astype(np.int16))
                                aux, n_ac = n_ac, n_ac + tw * th
                            elif tw <= 32 and th <= 32 and r < pal_frac + cfl_frac + filter_frac:
                                mode, filt = MODE_FILTER, int(rng.integers(0, 5))
                            else:
                                mode = int(rng.integers(0, 13))
                                if 1 <= mode <= 8:
                                    angle = int(rng.integers(-3, 4))
                            # intra block copy: max_w / max_h = the reference area mc() clamps to
                            mw, mh = (cw, ch) if mode == MODE_IBC else (cw - tx, ch - ty)
                            k = len(recs)
                            recs.append((tx, ty, tw, th, pl, mode, angle, flags, filt, alpha, x1, y1, mw, mh,
                                         aux, poff, reserved))
                            level_of.append(lv)
                            own[ty:ty + th, tx:tx + tw] = k
    blocks = np.array(recs, dtype=INTRA_DTYPE)
    lv = np.array(level_of, np.int64)
    order = np.argsort(lv, kind="stable")
    level_start = np.searchsorted(lv[order], np.arange(lv.max() + 2)).astype(np.int64)
    cat = lambda xs, d: np.concatenate(xs) if xs else np.zeros(1, d)  # noqa: E731
    return dict(blocks=blocks, order=order, level_start=level_start, ac=cat(ac, np.int16), idx=cat(idx, np.uint8),
                pal=cat(pal, dt), deps=dep_lists)


def final_mode(b):
    """The implementation mode rav1d_prepare_intra_edges turns a block's mode into (6 / 7 / 8:
    Z1 / Z2 / Z3; 3 / 4 / 5: LEFT_DC / TOP_DC / DC_128), and the final angle."""
    m = int(b["mode"])
    hl, ht = bool(b["flags"] & INTRA_HAVE_LEFT), bool(b["flags"] & INTRA_HAVE_TOP)
    if m == MODE_CFL:
        m = MODE_DC
    if 1 <= m <= 8:
        angle = BASE_ANGLES[m - 1] + 3 * int(b["angle"])
        if angle <= 90:
            return (6 if angle < 90 and ht else 1), angle
        if angle < 180:
            return 7, angle
        return (8 if angle > 180 and hl else 2), angle
    if m == MODE_DC:
        return (0 if ht else 3) if hl else (4 if ht else 5), 0
    if m == MODE_PAETH:
        return (12 if ht else 2) if hl else (1 if ht else 5), 0
    return m, 0


# kinds of block the census counts; the first five need a second tile
INTERIOR_KINDS = ("no_left_at_tile_col", "no_top_at_tile_row", "neither_at_tile_corner", "top_right_cut_by_tile_end",
                  "bottom_left_cut_by_tile_end")
EDGE_KINDS = ("straddles_right_end", "straddles_bottom_end", "z1_to_v", "z3_to_h", "dc_to_left_dc", "dc_to_top_dc",
              "dc_to_dc_128", "paeth_fallback")
SHORT_KIND = "top_right_run_shorter_than_w"
FLAGGED_KIND = "flagged_top_right_cut_by_tile_end"
CFL_KIND = "cfl_device_ac_padded"


def census(fr, layout, tile_cols=(0,), tile_rows=(0,)):
    """{(is_chroma, kind): count} over the blocks of a directed frame."""
    ss_h, ss_v = _subsampling(layout)
    out = {}

    def hit(c, kind):
        out[(c, kind)] = out.get((c, kind), 0) + 1

    for b in fr["blocks"]:
        c = bool(b["plane"])
        sh, sv = (ss_h, ss_v) if c else (0, 0)
        x, y, w, h = int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"])
        tile_w, tile_h, mode, flags = int(b["tile_w"]), int(b["tile_h"]), int(b["mode"]), int(b["flags"])
        x0 = max(t >> sh for t in tile_cols if (t >> sh) <= x)
        y0 = max(t >> sv for t in tile_rows if (t >> sv) <= y)
        last_col, last_row = x0 == tile_cols[-1] >> sh, y0 == tile_rows[-1] >> sv
        hl, ht = bool(flags & INTRA_HAVE_LEFT), bool(flags & INTRA_HAVE_TOP)
        assert hl == (x > x0) and ht == (y > y0)
        if mode == MODE_CFL and (flags & INTRA_CFL_AC) and (int(b["reserved"]) & 0xFFFF):
            hit(c, CFL_KIND)
        if mode in (MODE_PAL, MODE_IBC):
            continue                                     # no edge preparation
        if not hl and ht and x0 > 0:
            hit(c, "no_left_at_tile_col")
        if hl and not ht and y0 > 0:
            hit(c, "no_top_at_tile_row")
        if not hl and not ht and (x0 > 0 or y0 > 0):
            hit(c, "neither_at_tile_corner")
        if mode == MODE_FILTER:
            continue
        fm, angle = final_mode(b)
        # (blocks that read the row / column they straddle the end of)
        if tile_w - x < w and ht and (NEEDS[fm] & 2):
            hit(c, "straddles_right_end")
        if tile_h - y < h and hl and (NEEDS[fm] & 1):
            hit(c, "straddles_bottom_end")
        if mode != MODE_CFL:
            if fm == 6 and x + w == tile_w and not last_col:
                hit(c, "top_right_cut_by_tile_end")
                if (flags & INTRA_TOP_RIGHT) and angle == 36:
                    hit(c, FLAGGED_KIND)
            if fm == 8 and y + h == tile_h and not last_row:
                hit(c, "bottom_left_cut_by_tile_end")
            if fm == 6 and angle == 36 and (flags & INTRA_TOP_RIGHT) and 0 < tile_w - x - w < w:
                hit(c, SHORT_KIND)
            if 1 <= mode <= 8 and angle < 90 and not ht:
                hit(c, "z1_to_v")
            if 1 <= mode <= 8 and angle > 180 and not hl:
                hit(c, "z3_to_h")
            if mode == MODE_DC and fm != 0:
                hit(c, ("dc_to_left_dc", "dc_to_top_dc", "dc_to_dc_128")[fm - 3])
            if mode == MODE_PAETH and fm != 12:
                hit(c, "paeth_fallback")
    return out


# The frames of the GPU tests (tests/test_intra_frame_gpu.py): name -> (w, h, superblock, tile
# column starts, tile row starts, whether a top-right run shorter than the block can occur,
# whether a tile holds a second superblock row whose blocks carry TOP_RIGHT at the tile's end).
# In "B" it cannot: the last tile column is one 8-pixel block wide and every other tile ends
# on a multiple of 128, so a block that ends before its tile's end has a whole block of room.
# In "C" it cannot either: the short run lies beyond x = 64, in the next superblock of the only
# superblock row, which is decoded later, so those pixels are never written in time.
FRAMES = {
    "A": (200, 134, 64, (0, 64, 128), (0, 64), True, True),
    "B": (264, 200, 128, (0, 128, 256), (0, 128), False, False),
    "C": (72, 40, 64, (0,), (0,), False, False),
}

# (frame, bpc, layout, extreme, seed): every layout and every bit depth with both tiled frames,
# one extreme variant per bit depth. The seeds are the first for which the census holds.
CASES = [
    ("A", 8, 1, False, 1), ("A", 10, 0, False, 2), ("A", 12, 2, False, 0), ("A", 8, 3, False, 0),
    ("A", 12, 1, True, 0),
    ("B", 8, 1, False, 0), ("B", 10, 2, False, 0), ("B", 12, 3, False, 1), ("B", 8, 0, False, 0),
    ("B", 10, 3, True, 0),
    ("C", 10, 1, False, 0), ("C", 12, 0, False, 2), ("C", 8, 2, True, 7),
]


def case_id(case):
    name, bpc, layout, extreme, _ = case
    return f"{name}-{bpc}bpc-layout{layout}" + ("-extreme" if extreme else "")


def required_kinds(name, layout):
    """[(is_chroma, kind)] that the census of a case must hold."""
    w, h, sb, tcols, trows, short, flagged = FRAMES[name]
    kinds = list(EDGE_KINDS) + ([SHORT_KIND] if short else []) + ([FLAGGED_KIND] if flagged else [])
    if len(tcols) > 1 or len(trows) > 1:
        kinds += list(INTERIOR_KINDS)
    req = [(c, k) for c in ((False, True) if layout else (False,)) for k in kinds]
    return req + ([(True, CFL_KIND)] if layout else [])


@functools.lru_cache(maxsize=None)
def case_frame(case):
    """The case's frame with its residuals (make_intra_residuals)."""
    from rav1d_amd.intra import make_intra_residuals
    name, bpc, layout, extreme, seed = case
    w, h, sb, tcols, trows = FRAMES[name][:5]
    rng = np.random.default_rng([seed, bpc, layout, int(extreme), w, h])
    fr = make_directed_intra_frame(w, h, bpc, layout, rng, sb=sb, tile_cols=tcols, tile_rows=trows, extreme=extreme)
    return make_intra_residuals(fr, bpc, rng)


def without_tiles(blocks, w, h, layout):
    """The same blocks as one tile: left / top present wherever the picture has them, the tile's
    end at the coded area's end. (Tiles come in raster order, so those pixels are written.)"""
    ss_h, ss_v = _subsampling(layout)
    b = blocks.copy()
    c = b["plane"] > 0
    b["flags"] &= ~np.uint8(INTRA_HAVE_LEFT | INTRA_HAVE_TOP)
    b["flags"] |= np.where(b["x"] > 0, INTRA_HAVE_LEFT, 0).astype(np.uint8)
    b["flags"] |= np.where(b["y"] > 0, INTRA_HAVE_TOP, 0).astype(np.uint8)
    b["tile_w"] = np.where(c, _align(w, 8) >> ss_h, _align(w, 8))
    b["tile_h"] = np.where(c, _align(h, 8) >> ss_v, _align(h, 8))
    return b


def case_init(case, shapes):
    """The randomised picture buffers a case starts from: whole allocated planes."""
    _, bpc, layout, extreme, seed = case
    rng = np.random.default_rng([seed, bpc, layout, 77])
    return [rng.integers(0, 1 << bpc, size=s).astype(np.uint8 if bpc == 8 else np.uint16) for s in shapes]
