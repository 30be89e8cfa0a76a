"""A plain reference for DC-only residual blocks (DCT_DCT, eob < 1), from the specification of
the path (rav1d src/itx.rs:64-188 dc_only; C src/itx_tmpl.c:40-100), in Python integers:

  1. dc = (dc * 181 + 128) >> 8          when one side is twice the other (rect2 scaling)
  2. dc = (dc * 181 + 128) >> 8
  3. dc = (dc + rnd) >> shift            the size's row shift, rnd = (1 << shift) >> 1
  4. dc = (dc * 181 + 128 + 2048) >> 12
  5. pixel = clip(pixel + dc, 0, bitdepth_max)

Python's >> on a negative int is the arithmetic shift the C code relies on. The directed DC list
is what the DC tests feed every device path with: the values around zero where the roundings
differ, the extremes of the legal range, seeded draws over it, and for the int32 arenas of
10/12-bit frames values outside it (up to 2^23 in magnitude: beyond, dc * 181 leaves 32-bit
int in the reference and the kernels alike and no behaviour is defined)."""
import numpy as np

from rav1d_amd.synth import TX_DIMS

# the inverse transform's row shift per RectTxfmSize (src/itx.rs:439-457), TX_DIMS order
TX_SHIFT = [0, 1, 2, 2, 2, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2]
assert len(TX_SHIFT) == len(TX_DIMS)

N_DRAWS = 40


def dc_value(tx, dc):
    """The constant a DC-only block of size `tx` with DC coefficient `dc` adds to its pixels."""
    w, h = TX_DIMS[tx]
    dc = int(dc)
    if w == 2 * h or h == 2 * w:
        dc = (dc * 181 + 128) >> 8
    dc = (dc * 181 + 128) >> 8
    shift = TX_SHIFT[tx]
    dc = (dc + ((1 << shift) >> 1)) >> shift
    return (dc * 181 + 128 + 2048) >> 12


def dc_add(px, tx, dc, bpc):
    """`px` (any integer array) after a DC-only block of size tx: int64 pixels."""
    return np.clip(np.asarray(px).astype(np.int64) + dc_value(tx, dc), 0, (1 << bpc) - 1)


def legal_range(bpc):
    """(lo, hi) of a dequantised coefficient (rav1d src/recon.rs decode_coefs clamp)."""
    cf_max = (128 << bpc) - 1
    return -cf_max - 1, cf_max


def out_of_range_dcs(bpc):
    """Values an int32 arena can hold past the legal range; none at 8 bits (the int16 arena
    holds exactly the legal range)."""
    return [] if bpc == 8 else [1 << 20, -(1 << 20), (1 << 23) - 1, -(1 << 23)]


def directed_dcs(bpc, edges_first=False):
    """The directed DC list of a bit depth. edges_first: the same values with the out-of-range
    and extreme ones leading, for frames whose few DC blocks cycle through only its head."""
    lo, hi = legal_range(bpc)
    small = [0, 1, -1, 2, -2, 3, -3, 5, -5]
    extreme = [hi, lo, hi // 2, -(hi // 2)]
    rng = np.random.default_rng(0xDC00 + bpc)
    draws = [int(v) for v in rng.integers(lo, hi + 1, size=N_DRAWS)]
    oor = out_of_range_dcs(bpc)
    return oor + extreme + small + draws if edges_first else small + extreme + draws + oor


# ---- directed frames for the device DC paths ------------------------------------------------

ITX_DC_ITEMS = 16     # rav1d_amd/csrc/common.h kItxDcItems
FRAME_W, FRAME_H = 512, 256   # 128-aligned: padding plays no part


def itx_dc_blocks(tx):
    """Blocks one DC-path workgroup takes (rav1d_amd/csrc/common.h itx_dc_blocks)."""
    w, h = TX_DIMS[tx]
    return max(1, min(128, 64 * ITX_DC_ITEMS // (h * (1 if w < 8 else w // 8))))


def run_lengths(tx):
    """The DC-run lengths a directed frame holds, in band order: a full workgroup plus a one-block
    one, one block short of a workgroup, exactly one workgroup, a single block."""
    nb = itx_dc_blocks(tx)
    return [nb + 1, nb - 1, nb, 1]


def plane_dims(layout):
    ss_h, ss_v = int(layout in (1, 2)), int(layout == 1)
    c = (FRAME_W >> ss_h, FRAME_H >> ss_v)
    return [(FRAME_W, FRAME_H)] + ([c, c] if layout else [])


def directed_planes(rng, bpc, layout):
    """Destination pixels: texture with rows of 0 and rows of bdmax (period 12, so the rows fall
    differently into the blocks of every height)."""
    from rav1d_amd.synth import make_texture
    bdmax = (1 << bpc) - 1
    planes = []
    for pw, ph in plane_dims(layout):
        pl = make_texture(rng, pw, ph, bpc)
        y = np.arange(ph) % 12
        pl[y < 2] = 0
        pl[(y >= 2) & (y < 4)] = bdmax
        planes.append(pl)
    return planes


_frames = {}

# (tx, bpc, layout) of the directed frames: every size at every bit depth in 4:2:0, and a
# monochrome and a 4:4:4 variant of a small, a wide, a 32-point and a 64-point size
FRAME_CASES = [(tx, bpc, 1) for tx in range(len(TX_DIMS)) for bpc in (8, 10, 12)] + \
              [(tx, bpc, layout) for layout in (0, 3) for tx in (0, 8, 3, 18) for bpc in (8, 10, 12)]


def dc_frame(tx, bpc, layout=1):
    """One 512x256 frame of non-overlapping blocks of size `tx` whose DC runs (per band of
    rav1d_amd.synth.itx_band_order, DC-only blocks of every plane leading the band) have exactly
    run_lengths(tx) in four different bands; the first and third of them hold transform blocks
    after the run, and (when the frame has more than four bands of the size) one band holds
    transform blocks only. With chroma planes whose band holds a block of the size, a third of a
    run each lies on U and V. DCs cycle through directed_dcs(bpc, edges_first=True).

    Returns a dict that callers must not modify: blocks (decode order), coef, planes, dc (bool per
    block), band_blocks / band_start / dc_end (itx_band_order, itx_dc_runs), bands (the four run
    bands), ref (the oracle's pictures after every block), recon (after the non-DC blocks only)."""
    key = (tx, bpc, layout)
    if key in _frames:
        return _frames[key]
    from rav1d_amd import TXBLOCK_DTYPE
    from rav1d_amd.synth import itx_band_order, itx_dc_runs, make_coefs, tx_types
    from tests import oracle_lib
    rng = np.random.default_rng(0xD0C0 + tx * 16 + bpc + 1000 * layout)
    w, h = TX_DIMS[tx]
    dims = plane_dims(layout)

    def positions(p, q):
        pw, ph = dims[p]
        return [(x, y) for y in range(0, ph - h + 1, h) if y * 8 // ph == q for x in range(0, pw - w + 1, w)]

    occupied = [q for q in range(8) if positions(0, q)]
    bands = occupied[:4]
    assert len(bands) == 4
    chroma = layout != 0 and all(positions(1, q) for q in bands)
    dcs = directed_dcs(bpc, edges_first=True)
    recs, chunks, off, ndc = [], [], 0, 0

    def add_dc(p, x, y):
        nonlocal off, ndc
        recs.append((off, x, y, p, tx, 0, 0, 0))
        chunks.append(np.array([dcs[ndc % len(dcs)]], np.int64))   # the DC alone, as the front-end stores it
        off += 1
        ndc += 1

    def add_tx(p, x, y, regime):
        nonlocal off
        types = tx_types(tx)
        txtp = types[int(rng.integers(len(types)))]
        c, eob = make_coefs(rng, tx, txtp, regime, bpc)
        recs.append((off, x, y, p, tx, txtp, 0, max(eob, 1)))
        chunks.append(c)
        off += c.size

    for i, (q, n) in enumerate(zip(bands, run_lengths(tx))):
        per = [n, 0, 0]
        if chroma and n >= 3:
            nc = min(n // 3, len(positions(1, q)))
            per = [n - 2 * nc, nc, nc]
        for p in range(len(dims)):
            pos = positions(p, q)
            assert per[p] <= len(pos), "the run must fit inside one band"
            for (x, y) in pos[:per[p]]:
                add_dc(p, x, y)
            if i in (0, 2):   # both routes in one call: transform blocks after the band's run
                for k, (x, y) in enumerate(pos[per[p]:per[p] + (3 if p == 0 else 1)]):
                    add_tx(p, x, y, 1 + k % 2)
    for q in occupied[4:5]:   # a band without a run
        for k, (x, y) in enumerate(positions(0, q)[:2]):
            add_tx(0, x, y, 2 - k)
    blocks = np.array(recs, dtype=TXBLOCK_DTYPE)
    coef = np.concatenate(chunks).astype(np.int16 if bpc == 8 else np.int32)
    dc = (blocks["txtp"] == 0) & (blocks["eob"] < 1)
    assert np.array_equal(coef[blocks["coef_off"][dc]].astype(np.int64),
                          np.array([dcs[k % len(dcs)] for k in range(ndc)]))   # no value truncated by the arena
    planes = directed_planes(rng, bpc, layout)

    band_blocks, _, bs = itx_band_order(blocks, [ph for _, ph in dims] + [FRAME_H] * (3 - len(dims)))
    de = itx_dc_runs(band_blocks, bs)
    runs = (de.astype(np.int64) - bs[:, :-1])
    want = np.zeros_like(runs)
    want[tx, bands] = run_lengths(tx)
    assert np.array_equal(runs, want), "the frame's DC runs are not the lengths it was built for"
    assert (bs[tx, np.array(bands)[[0, 2]] + 1] > de[tx, np.array(bands)[[0, 2]]]).all(), "transform blocks after a run"

    ref = oracle_lib.itx_frame([p.copy() for p in planes], blocks, coef.copy(), bpc)
    recon = oracle_lib.itx_frame([p.copy() for p in planes], blocks[~dc], coef.copy(), bpc)
    # the plain reference and the oracle judge the device together: they must agree
    for b in blocks[dc]:
        p, x, y = int(b["plane"]), int(b["x"]), int(b["y"])
        exp = dc_add(planes[p][y:y + h, x:x + w], tx, int(coef[b["coef_off"]]), bpc)
        assert np.array_equal(ref[p][y:y + h, x:x + w], exp), (tx, bpc, p, x, y)
        assert np.array_equal(recon[p][y:y + h, x:x + w], planes[p][y:y + h, x:x + w])
    fr = dict(w=FRAME_W, h=FRAME_H, bpc=bpc, layout=layout, tx=tx, blocks=blocks, coef=coef, planes=planes, dc=dc,
              band_blocks=band_blocks, band_start=bs, dc_end=de, bands=bands, chroma=chroma, ref=ref, recon=recon)
    _frames[key] = fr
    return fr
