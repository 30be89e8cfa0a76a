"""CPU checks of the loop-restoration oracle (oracle/lr.c)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from rav1d_amd.synth import make_lr_meta, make_mixed_texture
from tests import oracle_lib
from tests.oracle_lib import load_oracle
from tests.test_oracle_lf import pad_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_table_digest(name):
    """Length and SHA-256 of the reference's dav1d_<name> (src/tables.c), recorded in
    tests/golden/ref_tables.json by tools/gen_tables.py --digests."""
    return json.load(open(os.path.join(ROOT, "tests", "golden", "ref_tables.json")))[name]


def table_digest(vals):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_tables
    return gen_tables.digest(vals)


def test_sgr_x_by_x_formula_matches_reference_table():
    o = load_oracle()
    o.oracle_sgr_x_by_x.restype = ctypes.POINTER(ctypes.c_uint8)
    ours = o.oracle_sgr_x_by_x()
    assert table_digest([ours[i] for i in range(256)]) == ref_table_digest("sgr_x_by_x")


def planes_for(w, h, bpc, layout, rng):
    ss_h = 1 if layout in (1, 2) else 0
    ss_v = 1 if layout == 1 else 0
    ps = [make_mixed_texture(rng, w, h, bpc)]
    if layout:
        ps += [make_mixed_texture(rng, (w + ss_h) >> ss_h, (h + ss_v) >> ss_v, bpc) for _ in range(2)]
    return ps


def identity_meta(lr):
    u = lr["lr_mask"]["lr"]
    u["filter_h"] = 0
    u["filter_v"] = 0
    # coded SGR weights cannot reach w0 = w1 = 0 (w1 = 128 - w0 - w1raw >= 2), so SGR units
    # become NONE here; Wiener with all taps 0 (centre 128) is an exact identity
    u["type"] = np.where(u["type"] >= 3, 0, u["type"])
    lr["lr_mask"]["lr"] = u
    return lr


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_identity_parameters_leave_frame_unchanged(bpc):
    """Zero Wiener taps (centre tap 128 in both passes) are an exact identity."""
    w, h, layout = 200, 150, 1
    rng = np.random.default_rng(bpc)
    c = pad_planes(planes_for(w, h, bpc, layout, rng), w, h, bpc, layout)
    d = pad_planes(planes_for(w, h, bpc, layout, rng), w, h, bpc, layout)
    lr = identity_meta(make_lr_meta(w, h, layout, rng, sb128=0, unit_log2=(6, 5)))
    out = oracle_lib.lr_frame(c, d, bpc, layout, w, h, lr)
    for p in range(3):
        assert np.array_equal(out[p], c[p])


def test_restoration_changes_pixels_and_stays_in_range():
    w, h, layout, bpc = 256, 200, 1, 10
    rng = np.random.default_rng(5)
    c = pad_planes(planes_for(w, h, bpc, layout, rng), w, h, bpc, layout)
    d = pad_planes(planes_for(w, h, bpc, layout, rng), w, h, bpc, layout)
    lr = make_lr_meta(w, h, layout, rng, sb128=1)
    out = oracle_lib.lr_frame(c, d, bpc, layout, w, h, lr)
    assert not np.array_equal(out[0], c[0])
    assert max(int(o.max()) for o in out) <= 1023


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_per_call_identity_filters_leave_unit_unchanged(bpc):
    """lr.wiener with the identity taps (centre 128, as lr_apply builds it: without the +128 at
    8 bits) and lr.sgr with zero weights return the unit unchanged for every edge combination,
    whatever the left / lpf neighbours hold."""
    import ctypes
    from rav1d_amd.synth import make_texture
    o = oracle_lib.load_oracle()
    VP, I, SS = ctypes.c_void_p, ctypes.c_int, ctypes.c_ssize_t
    o.oracle_lr_wiener.argtypes = [VP, SS, VP, VP, I, I, VP, I, I]
    o.oracle_lr_wiener.restype = None
    o.oracle_lr_sgr.argtypes = [I, VP, SS, VP, VP, I, I, ctypes.c_uint, ctypes.c_uint, I, I, I, I]
    o.oracle_lr_sgr.restype = None
    rng = np.random.default_rng(40 + bpc)
    bdmax = (1 << bpc) - 1
    f = np.zeros((2, 8), np.int16)
    f[0, 3] = 0 if bpc == 8 else 128
    f[1, 3] = 128
    for edges in range(16):
        pic = make_texture(rng, 120, 40, bpc)
        left = make_texture(rng, 4, 24, bpc)
        lpf = make_texture(rng, 120, 8, bpc)
        off = 8 * 120 + 8
        p = ctypes.c_void_p(pic.ctypes.data + off * pic.itemsize)
        lp = ctypes.c_void_p(lpf.ctypes.data + 8 * lpf.itemsize)
        before = pic.copy()
        o.oracle_lr_wiener(p, pic.strides[0], oracle_lib.ptr(left), lp, 97, 24, oracle_lib.ptr(f), edges, bdmax)
        assert np.array_equal(pic, before), ("wiener", edges)
        for kind, (s0, s1) in ((0, (140, 0)), (1, (0, 3236)), (2, (140, 3236))):
            o.oracle_lr_sgr(kind, p, pic.strides[0], oracle_lib.ptr(left), lp, 97, 24, s0, s1, 0, 0, edges, bdmax)
            assert np.array_equal(pic, before), ("sgr", kind, edges)
