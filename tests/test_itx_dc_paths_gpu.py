"""GPU parity: every device route of a DC-only residual block (DCT_DCT, eob < 1) at its edges.

The routes each carry their own copy of the scaling arithmetic: the transform path's dk[]
(mi_itx_frame, the per-call table), the DC-run path with direct adds (mi_itx_frame_runs), the
DC-run path deferred into the deblocking tiles (MI_ITX_DC_DEFER -> mi_deblock_frame_dc: a 16-bit
map entry and a packed 16-bit add), and the fused intra reconstruction (mi_intra_recon). The
directed frames (tests/dc_ref.py dc_frame: one transform size each, DC runs of exactly NB + 1,
NB - 1, NB and 1 blocks for the DC path's NB blocks per workgroup, runs on chroma, transform
blocks behind a run) carry the directed DC list: values around zero, the extremes of the legal
range, and at 10/12 bit values past it that an int32 arena can hold. Expected pictures are the
oracle's, which tests/test_dc_ref.py pins to the plain integer reference."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import ITX_DC_DEFER, ITX_KEEP_COEFS, lib
from rav1d_amd.frame import Frame, LoopFilterMeta, _stream_ptr
from rav1d_amd.synth import AV1FILTER_DTYPE, TX_DIMS, calc_eih, itx_device_order
from tests import dc_ref, oracle_lib
from tests.oracle_lib import ptr

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("tx,bpc,layout", dc_ref.FRAME_CASES,
                                ids=["%dx%d-%dbit-l%d" % (*TX_DIMS[t], b, lay) for t, b, lay in dc_ref.FRAME_CASES])


def _u32(a):
    return (ctypes.c_uint32 * a.size)(*[int(v) for v in a.reshape(-1)])


def _frame(fr):
    f = Frame(fr["w"], fr["h"], fr["bpc"], fr["layout"])
    for p, a in enumerate(fr["planes"]):
        f.set_plane_np(p, a)
    return f


def _check(f, want, what):
    for p in range(len(want)):
        got = f.plane_np(p)
        if not np.array_equal(got, want[p]):
            bad = np.argwhere(got != want[p])
            y, x = bad[0]
            raise AssertionError(f"{what}: plane {p}: {len(bad)} pixels differ, first at x={x} y={y}: "
                                 f"got {got[y, x]}, expected {want[p][y, x]}")


def _status(gpu):
    assert lib().mi_ctx_device_status(gpu.h, _stream_ptr(None)) == 0, "a descriptor was rejected"


def _runs(gpu, fr, f, coef, flags):
    blocks = torch.from_numpy(fr["band_blocks"].view(np.uint8).copy()).cuda()
    pic = f.picture()
    rc = lib().mi_itx_frame_runs(gpu.h, ctypes.byref(pic), ctypes.c_void_p(blocks.data_ptr()), _u32(fr["band_start"]),
                                 _u32(fr["dc_end"]), ctypes.c_void_p(coef.data_ptr()), flags, _stream_ptr(None))
    torch.cuda.synchronize()
    return rc


def _assert_runs(fr):
    tx = fr["tx"]
    runs = fr["dc_end"].astype(np.int64) - fr["band_start"][:, :-1]
    assert [int(runs[tx, q]) for q in fr["bands"]] == dc_ref.run_lengths(tx) and runs.sum() == sum(dc_ref.run_lengths(tx))


@CASES
def test_dc_blocks_on_the_transform_path(gpu, tx, bpc, layout):
    """mi_itx_frame in plain device order: the DC-only blocks go through itx_size's dk[]"""
    fr = dc_ref.dc_frame(tx, bpc, layout)
    blk, ss = itx_device_order(fr["blocks"])
    f = _frame(fr)
    blocks = torch.from_numpy(blk.view(np.uint8).copy()).cuda()
    coef = torch.from_numpy(fr["coef"].copy()).cuda()
    pic = f.picture()
    assert lib().mi_itx_frame(gpu.h, ctypes.byref(pic), ctypes.c_void_p(blocks.data_ptr()), _u32(ss),
                              ctypes.c_void_p(coef.data_ptr()), 0, _stream_ptr(None)) == 0
    _status(gpu)
    _check(f, fr["ref"], "mi_itx_frame")
    assert not coef.cpu().numpy().any(), "the arena is zeroed"


@CASES
def test_dc_runs_added_directly(gpu, tx, bpc, layout):
    """mi_itx_frame_runs: the runs on itx_dc (whole and partial workgroups), the rest on itx_size"""
    fr = dc_ref.dc_frame(tx, bpc, layout)
    _assert_runs(fr)
    f = _frame(fr)
    coef = torch.from_numpy(fr["coef"].copy()).cuda()
    assert _runs(gpu, fr, f, coef, 0) == 0
    _status(gpu)
    _check(f, fr["ref"], "mi_itx_frame_runs")
    assert not coef.cpu().numpy().any(), "the arena is zeroed"
    f = _frame(fr)
    coef = torch.from_numpy(fr["coef"].copy()).cuda()
    assert _runs(gpu, fr, f, coef, ITX_KEEP_COEFS) == 0
    _status(gpu)
    _check(f, fr["ref"], "mi_itx_frame_runs(KEEP_COEFS)")
    assert np.array_equal(coef.cpu().numpy(), fr["coef"]), "MI_ITX_KEEP_COEFS leaves the arena untouched"


def _lf_off(fr):
    """deblocking off (filter_y 0) for the frame's geometry: mi_deblock_frame_dc then copies the
    reconstruction and adds the deferred DC"""
    sbw, sbh = (fr["w"] + 127) >> 7, (fr["h"] + 127) >> 7
    e, i = calc_eih(0)
    return LoopFilterMeta(dict(level=np.zeros((sbh * 32, sbw * 32, 4), np.uint8), masks=np.zeros((sbh, sbw), AV1FILTER_DTYPE),
                               lim_e=e, lim_i=i, b4_stride=sbw * 32, sb128w=sbw, filter_y=0, filter_uv=0))


@CASES
def test_dc_runs_deferred_into_deblock(gpu, tx, bpc, layout):
    """mi_itx_frame_runs(MI_ITX_DC_DEFER) + mi_deblock_frame_dc: the destination has every
    residual; the reconstruction has the source plus the non-DC residuals and no DC (the
    documented contract: it lacks the DC runs). Values past the legal range must give the pixel
    of int arithmetic, as on the undeferred routes.

    Before the deferred DC was clamped to +-bdmax (itx.hip itx_dc) this failed at 10 and 12 bit
    for every size but the six 2:1 ones with a side of 16 or more (whose wrapped values happen
    to keep their sign): e.g. 4x4, the block at x=8 y=0 with DC coefficient 2^23 - 1, scaled
    262088, which wrapped in the map's 16-bit field to -56: pixel 0 gave 0, not bdmax."""
    fr = dc_ref.dc_frame(tx, bpc, layout)
    _assert_runs(fr)
    f = _frame(fr)
    d = Frame(fr["w"], fr["h"], bpc, layout)
    coef = torch.from_numpy(fr["coef"].copy()).cuda()
    lf = _lf_off(fr)
    assert _runs(gpu, fr, f, coef, ITX_KEEP_COEFS | ITX_DC_DEFER) == 0
    ps, pd = f.picture(), d.picture()
    assert lib().mi_deblock_frame_dc(gpu.h, ctypes.byref(ps), ctypes.byref(pd), ctypes.byref(lf.s), _stream_ptr(None)) == 0
    _status(gpu)
    _check(d, fr["ref"], "deferred DC, destination")
    _check(f, fr["recon"], "deferred DC, reconstruction (source + non-DC residuals, no DC)")


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_per_call_table_directed_dc(gpu, bpc):
    """mi_dsp_itxfm_add (DCT_DCT, eob 0) over the directed DC list at every size, on rows of 0,
    rows of bdmax and random pixels; the oracle's itxfm_add and the plain reference agree"""
    L = lib()
    o = oracle_lib.load_oracle()
    rng = np.random.default_rng(300 + bpc)
    bdmax = (1 << bpc) - 1
    cdt = np.int16 if bpc == 8 else np.int32
    dt = np.uint8 if bpc == 8 else np.uint16
    for tx, (w, h) in enumerate(TX_DIMS):
        base = rng.integers(0, 1 << bpc, size=(h, w + 16)).astype(dt)
        base[0], base[1] = 0, bdmax
        for dc in dc_ref.directed_dcs(bpc):
            c = np.zeros(min(w, 32) * min(h, 32), cdt)
            c[0] = dc
            c_ref, d, d_ref = c.copy(), base.copy(), base.copy()
            o.oracle_itxfm_add(tx, 0, ptr(d_ref), d_ref.strides[0], ptr(c_ref), 0, bdmax)
            assert np.array_equal(d_ref[:, :w], dc_ref.dc_add(base[:, :w], tx, dc, bpc))
            assert L.mi_dsp_itxfm_add(tx, 0, ptr(d), d.strides[0], ptr(c), 0, bdmax) == 0
            assert np.array_equal(d, d_ref), (tx, dc)
            assert not c.any()


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_intra_fused_directed_dc(gpu, bpc):
    """mi_intra_recon (ipred.hip itx_rows' DC branch): an intra frame whose DC-only transform
    blocks carry the directed DC list, against the oracle's decode-order reconstruction"""
    from rav1d_amd.intra import IntraFrame, device_status, make_intra_residuals
    from rav1d_amd.ipred_synth import make_intra_frame
    w, h, layout = 256, 192, 1
    rng = np.random.default_rng(700 + bpc)
    fr = make_intra_residuals(make_intra_frame(w, h, bpc, layout, rng), bpc, rng)
    tb = fr["tx_blocks"]
    dc = np.nonzero((tb["txtp"] == 0) & (tb["eob"] == 0))[0]
    assert len(set(int(t) for t in tb["tx"][dc])) >= 4, "DC-only blocks of at least four sizes"
    dcs = dc_ref.directed_dcs(bpc, edges_first=True)
    assert len(dc) >= len(dcs)
    fr["coef"][tb["coef_off"][dc]] = np.array([dcs[k % len(dcs)] for k in range(len(dc))], fr["coef"].dtype)
    cur = Frame(w, h, bpc, layout)
    for p in range(3):
        cur.set_buffer_np(p, rng.integers(0, 1 << bpc, size=cur.buffer_np(p).shape))
    init = [cur.buffer_np(p) for p in range(3)]
    IntraFrame(gpu, fr).recon(cur.picture())
    device_status(gpu)
    exp, _ = oracle_lib.intra_recon(init, bpc, fr["blocks"], tb[fr["tx_of_block"]], fr["ac"], fr["idx"], fr["pal"], fr["coef"])
    for p in range(3):
        got = cur.buffer_np(p)
        if not np.array_equal(got, exp[p]):
            bad = np.argwhere(got != exp[p])
            raise AssertionError(f"plane {p}: {len(bad)} mismatches, first at {bad[0]}")
