"""GPU parity: DC-only residuals deferred into the deblocking pass.

mi_itx_frame_runs(MI_ITX_DC_DEFER) records each DC-only block's constant in the context's DC
map instead of adding it; mi_deblock_frame_dc adds it to the pixels it stages. The deblocked
picture must equal the one of the plain order (itx adds every residual, then deblock), which the
oracle's itx_frame + deblock_frame produce (rav1d src/itx.rs:64-188 dc_only path, then
src/lf_apply.rs:597-834)."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import ITX_DC_DEFER, ITX_KEEP_COEFS, lib
from rav1d_amd.frame import Frame, LoopFilterMeta, _stream_ptr
from rav1d_amd.synth import itx_band_order, itx_dc_runs, make_frame
from tests import oracle_lib
from tests.pipeline import pad_planes

pytestmark = pytest.mark.gpu


def _inputs(w, h, bpc, layout, seed):
    fr = make_frame(w, h, bpc, layout, seed=seed, with_fg=False)
    ah = (h + 127) & ~127
    ssv = 1 if layout == 1 else 0
    blk, _, bs = itx_band_order(fr["blocks"], [ah, ah >> ssv, ah >> ssv])
    de = itx_dc_runs(blk, bs)
    return fr, blk, bs, de


def _run(gpu, fr, blk, bs, de, defer, filter_y=None, dst_same=False):
    w, h, bpc, layout = fr["w"], fr["h"], fr["bpc"], fr["layout"]
    A = Frame(w, h, bpc, layout)
    for p, a in enumerate(fr["planes"]):
        A.set_plane_np(p, a)
    D = A if dst_same else Frame(w, h, bpc, layout)
    blocks = torch.from_numpy(blk.view(np.uint8).copy()).cuda()
    coef = torch.from_numpy(fr["coef"].copy()).cuda()
    lf = LoopFilterMeta(fr["lf"])
    if filter_y is not None:
        lf.s.filter_y = filter_y
    pa, pd = A.picture(), D.picture()
    bsa = (ctypes.c_uint32 * bs.size)(*[int(v) for v in bs.reshape(-1)])
    dea = (ctypes.c_uint32 * de.size)(*[int(v) for v in de.reshape(-1)])
    sp = _stream_ptr(None)
    L = lib()
    rc = L.mi_itx_frame_runs(gpu.h, ctypes.byref(pa), ctypes.c_void_p(blocks.data_ptr()), bsa, dea,
                             ctypes.c_void_p(coef.data_ptr()), ITX_KEEP_COEFS | (ITX_DC_DEFER if defer else 0), sp)
    assert rc == 0
    rc = L.mi_deblock_frame_dc(gpu.h, ctypes.byref(pa), ctypes.byref(pd), ctypes.byref(lf.s), sp)
    torch.cuda.synchronize()
    return rc, A, D


def _oracle(fr, deblock=True):
    """the plain order on the CPU, as tests/pipeline.py's oracle_pipeline: itx, then deblock"""
    w, h, bpc, layout = fr["w"], fr["h"], fr["bpc"], fr["layout"]
    A = oracle_lib.itx_frame(pad_planes(fr["planes"], w, h, bpc, layout), fr["blocks"], fr["coef"].copy(), bpc)
    return oracle_lib.deblock_frame(A, bpc, layout, w, h, fr["lf"], sb128=1) if deblock else A


@pytest.mark.parametrize("geom", [(256, 192, 8, 1), (640, 360, 10, 1), (352, 288, 12, 3), (720, 486, 10, 2),
                                  (200, 136, 10, 0), (1920, 1080, 10, 1)])
def test_deferred_dc_matches_oracle(gpu, geom):
    w, h, bpc, layout = geom
    fr, blk, bs, de = _inputs(w, h, bpc, layout, seed=w * 3 + bpc)
    assert (de > bs[:, :-1]).any(), "the frame must hold DC runs"
    rc, A, D = _run(gpu, fr, blk, bs, de, defer=True)
    assert rc == 0
    ref = _oracle(fr)
    for p in range(3 if layout else 1):
        got = D.plane_np(p)
        ph, pw = got.shape
        assert np.array_equal(got, ref[p][:ph, :pw]), f"plane {p}"


def test_deferred_dc_equals_plain_order_at_4k10(gpu):
    fr, blk, bs, de = _inputs(3840, 2160, 10, 1, seed=0x4C100001)
    rc, _, d_defer = _run(gpu, fr, blk, bs, de, defer=True)
    assert rc == 0
    rc, _, d_plain = _run(gpu, fr, blk, bs, de, defer=False)
    assert rc == 0
    for p in range(3):
        assert np.array_equal(d_defer.plane_np(p), d_plain.plane_np(p)), p


def test_deferred_dc_with_deblocking_off(gpu):
    # filter_y 0: the output is the reconstruction with the DC added, nothing filtered
    fr, blk, bs, de = _inputs(640, 360, 10, 1, seed=5)
    rc, _, D = _run(gpu, fr, blk, bs, de, defer=True, filter_y=0)
    assert rc == 0
    ref = _oracle(fr, deblock=False)
    for p in range(3):
        got = D.plane_np(p)
        ph, pw = got.shape
        assert np.array_equal(got, ref[p][:ph, :pw]), p


def test_deferred_dc_rejects_in_place_and_other_geometry(gpu):
    fr, blk, bs, de = _inputs(256, 192, 10, 1, seed=6)
    rc, _, _ = _run(gpu, fr, blk, bs, de, defer=True, dst_same=True)
    assert rc == -22
    # a pending deferral is consumed by the next deblock call; a picture of another size is refused
    rc, A, _ = _run(gpu, fr, blk, bs, de, defer=False)
    assert rc == 0
    other = Frame(320, 192, 10, 1)
    blocks = torch.from_numpy(blk.view(np.uint8).copy()).cuda()
    coef = torch.from_numpy(fr["coef"].copy()).cuda()
    pa = A.picture()
    L = lib()
    assert L.mi_itx_frame_runs(gpu.h, ctypes.byref(pa), ctypes.c_void_p(blocks.data_ptr()),
                               (ctypes.c_uint32 * bs.size)(*[int(v) for v in bs.reshape(-1)]),
                               (ctypes.c_uint32 * de.size)(*[int(v) for v in de.reshape(-1)]),
                               ctypes.c_void_p(coef.data_ptr()), ITX_KEEP_COEFS | ITX_DC_DEFER, _stream_ptr(None)) == 0
    lf = LoopFilterMeta(fr["lf"])
    po, pd = other.picture(), Frame(320, 192, 10, 1).picture()
    assert L.mi_deblock_frame_dc(gpu.h, ctypes.byref(po), ctypes.byref(pd), ctypes.byref(lf.s), _stream_ptr(None)) == -22
    # the DEFER flag needs the runs table
    ss = (ctypes.c_uint32 * 20)(*[0] * 20)
    assert L.mi_itx_frame(gpu.h, ctypes.byref(pa), ctypes.c_void_p(blocks.data_ptr()), ss,
                          ctypes.c_void_p(coef.data_ptr()), ITX_DC_DEFER, _stream_ptr(None)) == -22


def test_deferred_dc_under_graph_capture(gpu):
    # captured, the deferral is not taken (a tag fixed in the graph could match a previous
    # replay's entries): replaying the graph gives the plain order's picture
    fr, blk, bs, de = _inputs(640, 360, 10, 1, seed=8)
    w, h = 640, 360
    A, D = Frame(w, h, 10, 1), Frame(w, h, 10, 1)
    blocks = torch.from_numpy(blk.view(np.uint8).copy()).cuda()
    coef = torch.from_numpy(fr["coef"].copy()).cuda()
    lf = LoopFilterMeta(fr["lf"])
    pa, pd = A.picture(), D.picture()
    bsa = (ctypes.c_uint32 * bs.size)(*[int(v) for v in bs.reshape(-1)])
    dea = (ctypes.c_uint32 * de.size)(*[int(v) for v in de.reshape(-1)])
    L = lib()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert L.mi_itx_frame_runs(gpu.h, ctypes.byref(pa), ctypes.c_void_p(blocks.data_ptr()), bsa, dea,
                                   ctypes.c_void_p(coef.data_ptr()), ITX_KEEP_COEFS | ITX_DC_DEFER, _stream_ptr(s)) == 0
        assert L.mi_deblock_frame_dc(gpu.h, ctypes.byref(pa), ctypes.byref(pd), ctypes.byref(lf.s), _stream_ptr(s)) == 0
    for p, a in enumerate(fr["planes"]):
        A.set_plane_np(p, a)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    ref = _oracle(fr)
    for p in range(3):
        got = D.plane_np(p)
        ph, pw = got.shape
        assert np.array_equal(got, ref[p][:ph, :pw]), p


# ---- the deferral's state on the context (the tag, what is pending, the map) ----
# Each test has a context of its own: the session context's tag and pending state cannot leak
# into it, nor its own out.

@pytest.fixture
def own_ctx(gpu):
    from rav1d_amd.frame import Context
    c = Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()


class _Calls:
    """One frame's device inputs and the two calls on a context, returning their status."""

    def __init__(self, ctx, fr, blk, bs, de):
        self.ctx, self.fr = ctx, fr
        self.A = Frame(fr["w"], fr["h"], fr["bpc"], fr["layout"])
        self.load(fr["planes"])
        self.blocks = torch.from_numpy(blk.view(np.uint8).copy()).cuda()
        self.coef = torch.from_numpy(fr["coef"].copy()).cuda()
        self.bsa = (ctypes.c_uint32 * bs.size)(*[int(v) for v in bs.reshape(-1)])
        self.dea = (ctypes.c_uint32 * de.size)(*[int(v) for v in de.reshape(-1)])
        self.lf = LoopFilterMeta(fr["lf"])

    def load(self, planes):
        for p, a in enumerate(planes):
            self.A.set_plane_np(p, a)

    def new_frame(self):
        return Frame(self.fr["w"], self.fr["h"], self.fr["bpc"], self.fr["layout"])

    def itx(self, defer, blocks=True, stream=None):
        pa = self.A.picture()
        return lib().mi_itx_frame_runs(self.ctx.h, ctypes.byref(pa), ctypes.c_void_p(self.blocks.data_ptr() if blocks else 0),
                                       self.bsa, self.dea, ctypes.c_void_p(self.coef.data_ptr()),
                                       ITX_KEEP_COEFS | (ITX_DC_DEFER if defer else 0), _stream_ptr(stream))

    def deblock_dc(self, dst, stream=None):
        pa, pd = self.A.picture(), dst.picture()
        rc = lib().mi_deblock_frame_dc(self.ctx.h, ctypes.byref(pa), ctypes.byref(pd), ctypes.byref(self.lf.s),
                                       _stream_ptr(stream))
        if stream is None:
            torch.cuda.synchronize()
        return rc


def _same(frame, ref, what):
    for p in range(len(frame.planes)):
        got = frame.plane_np(p)
        ph, pw = got.shape
        if not np.array_equal(got, ref[p][:ph, :pw]):
            bad = np.argwhere(got != ref[p][:ph, :pw])
            y, x = bad[0]
            raise AssertionError(f"{what}: plane {p}: {len(bad)} pixels differ, first at x={x} y={y}: "
                                 f"got {got[y, x]}, expected {ref[p][y, x]}")


def _oracle_deblock(fr, planes):
    w, h, bpc, layout = fr["w"], fr["h"], fr["bpc"], fr["layout"]
    return oracle_lib.deblock_frame(pad_planes(planes, w, h, bpc, layout), bpc, layout, w, h, fr["lf"], sb128=1)


def _other_planes(fr, seed):
    from rav1d_amd.synth import make_mixed_texture
    rng = np.random.default_rng(seed)
    return [make_mixed_texture(rng, p.shape[1], p.shape[0], fr["bpc"]) for p in fr["planes"]]


def test_failed_deferring_call_leaves_nothing_pending(own_ctx):
    """a deferring call refused after its tag was drawn (no block array) defers nothing: an in-place
    mi_deblock_frame_dc is then the plain in-place deblock, not refused for a deferral that does
    not exist"""
    fr, blk, bs, de = _inputs(256, 192, 10, 1, seed=21)
    c = _Calls(own_ctx, fr, blk, bs, de)
    assert c.itx(defer=True, blocks=False) == -22
    assert c.deblock_dc(c.A) == 0
    _same(c.A, _oracle_deblock(fr, fr["planes"]), "in place after a failed deferral")
    B = c.new_frame()
    for p, a in enumerate(fr["planes"]):
        B.set_plane_np(p, a)
    pb = B.picture()
    assert lib().mi_deblock_frame(own_ctx.h, ctypes.byref(pb), ctypes.byref(c.lf.s), _stream_ptr(None)) == 0
    torch.cuda.synchronize()
    for p in range(3):
        assert np.array_equal(c.A.buffer_np(p), B.buffer_np(p)), p


def test_later_itx_call_supersedes_a_deferral(own_ctx):
    """deferral, source restored, the same blocks again without the flag: the DC runs are in the
    pixels now, and mi_deblock_frame_dc must not add the superseded deferral's on top"""
    fr, blk, bs, de = _inputs(256, 192, 10, 1, seed=22)
    assert (de > bs[:, :-1]).any()
    c = _Calls(own_ctx, fr, blk, bs, de)
    assert c.itx(defer=True) == 0
    torch.cuda.synchronize()
    c.load(fr["planes"])
    assert c.itx(defer=False) == 0
    D = c.new_frame()
    assert c.deblock_dc(D) == 0
    _same(D, _oracle(fr), "plain order after a superseded deferral")


def test_plain_deblock_calls_drop_a_pending_deferral(own_ctx):
    """mi_deblock_frame_to and mi_deblock_frame do not add a deferral, and it does not survive
    them: new planes, no itx call, then mi_deblock_frame_dc is the deblock of the new planes"""
    fr, blk, bs, de = _inputs(256, 192, 10, 1, seed=23)
    c = _Calls(own_ctx, fr, blk, bs, de)
    for k, in_place in enumerate((False, True)):
        c.load(fr["planes"])
        assert c.itx(defer=True) == 0
        T = c.new_frame()
        pa, pt = c.A.picture(), T.picture()
        if in_place:
            assert lib().mi_deblock_frame(own_ctx.h, ctypes.byref(pt), ctypes.byref(c.lf.s), _stream_ptr(None)) == 0
        else:
            assert lib().mi_deblock_frame_to(own_ctx.h, ctypes.byref(pa), ctypes.byref(pt), ctypes.byref(c.lf.s),
                                             _stream_ptr(None)) == 0
        torch.cuda.synchronize()
        planes = _other_planes(fr, 230 + k)
        c.load(planes)
        D = c.new_frame()
        assert c.deblock_dc(D) == 0
        _same(D, _oracle_deblock(fr, planes), "after mi_deblock_frame" + ("" if in_place else "_to"))


def test_pending_deferral_is_refused_under_capture(own_ctx):
    """a deferral made outside a capture must not be baked into a graph: the captured
    mi_deblock_frame_dc is refused and enqueues nothing, the deferral stays pending, and the
    uncaptured call after the capture consumes it"""
    fr, blk, bs, de = _inputs(256, 192, 10, 1, seed=24)
    c = _Calls(own_ctx, fr, blk, bs, de)
    D = c.new_frame()
    assert c.itx(defer=True) == 0
    torch.cuda.synchronize()
    scratch = torch.zeros(64, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = c.deblock_dc(D, stream=s)
        scratch.add_(1)          # one valid captured operation: the graph is not empty
    torch.cuda.synchronize()
    assert rc == -22
    assert c.deblock_dc(D) == 0
    _same(D, _oracle(fr), "the deferral consumed after the capture")


def _full_cover_blocks(w, h, layout):
    """64x64 DC-only blocks over every 128-aligned plane area: every unit of the DC map"""
    from rav1d_amd import TXBLOCK_DTYPE
    aw, ah = (w + 127) & ~127, (h + 127) & ~127
    ssh, ssv = int(layout in (1, 2)), int(layout == 1)
    recs = []
    for p, (pw, ph) in enumerate([(aw, ah), (aw >> ssh, ah >> ssv), (aw >> ssh, ah >> ssv)]):
        for y in range(0, ph, 64):
            for x in range(0, pw, 64):
                recs.append((len(recs), x, y, p, 4, 0, 0, 0))
    return np.array(recs, dtype=TXBLOCK_DTYPE), [ah, ah >> ssv, ah >> ssv]


def test_tag_wrap_does_not_revive_old_entries(own_ctx):
    """The 16-bit tag wraps after 65535 deferring calls; the entries an earlier call wrote under
    the tag value that comes round again must not be added. Through the public API only: one
    deferral tags every unit of the map (tag 1), 65534 deferring calls with empty tables advance
    the tag and launch nothing, then a deferral over part of the picture draws tag 1 again."""
    w, h, bpc, layout = 256, 192, 10, 1
    L = lib()
    blocks, heights = _full_cover_blocks(w, h, layout)
    coef = np.full(len(blocks), 4000, np.int32)          # 64x64: a constant of +31 per pixel
    rng = np.random.default_rng(25)
    planes = [rng.integers(100, 900, size=s).astype(np.uint16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    A, D = Frame(w, h, bpc, layout), Frame(w, h, bpc, layout)
    for p, a in enumerate(planes):
        A.set_plane_np(p, a)
    pa, pd = A.picture(), D.picture()
    sp = _stream_ptr(None)
    cdev = torch.from_numpy(coef).cuda()
    lf = LoopFilterMeta(dict(_inputs(w, h, bpc, layout, seed=26)[0]["lf"], filter_y=0))

    def defer(blk):
        blk, _, bs = itx_band_order(blk, heights)
        de = itx_dc_runs(blk, bs)
        assert (de == bs[:, 1:]).all() and len(blk)
        bdev = torch.from_numpy(blk.view(np.uint8).copy()).cuda()
        rc = L.mi_itx_frame_runs(own_ctx.h, ctypes.byref(pa), ctypes.c_void_p(bdev.data_ptr()),
                                 (ctypes.c_uint32 * bs.size)(*[int(v) for v in bs.reshape(-1)]),
                                 (ctypes.c_uint32 * de.size)(*[int(v) for v in de.reshape(-1)]),
                                 ctypes.c_void_p(cdev.data_ptr()), ITX_KEEP_COEFS | ITX_DC_DEFER, sp)
        torch.cuda.synchronize()
        return rc

    assert defer(blocks) == 0
    assert L.mi_deblock_frame_dc(own_ctx.h, ctypes.byref(pa), ctypes.byref(pd), ctypes.byref(lf.s), sp) == 0
    torch.cuda.synchronize()
    full = oracle_lib.itx_frame(pad_planes(planes, w, h, bpc, layout), blocks, coef.copy(), bpc)
    for p in range(3):
        got = D.plane_np(p)
        assert np.array_equal(got, full[p][:got.shape[0], :got.shape[1]]) and (got != planes[p]).all(), p
    zb, zd, none = (ctypes.c_uint32 * 171)(), (ctypes.c_uint32 * 152)(), ctypes.c_void_p(0)
    call, ctxh, pic, fl = L.mi_itx_frame_runs, own_ctx.h, ctypes.byref(pa), ITX_KEEP_COEFS | ITX_DC_DEFER
    bad = 0
    for _ in range(65534):
        bad |= call(ctxh, pic, none, zb, zd, none, fl, sp)
    assert bad == 0
    part = blocks[(blocks["x"] == 0) & (blocks["y"] == 0)]        # the top-left block of each plane
    assert len(part) == 3
    assert defer(part) == 0
    assert L.mi_deblock_frame_dc(own_ctx.h, ctypes.byref(pa), ctypes.byref(pd), ctypes.byref(lf.s), sp) == 0
    torch.cuda.synchronize()
    ref = oracle_lib.itx_frame(pad_planes(planes, w, h, bpc, layout), part, coef.copy(), bpc)
    _same(D, ref, "after the tag wrapped")
    for p in range(3):     # units outside the runs got no DC
        assert np.array_equal(D.plane_np(p)[64:], planes[p][64:]) and np.array_equal(D.plane_np(p)[:, 64:], planes[p][:, 64:])
