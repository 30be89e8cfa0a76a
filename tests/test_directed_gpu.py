"""GPU parity over the directed inputs of tests/directed_filters.py: every device route of the
three in-loop filters against the plain oracle, bit-exact. tests/test_directed_census.py shows
on the CPU what these frames reach (every deblock comparison at its limit and one past it,
direction ties, the Wiener clips, the u32 products of the self-guided filter past 2^31, ...)
and that each single-decision mutant of the oracle changes at least one of their pixels."""
import ctypes

import numpy as np
import pytest
import torch

from rav1d_amd import lib
from rav1d_amd.frame import CdefMeta, Frame, LrMeta, cdef_frame, lr_frame
from rav1d_amd.synth import SGR_PARAMS
from tests import directed_filters as D
from tests.test_directed_census import run_cdef, run_lf, run_lr
from tests.test_dsp_calls_gpu import P, _o
from tests.test_lf_gpu import run_gpu as run_deblock_gpu
from tests.test_lr_gpu import to_frame

pytestmark = pytest.mark.gpu


def assert_planes(got, ref, what):
    for p, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r), f"{what} plane {p}: first differences at {np.argwhere(g != r)[:4].tolist()}"


@pytest.mark.parametrize("oop", [False, True], ids=["inplace", "tiles"])
@pytest.mark.parametrize("seed", range(len(D.LF_SEEDS)))
@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("bpc", D.BPCS)
def test_deblock_directed(gpu, bpc, layout, seed, oop):
    """In place through the two-pass kernels, and out of place through the tile kernel with a
    poisoned destination and the source checked untouched (tests/test_lf_gpu.run_gpu)."""
    planes, lf, w, h, _ = D.lf_directed(bpc, layout, seed)
    got = run_deblock_gpu(gpu, [p.copy() for p in planes], lf, w, h, bpc, layout, oop)
    assert_planes(got, run_lf(bpc, layout, seed), "deblock")


@pytest.mark.parametrize("ordered", [False, True], ids=["plain", "ordered"])
@pytest.mark.parametrize("seed", range(len(D.CDEF_SEEDS)))
@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("bpc", D.BPCS)
def test_cdef_directed(gpu, bpc, layout, seed, ordered):
    planes, masks, cd, w, h = D.cdef_directed(bpc, layout, seed)
    src, dst = to_frame(planes, w, h, bpc, layout), Frame(w, h, bpc, layout)
    cdef_frame(gpu, src, dst, CdefMeta(masks, cd, geometry=(w, h, layout) if ordered else None))
    torch.cuda.synchronize()
    assert_planes([dst.plane_np(p) for p in range(len(planes))], run_cdef(bpc, layout, seed), "cdef")
    assert_planes([src.plane_np(p) for p in range(len(planes))], planes, "cdef source")


@pytest.mark.parametrize("ordered", [False, True], ids=["plain", "ordered"])
@pytest.mark.parametrize("seed", range(len(D.LR_SEEDS)))
@pytest.mark.parametrize("layout", D.LAYOUTS)
@pytest.mark.parametrize("bpc", D.BPCS)
def test_lr_directed(gpu, bpc, layout, seed, ordered):
    c, d, lr, w, h = D.lr_directed(bpc, layout, seed)
    fo = Frame(w, h, bpc, layout)
    lr_frame(gpu, to_frame(c, w, h, bpc, layout), to_frame(d, w, h, bpc, layout), fo,
             LrMeta(lr, geometry=(w, h, layout) if ordered else None))
    torch.cuda.synchronize()
    assert_planes([fo.plane_np(p) for p in range(len(c))], run_lr(bpc, layout, seed), "lr")


# ---------------------------------------------------------------------------------------
# The per-call table entries on patches of the directed frames
# ---------------------------------------------------------------------------------------

M = 16      # margin around a plane, so that every window a call may stage lies inside the buffer


def margin(a):
    return np.ascontiguousarray(np.pad(a, M, mode="edge"))


@pytest.mark.parametrize("direction", [0, 1], ids=["cols", "rows"])
@pytest.mark.parametrize("cls", [0, 1], ids=["luma", "chroma"])
@pytest.mark.parametrize("bpc", D.BPCS)
def test_loop_filter_sb_directed(gpu, bpc, cls, direction):
    """mi_dsp_loop_filter_sb over every edge run of the frames written for this direction; the
    chroma planes of 4:2:0 and 4:4:4 in turn."""
    o = _o()
    bdmax = (1 << bpc) - 1
    for seed, (_, _, dirn, _) in enumerate(D.LF_SEEDS):
        if dirn != direction:
            continue
        layout = 1 if seed % 2 == 0 or not cls else 3
        planes, lf, w, h, _ = D.lf_directed(bpc, layout, seed)
        plane = 1 if cls else 0
        level = np.ascontiguousarray(lf["level"])
        lut = np.zeros(144, np.uint8)
        lut[:64], lut[64:128] = lf["lim_e"], lf["lim_i"]
        ref, got = margin(planes[plane]), margin(planes[plane])
        stride = ref.shape[1]
        runs = D.lf_call_runs(bpc, layout, seed, plane, direction)
        assert len(runs) > 20
        for x, y, vm, lrow, lcol, slot in runs:
            vmask = np.array(vm, np.uint32)
            lv = ctypes.c_void_p(level.ctypes.data + (lrow * lf["b4_stride"] + lcol) * 4 + slot)
            off = (y + M) * stride + x + M
            o.oracle_lf_sb(cls, direction, P(ref, off), ref.strides[0], P(vmask), lv, lf["b4_stride"], P(lut),
                           P(lut, 64), 32, bdmax)
            assert lib().mi_dsp_loop_filter_sb(cls, direction, P(got, off), got.strides[0], P(vmask), lv,
                                               lf["b4_stride"], P(lut), 32, bdmax) == 0
        assert not np.array_equal(ref, margin(planes[plane]))
        assert np.array_equal(got, ref), (seed, np.argwhere(got != ref)[:4].tolist())


@pytest.mark.parametrize("layout", [1, 2, 0], ids=["420", "422", "mono"])
@pytest.mark.parametrize("bpc", D.BPCS)
def test_cdef_calls_directed(gpu, bpc, layout):
    """mi_dsp_cdef_dir on every luma 8x8 block of two directed frames, and mi_dsp_cdef_filter on
    the luma blocks (mono) or the 4x4 / 4x8 chroma blocks, with the frame's strengths in turn
    and the edge flags of the block's place in the frame."""
    o = _o()
    bdmax, bdm8 = (1 << bpc) - 1, bpc - 8
    for seed in (0, 1):
        planes, masks, cd, w, h = D.cdef_directed(bpc, layout, seed)
        luma = margin(planes[0])
        dirs = {}
        for by in range(h // 8):
            for bx in range(w // 8):
                off = (by * 8 + M) * luma.shape[1] + bx * 8 + M
                var_o, var_g = ctypes.c_uint(0), ctypes.c_uint(0)
                d_o = o.oracle_cdef_find_dir(P(luma, off), luma.strides[0], ctypes.byref(var_o), bdmax)
                d_g = lib().mi_dsp_cdef_dir(P(luma, off), luma.strides[0], ctypes.byref(var_g), bdmax)
                assert (d_g, var_g.value) == (d_o, var_o.value), (seed, bx, by)
                dirs[by, bx] = d_o
        plane, fb = (0, 0) if layout == 0 else (1, 2 if layout == 1 else 1)
        bw, bh = (8 if fb == 0 else 4), (4 if fb == 2 else 8)
        src = margin(planes[plane])
        ph, pw = planes[plane].shape
        stride = src.shape[1]
        n = 0
        for by in range(0, ph // bh, 2 if seed else 1):
            for bx in range(pw // bw):
                n += 1
                st = int(D._CDEF_STRENGTHS[n % len(D._CDEF_STRENGTHS)])
                sec = st & 3
                pri, sec = (st >> 2) << bdm8, (sec + (sec == 3)) << bdm8
                if not (pri or sec):
                    continue
                x, y = bx * bw, by * bh
                edges = (1 if x else 0) | (2 if x + bw < pw else 0) | (4 if y else 0) | (8 if y + bh < ph else 0)
                damping = cd["damping"] + bdm8 - (fb > 0)
                d = dirs.get((by * bh // (8 >> (layout == 1)), bx), n % 8)
                off = (y + M) * stride + x + M
                left = np.ascontiguousarray(src[y + M:y + M + bh, x + M - 2:x + M])
                ref, got = src.copy(), src.copy()
                o.oracle_cdef_filter_block(P(ref, off), ref.strides[0], P(src, off), src.strides[0], P(left),
                                           P(src, off - 2 * stride), P(src, off + bh * stride), pri, sec, d, damping,
                                           bw, bh, edges, bdmax)
                assert lib().mi_dsp_cdef_filter(fb, P(got, off), got.strides[0], P(left), P(src, off - 2 * stride),
                                                P(src, off + bh * stride), pri, sec, d, damping, edges, bdmax) == 0
                assert np.array_equal(got, ref), (seed, bx, by, pri, sec, d, damping, edges)


@pytest.mark.parametrize("plane", [0, 1], ids=["luma", "chroma"])
@pytest.mark.parametrize("bpc", D.BPCS)
def test_lr_calls_directed(gpu, bpc, plane):
    """mi_dsp_lr_wiener / mi_dsp_lr_sgr on every unit and stripe of the directed 4:2:0 frames:
    the pixels from C, the rows above and below from D, the columns to the left from C."""
    o = _o()
    I = ctypes.c_int
    o.oracle_lr_wiener.argtypes = [ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_void_p, ctypes.c_void_p, I, I,
                                   ctypes.c_void_p, I, I]
    o.oracle_lr_wiener.restype = None
    o.oracle_lr_sgr.argtypes = [I, ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_void_p, ctypes.c_void_p, I, I,
                                ctypes.c_uint, ctypes.c_uint, I, I, I, I]
    o.oracle_lr_sgr.restype = None
    bdmax = (1 << bpc) - 1
    for seed in range(len(D.LR_SEEDS)):
        c, d, lr, w, h = D.lr_directed(bpc, 1, seed)
        pic, dd = margin(c[plane]), margin(d[plane])
        ph = c[plane].shape[0]
        stride = pic.shape[1]
        for x, y, uw, sh, edges, rec in D.lr_call_units(bpc, 1, seed, plane):
            off = (y + M) * stride + x + M
            left = np.ascontiguousarray(pic[y + M:y + M + sh, x + M - 4:x + M])
            lpf = np.zeros((8, stride), pic.dtype)
            rows = [y - 2, y - 1, min(y + sh, ph - 1), min(y + sh + 1, ph - 1)]
            lpf[[0, 1, 6, 7]] = dd[[r + M for r in rows]]
            ref, got = pic.copy(), pic.copy()
            if rec["type"] == 2:
                f = np.zeros((2, 8), np.int16)
                for k, t in enumerate((rec["filter_h"], rec["filter_v"])):
                    t = [int(v) for v in t]
                    f[k, :7] = t + [-2 * sum(t) + (128 if (k == 1 or bpc > 8) else 0)] + t[::-1]
                o.oracle_lr_wiener(P(ref, off), ref.strides[0], P(left), P(lpf, x + M), uw, sh, P(f), edges, bdmax)
                rc = lib().mi_dsp_lr_wiener(P(got, off), got.strides[0], P(left), P(lpf, x + M), uw, sh, P(f), edges,
                                            bdmax)
            else:
                s0, s1 = SGR_PARAMS[int(rec["type"]) - 3]
                kind = (s0 != 0) + 2 * (s1 != 0) - 1
                w0 = int(rec["sgr_weights"][0])
                w1 = 128 - (w0 + int(rec["sgr_weights"][1]))
                prm = np.zeros(6, np.int16)
                prm.view(np.uint32)[:2] = [s0, s1]
                prm[4:6] = [w0, w1]
                o.oracle_lr_sgr(kind, P(ref, off), ref.strides[0], P(left), P(lpf, x + M), uw, sh, s0, s1, w0, w1,
                                edges, bdmax)
                rc = lib().mi_dsp_lr_sgr(kind, P(got, off), got.strides[0], P(left), P(lpf, x + M), uw, sh, P(prm),
                                         edges, bdmax)
            assert rc == 0
            assert np.array_equal(got, ref), (seed, x, y, uw, sh, edges, int(rec["type"]),
                                              np.argwhere(got != ref)[:4].tolist())
