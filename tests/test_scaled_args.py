"""CPU, no device: mi_display_scaled checks its arguments on the host before any device work, with
the NULL context checked last (as mi_display_tensor, tests/test_tensor_args.py). Every rule of the
header has a case that differs from a passing call in the named argument only. Without a context
a passing call is -EINVAL too (for the context alone), so the same two tables run again with a live
context in tests/test_scaled_gpu.py, where PASSING returns 0 and REJECTED still -EINVAL."""
import ctypes
import errno

import pytest

from rav1d_amd import MiPicture, lib
from rav1d_amd.av1dec import MiColorInfo
from rav1d_amd.display import MiScaledImage

BUF = (ctypes.c_uint8 * (1 << 17))()
P = (ctypes.addressof(BUF) + 63) & ~63
E = -errno.EINVAL

# The passing call: a 32 x 16 8-bit 4:2:0 picture to one 8 x 4 8-bit rung, tight strides, no crop,
# chr 0. A case names what it changes:
#   w, h, bpc, layout        the source picture
#   ow, oh, obpc, crop       the rung (crop: (x, y, w, h))
#   stride_y, stride_uv      bytes (default: tight); off_y, off_uv: bytes added to the pointers
#   null                     one of "in", "outs", "y", "uv", "color"
#   n_outs                   the rung is repeated (default 1)
#   chr                      color->chr
BASE = dict(w=32, h=16, bpc=8, layout=1, ow=8, oh=4, obpc=8, crop=None, stride_y=None, stride_uv=None, off_y=0, off_uv=0,
            null=None, n_outs=1, chr=0)

PASSING = [
    ("baseline", {}),
    ("4:0:0 with NULL data[1]", dict(layout=0, null="uv")),
    ("4:2:2", dict(layout=2)),
    ("4:4:4", dict(layout=3)),
    ("NULL color", dict(null="color")),
    ("chr 1", dict(chr=1)),
    ("chr 2", dict(chr=2)),
    ("8 rungs", dict(n_outs=8)),
    ("10-bit source to 8 bits", dict(bpc=10)),
    ("8-bit source to 12 bits", dict(obpc=12)),
    ("padded strides", dict(stride_y=24, stride_uv=40)),
    ("16-bit rows padded by a sample", dict(obpc=10, stride_y=18, stride_uv=18)),
    ("64:1 exactly", dict(w=512, ow=8)),
    ("64:1 exactly through a crop", dict(w=600, ow=8, crop=(88, 0, 512, 16))),
    ("even crop", dict(crop=(2, 4, 20, 10))),
    ("crop of one chroma sample", dict(crop=(30, 14, 2, 2))),
    ("odd crop extents reaching the odd edges", dict(w=33, h=17, crop=(2, 2, 31, 15))),
    ("one luma sample at the odd corner", dict(w=33, h=17, crop=(32, 16, 1, 1))),
    ("4:4:4 odd crop origin and extents", dict(layout=3, crop=(1, 1, 7, 5))),
    ("4:2:2 odd crop row and height", dict(layout=2, crop=(2, 1, 8, 5))),
    ("upscale", dict(ow=100, oh=50)),
]

REJECTED = [
    ("NULL in", dict(null="in")),
    ("NULL outs", dict(null="outs")),
    ("n_outs 0", dict(n_outs=0)),
    ("n_outs 9", dict(n_outs=9)),
    ("NULL data[0]", dict(null="y")),
    ("NULL data[1] with 4:2:0", dict(null="uv")),
    ("NULL data[1] with 4:4:4", dict(layout=3, null="uv")),
    ("w 0", dict(ow=0)),
    ("w -1", dict(ow=-1)),
    ("w 65537", dict(ow=65537)),
    ("h 0", dict(oh=0)),
    ("h 65537", dict(oh=65537)),
    ("bpc 9", dict(obpc=9)),
    ("bpc 16", dict(obpc=16)),
    ("Y stride below the row", dict(stride_y=7)),
    ("Y stride negative", dict(stride_y=-8)),
    ("UV stride below the row", dict(stride_uv=7)),
    ("UV stride below the row of an odd width", dict(ow=9, stride_uv=9)),
    ("Y stride no multiple of the sample", dict(obpc=10, stride_y=17)),
    ("UV stride no multiple of the sample", dict(obpc=12, stride_uv=19)),
    ("Y pointer off the sample", dict(obpc=10, off_y=1)),
    ("UV pointer off the sample", dict(obpc=10, off_uv=1)),
    ("crop past the right edge", dict(crop=(2, 0, 32, 16))),
    ("crop past the bottom edge", dict(crop=(0, 2, 32, 16))),
    ("crop wider than the picture", dict(crop=(0, 0, 34, 16))),
    ("crop_x negative", dict(crop=(-2, 0, 8, 8))),
    ("crop_y negative", dict(crop=(0, -2, 8, 8))),
    ("crop_w zero", dict(crop=(0, 0, 0, 8))),
    ("crop_h zero", dict(crop=(0, 0, 8, 0))),
    ("crop_w negative", dict(crop=(4, 4, -2, 8))),
    ("crop_x odd with 4:2:0", dict(crop=(1, 0, 8, 8))),
    ("crop_x odd with 4:2:2", dict(layout=2, crop=(1, 0, 8, 8))),
    ("crop_y odd with 4:2:0", dict(crop=(0, 1, 8, 8))),
    ("crop_w odd inside the picture, 4:2:0", dict(crop=(0, 0, 7, 8))),
    ("crop_w odd inside the picture, 4:2:2", dict(layout=2, crop=(0, 0, 7, 8))),
    ("crop_h odd inside the picture", dict(crop=(0, 0, 8, 7))),
    ("above 64:1 in x", dict(w=521, ow=8)),
    ("above 64:1 in y", dict(w=64, h=300, ow=8, oh=4)),
    ("above 64:1 through a crop", dict(w=600, ow=8, crop=(0, 0, 514, 16))),
    ("chr 3", dict(chr=3)),
    ("chr -1", dict(chr=-1)),
]


def arguments(case, pic, y_ptr, uv_ptr):
    """The ctypes arguments of a case after the context: `pic` is the MiPicture of the case's
    source (geometry BASE + case), y_ptr / uv_ptr are 64-byte aligned destinations."""
    k = dict(BASE, **case)
    es = 1 if k["obpc"] == 8 else 2
    sh = int(k["layout"] in (1, 2))
    im = MiScaledImage()
    im.w, im.h, im.bpc = k["ow"], k["oh"], k["obpc"]
    im.data[0] = None if k["null"] == "y" else y_ptr + k["off_y"]
    im.data[1] = None if k["null"] == "uv" else uv_ptr + k["off_uv"]
    im.stride[0] = k["stride_y"] if k["stride_y"] is not None else max(k["ow"], 0) * es
    im.stride[1] = k["stride_uv"] if k["stride_uv"] is not None else 2 * ((max(k["ow"], 0) + sh) >> sh) * es
    if k["crop"] is not None:
        im.crop_x, im.crop_y, im.crop_w, im.crop_h = k["crop"]
    outs = (MiScaledImage * max(k["n_outs"], 1))(*([im] * max(k["n_outs"], 1)))
    color = MiColorInfo(1, 1, 1, 0, k["chr"])
    return (ctypes.byref(pic) if k["null"] != "in" else None, outs if k["null"] != "outs" else None, k["n_outs"],
            ctypes.byref(color) if k["null"] != "color" else None, None, None), (outs, color)


def picture(case):
    k = dict(BASE, **case)
    pic = MiPicture()
    for p in range(3):
        pic.data[p] = P + 32768 * p
    pxb = 1 if k["bpc"] == 8 else 2
    pic.stride[0] = pic.stride[1] = max(128, k["w"]) * pxb
    pic.w, pic.h, pic.bpc, pic.layout = k["w"], k["h"], k["bpc"], k["layout"]
    return pic


def call(case):
    pic = picture(case)
    args, _keep = arguments(case, pic, P + 98304, P + 98304 + 8192)
    return lib().mi_display_scaled(None, *args)


@pytest.mark.parametrize("case", [c for _, c in REJECTED], ids=[n for n, _ in REJECTED])
def test_rejected(case):
    assert call(case) == E


@pytest.mark.parametrize("case", [c for _, c in PASSING], ids=[n for n, _ in PASSING])
def test_passing_but_for_the_context(case):
    """Everything but the context passes: -EINVAL for the NULL context, nothing was launched."""
    assert call(case) == E


def test_malformed_source():
    for bad in (dict(bpc=9), dict(layout=4), dict(w=0), dict(h=0)):
        assert call(bad) == E
    pic = picture({})
    pic.stride[0] = 31
    args, _keep = arguments({}, pic, P + 98304, P + 98304 + 8192)
    assert lib().mi_display_scaled(None, *args) == E
    pic = picture({})
    pic.data[2] = None
    args, _keep = arguments({}, pic, P + 98304, P + 98304 + 8192)
    assert lib().mi_display_scaled(None, *args) == E


def test_each_rung_is_checked():
    """A bad rung anywhere in the list rejects the call."""
    pic = picture({})
    (p, outs, _, color, fg, st), _keep = arguments(dict(n_outs=3), pic, P + 98304, P + 98304 + 8192)
    for r in range(3):
        good = outs[r].bpc
        outs[r].bpc = 9
        assert lib().mi_display_scaled(None, p, outs, 3, color, fg, st) == E
        outs[r].bpc = good
