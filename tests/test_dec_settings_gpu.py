"""The reference's explicit test() entries of the sframe, svc and vq_suite lists
(tests/golden/settings/, with the decoder settings each names) decoded on the MI355X: the
front-end's event stream executed by mi_frame_run, shown pictures hashed by the product md5 muxer.
These are the only reference streams with spatial layers (a 2:1 scaled reference on every second
frame), S-frames and mid-stream resolution switches; with all_layers off the picture shown by an
event is not the one it reconstructs, so the device pools have to keep a held-back picture until
the front-end releases it. Expected MD5s are the reference's: exact, no tolerance."""
import pytest

from tests.settings_lib import VECTORS, load, settings_of, vector


def _ivf_md5(ctx, v):
    """decode_ivf, every shown picture read back and written through the md5 muxer."""
    from rav1d_amd.output import Muxer, host_picture_np
    from rav1d_amd.stream import decode_ivf
    m = Muxer("md5")
    sizes = []
    for pic in decode_ivf(ctx, load(v), threads=1, **settings_of(v)):
        planes = [pic.buffer_np(p) for p in range(len(pic.planes))]
        m.write(host_picture_np(planes, pic.w, pic.h, pic.bpc, pic.layout))
        sizes.append((pic.w, pic.h))
    md5 = m.digest()
    m.close()
    return md5, sizes


def _muxer_md5(ctx, v, **kw):
    from rav1d_amd.output import Muxer
    from rav1d_amd.stream import decode_to_muxer
    m = Muxer("md5")
    n = decode_to_muxer(ctx, load(v), m, apply_grain=bool(v["args"]["filmgrain"]), **settings_of(v), **kw)
    md5 = m.digest()
    m.close()
    return md5, n


@pytest.mark.gpu
@pytest.mark.parametrize("v", VECTORS, ids=[v["name"] for v in VECTORS])
def test_gpu_decode_with_settings_matches_reference_md5(gpu, v):
    if v["args"]["filmgrain"]:
        # --filmgrain 1: the grain is applied on the device as the picture is output
        md5, n = _muxer_md5(gpu, v, pipelined=False)
    else:
        md5, sizes = _ivf_md5(gpu, v)
        n = len(sizes)
    assert n > 0
    assert md5 == v["md5"], f"{v['name']}: {n} pictures, md5 {md5} != {v['md5']}"


@pytest.mark.gpu
def test_gpu_top_layer_only_picture_sizes(gpu):
    """all_layers off on the device: 8 pictures, all of the top layer's size."""
    _, sizes = _ivf_md5(gpu, vector("svc-L2T1-op0-top"))
    assert sizes == [(1280, 720)] * 8


LANES = [n for n in ("svc-L2T1-op0-top", "svc-L2T1-op1-top", "svc-L2T1", "svc-L2T2-op0-top", "svc-L2T2-op1-top",
                     "svc-L2T2-op2-top", "svc-L2T2-op3-top", "svc-L2T2")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", LANES)
def test_gpu_pipelined_lanes_keep_the_held_back_picture(gpu, name):
    """decode_to_muxer(pipelined=True): frames alternate over two (context, stream) lanes and the
    front-end runs ahead on its frame threads; a held-back picture is copied out by a later
    event, on the lane that reconstructed it, while the other lane works on the next frame."""
    v = vector(name)
    md5, n = _muxer_md5(gpu, v, pipelined=True)
    assert md5 == v["md5"], f"{name}: {n} pictures, md5 {md5} != {v['md5']}"
