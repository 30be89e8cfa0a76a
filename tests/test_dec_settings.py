"""The front-end's decoder settings (include/mi_av1dec.h: mi_dec_set_operating_point,
mi_dec_set_all_layers, mi_dec_drain, mi_dec_set_decode_frame_type, mi_dec_set_frame_size_limit)
against the reference's own explicit test() entries (tests/dav1d-test-data/8-bit/{sframe,svc,
vq_suite}/meson.build, copied with their arguments into tests/golden/settings/ by
tools/make_stream_fixtures.py), through the front-end and the CPU restatement. The digests are
exact: there is no tolerance.
"""
import ctypes
import errno
import json
import os

import pytest

from tests.settings_lib import VECTORS, decode_settings, load, settings_of, vector

STREAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streams")

_cache = {}


def decoded(name, threads=1, **override):
    """One decode per (vector, threads, settings), shared by the tests that look at it."""
    v = vector(name)
    st = dict(settings_of(v), **override)
    key = (v["file"], threads, bool(v["args"]["filmgrain"]), tuple(sorted(st.items())))
    if key not in _cache:
        _cache[key] = decode_settings(load(v), threads=threads, apply_grain=bool(v["args"]["filmgrain"]), **st)
    return _cache[key]


def test_vector_table():
    """All 26 explicit entries of the three meson lists, with the four arguments each."""
    assert len(VECTORS) == 26 and len({v["name"] for v in VECTORS}) == 26
    for v in VECTORS:
        assert set(v["args"]) == {"oppoint", "alllayers", "decodeframetype", "filmgrain"}
        assert len(v["md5"]) == 32
    assert sum(1 for v in VECTORS if not v["args"]["alllayers"] or v["args"]["decodeframetype"] != "all") == 19


@pytest.mark.parametrize("v", VECTORS, ids=[v["name"] for v in VECTORS])
def test_reference_md5(v):
    r = decoded(v["name"])
    assert r.sizes, "nothing shown"
    assert r.md5 == v["md5"], f"{v['name']}: {len(r.sizes)} pictures, md5 {r.md5} != {v['md5']}"


NO_GRAIN = [v for v in VECTORS if not v["args"]["filmgrain"]]


@pytest.mark.parametrize("v", NO_GRAIN, ids=[v["name"] for v in NO_GRAIN])
def test_reference_md5_frame_threads(v):
    """threads 8: events are popped in decode order while the frames decode on workers; the
    selection was made when the unit was parsed."""
    r = decoded(v["name"], threads=8)
    assert r.md5 == v["md5"], f"{v['name']}: {len(r.sizes)} pictures, md5 {r.md5} != {v['md5']}"
    assert r.events == decoded(v["name"]).events


# L2T1's operating points are 0x301, 0x101; L2T2's 0x303, 0x301, 0x103, 0x101 with temporal ids
# alternating 0 and 1 per temporal unit (8 units, two spatial layers each)
@pytest.mark.parametrize("name,n,size", [
    ("svc-L2T1-op0-top", 8, (1280, 720)), ("svc-L2T1-op1-top", 8, (640, 360)),
    ("svc-L2T2-op0-top", 8, (1280, 720)), ("svc-L2T2-op1-top", 4, (1280, 720)),
    ("svc-L2T2-op2-top", 8, (640, 360)), ("svc-L2T2-op3-top", 4, (640, 360))])
def test_picture_counts_follow_operating_point(name, n, size):
    assert decoded(name).sizes == [size] * n


def test_all_layers_shows_both_spatial_layers():
    r = decoded("svc-L2T1")
    assert r.sizes == [(640, 360), (1280, 720)] * 8
    # the appended event fields: the shown pictures' layers, one temporal unit per pair
    shown = [e for e in r.events if e[1] >= 0]
    assert [e[4] for e in shown] == [0, 1] * 8
    assert [e[5] for e in shown] == [1, 0] * 8
    t = decoded("svc-L2T2")
    assert [e[3] for e in t.events if e[1] >= 0] == [0, 0, 1, 1] * 4


def test_held_back_picture_is_shown_by_a_later_event():
    """all_layers=0: a shown frame's own event never shows it; the base layer is dropped when
    the top layer arrives, the top layer is shown when the next unit starts, the last at drain."""
    r = decoded("svc-L2T1-op0-top")
    frames = [e for e in r.events if e[0] >= 0]
    assert len(frames) == 16 and all(e[1] != e[0] for e in frames)
    assert [e[4] for e in r.events if e[1] >= 0] == [1] * 8
    assert r.events[-1][0] == -1 and r.events[-1][1] >= 0      # the drain event


def test_operating_point_beyond_the_sequence_is_zero():
    assert decoded("svc-L2T1-op0-top", operating_point=5).md5 == vector("svc-L2T1-op0-top")["md5"]
    assert decoded("svc-L2T1-op0-top", operating_point=5).events == decoded("svc-L2T1-op0-top").events


def test_all_layers_off_changes_nothing_with_one_spatial_layer():
    assert decoded("svc-L1T2", all_layers=False).md5 == vector("svc-L1T2")["md5"]
    assert decoded("svc-L1T2", all_layers=False).events == decoded("svc-L1T2").events
    assert decoded("vq_019", all_layers=False).md5 == vector("vq_019")["md5"]
    assert decoded("vq_019", all_layers=False).events == decoded("vq_019").events


def _drive(data, **settings):
    from rav1d_amd.av1dec import Av1Decoder, stream_units
    dec = Av1Decoder(**settings)
    n = 0
    for tu in stream_units(data):
        dec.send(tu)
        n += sum(1 for _ in dec.events())
    return dec, n


def test_draining_twice_adds_nothing():
    for name in ("svc-L2T1-op0-top", "svc-L2T1"):
        dec, _ = _drive(load(vector(name)), **settings_of(vector(name)))
        dec.drain()
        first = [(ev.show_pic, ev.n_release) for ev in dec.events()]
        assert len(first) == (1 if name.endswith("top") else 0)
        dec.drain()
        assert list(dec.events()) == []


def test_no_release_names_a_picture_shown_later():
    """(decode_settings asserts it event by event; here from the recorded streams.)"""
    for v in VECTORS:
        if v["args"]["filmgrain"] or "autostitch" in v["name"]:
            continue
        released = set()
        for _, show, rel, *_ in decoded(v["name"]).events:
            assert show not in released, (v["name"], show)
            released.update(rel)


def _stream_vector(name):
    table = json.load(open(os.path.join(STREAMS, "vectors.json")))
    v = next(t for t in table if t["file"].endswith(os.path.basename(vector(name)["file"])))
    return v, open(os.path.join(STREAMS, v["file"]), "rb").read()


def test_decode_frame_type_key_and_all():
    from rav1d_amd.av1dec import stream_events
    v2, data2 = _stream_vector("vq_002-key")
    # "key": every frame handed out is a key frame, i.e. predicts from nothing and is the only
    # kind left; vq_suite 002 has one
    evs = [(bool(ev.frame), list(ev.ref_pic)) for ev in stream_events(data2, decode_frame_type="key")]
    assert [e for e in evs if e[0]] == [(True, [-1] * 7)]
    assert decoded("vq_002-key").sizes == [(432, 240)]
    # "intra" leaves no inter frame either
    assert all(r < 0 for ev in stream_events(load(vector("vq_001-intra")), decode_frame_type=2) for r in ev.ref_pic)
    # "all" is today's decode
    v1, data1 = _stream_vector("vq_001-intra")
    assert decode_settings(data1, decode_frame_type="all").md5 == v1["md5"]
    assert decode_settings(data2, decode_frame_type=0).md5 == v2["md5"]


def test_bad_values_are_einval():
    from rav1d_amd.av1dec import Av1Decoder, dec_lib
    L = dec_lib()
    h = ctypes.c_void_p()
    assert L.mi_dec_create(ctypes.byref(h)) == 0
    try:
        assert L.mi_dec_set_operating_point(h, -1) == -errno.EINVAL
        assert L.mi_dec_set_operating_point(h, 32) == -errno.EINVAL
        assert L.mi_dec_set_operating_point(h, 31) == 0
        assert L.mi_dec_set_decode_frame_type(h, 4) == -errno.EINVAL
        assert L.mi_dec_set_decode_frame_type(h, -1) == -errno.EINVAL
        assert L.mi_dec_set_decode_frame_type(h, 3) == 0
        assert L.mi_dec_set_all_layers(h, 0) == 0
        assert L.mi_dec_set_frame_size_limit(h, 0) == 0
        assert L.mi_dec_drain(h) == 0
        assert L.mi_dec_drain(None) == -errno.EINVAL
    finally:
        L.mi_dec_destroy(h)
    for bad in (dict(operating_point=-1), dict(operating_point=32), dict(decode_frame_type=4),
                dict(decode_frame_type="keys")):
        with pytest.raises(ValueError):
            Av1Decoder(**bad)


def test_frame_size_limit():
    from rav1d_amd.av1dec import DecoderError
    v, data = _stream_vector("vq_001-intra")
    assert decode_settings(data, frame_size_limit=432 * 240).md5 == v["md5"]
    with pytest.raises(DecoderError) as e:
        _drive(data, frame_size_limit=432 * 240 - 1)
    assert e.value.code == -errno.ERANGE
