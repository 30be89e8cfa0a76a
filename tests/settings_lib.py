"""Stream decode with the decoder settings of include/mi_av1dec.h (operating point, all layers,
decode frame type, frame size limit): the event loop of tests/stream_lib.py's decode_stream with
those settings passed on, and with the checks every event stream has to pass whatever the
settings are. The fixtures are tests/golden/settings/ (tools/make_stream_fixtures.py).

TEST INFRASTRUCTURE ONLY.
"""
import hashlib
import json
import os
from collections import namedtuple

from tests import oracle_lib
from tests.stream_lib import md5_update_picture, oracle_frame

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = os.path.join(HERE, "golden", "settings")
VECTORS = json.load(open(os.path.join(SETTINGS, "vectors.json")))

Decoded = namedtuple("Decoded", "md5 sizes events")
# events: one (pic_id or -1, show_pic, (release...), temporal_id, spatial_id, new_temporal_unit)
# tuple per event, for comparing whole event streams


def vector(name):
    return next(v for v in VECTORS if v["name"] == name)


def load(v):
    """The bytes of a vector: `file` under tests/golden/settings/ (or, for the streams the other
    suites already hold, a path into tests/golden/streams/), or its `parts` joined."""
    names = v.get("parts") or [v["file"]]
    return b"".join(open(os.path.join(SETTINGS, n), "rb").read() for n in names)


def settings_of(v):
    a = v["args"]
    return dict(operating_point=a["oppoint"], all_layers=bool(a["alllayers"]), decode_frame_type=a["decodeframetype"])


def check_event(ev, have, released):
    """The invariants of one event against the pictures produced so far (`have`: ids of frames
    whose event was handed out) and the ids released so far; updates both."""
    if ev.frame:
        assert ev.pic_id >= 0 and ev.pic_id not in have, f"picture {ev.pic_id} produced twice"
        have.add(ev.pic_id)
        for r in ev.ref_pic:
            assert r < 0 or (r in have and r not in released), f"frame {ev.pic_id} reads picture {r}"
    if ev.show_pic >= 0:
        assert ev.show_pic in have, f"event shows picture {ev.show_pic}, never produced"
        assert ev.show_pic not in released, f"event shows picture {ev.show_pic} after its release"
    for i in range(ev.n_release):
        r = ev.release[i]
        assert r in have, f"release of picture {r}, never produced"
        assert r not in released, f"picture {r} released twice"
        released.add(r)


def decode_settings(data, recon=oracle_frame, threads=1, apply_grain=False, **settings):
    """Decode a stream through the front-end with `settings` (Av1Decoder's) and `recon` (the
    oracle by default); returns Decoded(md5 of the shown pictures as the md5 muxer hashes them,
    [(w, h)] of the shown pictures, the event stream)."""
    from rav1d_amd.av1dec import stream_events
    pics, have, released = {}, set(), set()
    md5 = hashlib.md5()
    sizes, events = [], []
    for ev in stream_events(data, threads, **settings):
        check_event(ev, have, released)
        if ev.frame:
            fr = ev.frame.contents
            refs = [None] * 7
            for i in range(7):
                r = ev.ref_pic[i]
                if r >= 0:
                    refs[i] = pics[r][:3]
            planes = recon(fr, refs) if recon else None
            pics[ev.pic_id] = (planes, fr.up_w, fr.h, fr.layout, fr.bpc)
        if ev.show_pic >= 0:
            planes, w, h, layout, bpc = pics[ev.show_pic]
            if recon:
                if apply_grain and ev.fg_present:
                    planes = oracle_lib.film_grain(planes, bpc, layout, w, h, ev.fg, ev.mtrx_identity)
                md5_update_picture(md5, planes, w, h, layout)
            sizes.append((w, h))
        events.append((ev.pic_id if ev.frame else -1, ev.show_pic, tuple(ev.release[i] for i in range(ev.n_release)),
                       ev.temporal_id, ev.spatial_id, ev.new_temporal_unit))
        for i in range(ev.n_release):
            pics.pop(ev.release[i], None)
    return Decoded(md5.hexdigest(), sizes, events)
