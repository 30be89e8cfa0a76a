"""The decode loop the stream generators share (rav1d_amd.stream.shown_pictures), on the CPU: the
front-end is real, run_frame and frame_end are recorders. What is pinned is the order of things:
which pictures are shown, when each frame is checked, which references a frame is given, and that
a picture is dropped only when the front-end has released it and the consumer has taken the shown
one. The pixels are the GPU suites' business."""
import functools
import weakref
from collections import namedtuple

import pytest

from rav1d_amd import stream as S
from rav1d_amd.av1dec import stream_events
from tests import stream_lib
from tests.settings_lib import check_event, load, settings_of, vector

# 18x16, a key and an inter frame; two spatial layers, both shown; the same stream with every shown
# picture held back to a later event (the last one to the drain)
NAMES = ["av1-1-b8-01-size-18x16", "svc-L2T1", "svc-L2T1-op0-top"]
HELD_BACK = "svc-L2T1-op0-top"

# one decoder event: its frame's picture (None: no frame) and references (None for -1), the picture
# it shows (-1: none), how many it releases, and the pictures produced and not yet released before it
# and when it shows
Event = namedtuple("Event", "pic_id refs show n_release live_before live_shown")


@functools.lru_cache(maxsize=None)
def replay(name):
    """(data, settings, [Event], the pictures the front-end never released) of a vector: its event
    stream consumed on its own, with settings_lib.check_event's bookkeeping."""
    if name in stream_lib.VECTORS:
        data, settings = stream_lib.stream(name)[1], {}
    else:
        data, settings = load(vector(name)), settings_of(vector(name))
    have, released, events = set(), set(), []
    for ev in stream_events(data, lookahead=0, **settings):
        before = frozenset(have - released)
        pic_id = ev.pic_id if ev.frame else None
        events.append(Event(pic_id, tuple(r if r >= 0 else None for r in ev.ref_pic), ev.show_pic, ev.n_release,
                            before, before | {pic_id} if ev.frame else before))
        check_event(ev, have, released)
    return data, settings, events, frozenset(have - released)


class Token:
    """What a fake picture set's output() gives: it carries the frame's pic_id."""

    def __init__(self, pic_id):
        self.pic_id = pic_id


class FakePictureSet:
    def __init__(self, pic_id):
        self.token = Token(pic_id)

    def output(self):
        return self.token


class Recorder:
    """Stands in for run_frame and frame_end. The k-th run_frame call is the k-th frame of the
    event stream, which gives it its pic_id. `log` holds ("run", pic_id, refs, live), ("end",) and,
    added by drive(), ("yield", pic_id, live): live is the set of picture sets still referenced,
    that is, still held by the loop (nothing here keeps one)."""

    def __init__(self, monkeypatch, events):
        self.ids = iter([e.pic_id for e in events if e.pic_id is not None])
        self.sets = weakref.WeakSet()
        self.log = []
        monkeypatch.setattr(S, "run_frame", self.run_frame)
        monkeypatch.setattr(S, "frame_end", self.frame_end)

    def live(self):
        return frozenset(ps.token.pic_id for ps in self.sets)

    def run_frame(self, ctx, fr, stream=None, refs=None):
        assert ctx is None and fr.w > 0
        ps = FakePictureSet(next(self.ids))
        self.log.append(("run", ps.token.pic_id, tuple(r.pic_id if r is not None else None for r in refs), self.live()))
        self.sets.add(ps)
        return ps

    def frame_end(self, ctx, stream=None):
        self.log.append(("end",))
        self.held_at_end = self.live()      # (of the last call: the loop still holds its pictures there)

    def runs(self):
        return sum(1 for e in self.log if e[0] == "run")


def drive(rec, data, sync_each, settings):
    """Consume the shared loop, logging the yields; returns what is held once the generator is gone."""
    gen = S.shown_pictures(None, data, None, sync_each, **settings)
    for ev, token in gen:
        assert ev.show_pic == token.pic_id
        rec.log.append(("yield", token.pic_id, rec.live()))
    del gen
    return rec.live()


@pytest.mark.parametrize("sync_each", [True, False], ids=["sync", "nosync"])
@pytest.mark.parametrize("name", NAMES)
def test_loop_order(monkeypatch, name, sync_each):
    data, settings, events, never_released = replay(name)
    rec = Recorder(monkeypatch, events)
    held_after = drive(rec, data, sync_each, settings)
    log = rec.log

    # the shown pictures, in order, are the event stream's
    shown = [e.show for e in events if e.show >= 0]
    assert [e[1] for e in log if e[0] == "yield"] == shown and len(shown) > 1
    # every frame is checked once before anything is yielded (sync_each) or not at all in between,
    # and one more check follows the last event
    assert log[-1] == ("end",)
    assert sum(1 for e in log if e[0] == "end") == (rec.runs() if sync_each else 0) + 1
    for i, e in enumerate(log[:-1]):
        if e[0] == "run":
            assert (log[i + 1] == ("end",)) == sync_each
        elif e[0] == "end":
            assert log[i - 1][0] == "run"
    # the whole sequence: each frame's references slot by slot, and the pictures held at every
    # run_frame (the earlier events' releases done) and at every yield (this event's not yet)
    want = []
    for e in events:
        if e.pic_id is not None:
            want.append(("run", e.pic_id, e.refs, e.live_before))
            if sync_each:
                want.append(("end",))
        if e.show >= 0:
            want.append(("yield", e.show, e.live_shown))
    assert log == want + [("end",)]
    assert any(r is not None for e in log if e[0] == "run" for r in e[2]), "no inter frame in the vector"
    if name != NAMES[0]:        # (the two frames of the first vector are never released)
        assert any(e.show >= 0 and e.n_release for e in events[:-1]), "no event shows a picture and releases others"
    # a shown picture is still held when it is yielded, also when an earlier event produced it
    assert all(e[1] in e[2] for e in log if e[0] == "yield")
    if name == HELD_BACK:
        assert all(e.show != e.pic_id for e in events if e.show >= 0)
        assert events[-1].show >= 0 and events[-1].pic_id is None         # the last one comes with the drain
    # at the end only what the front-end never released is held, and nothing outlives the loop
    assert rec.held_at_end == never_released
    assert held_after == frozenset()


@pytest.mark.parametrize("call", [
    lambda data: S.decode_to_batches(None, data, size=(8, 8), fit="nope"),
    lambda data: S.decode_to_batches(None, data, size=(8, 8), batch=0),
    lambda data: S.decode_to_batches(None, data, size=(8, 8), every=0),
    lambda data: S.decode_to_ladder(None, data, [(8, 8)], fit="nope"),
    lambda data: S.decode_to_ladder(None, data, []),
    lambda data: S.decode_ivf(None, data, decode_frame_type="nope"),
], ids=["batches-fit", "batches-batch", "batches-every", "ladder-fit", "ladder-sizes", "ivf-setting"])
def test_argument_errors_come_before_any_decoding(monkeypatch, call):
    data, _, events, _ = replay(NAMES[0])
    rec = Recorder(monkeypatch, events)
    gen = call(data)                 # (a generator: nothing has run yet)
    with pytest.raises(ValueError):
        next(gen)
    assert rec.log == []
