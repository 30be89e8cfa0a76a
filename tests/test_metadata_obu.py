"""CPU: the front-end's metadata OBUs (include/mi_av1dec.h: MiContentLight, MiMasteringDisplay,
MiItutT35 of every event, mi_dec_event_metadata). The model is a bit reader of its own that restates the three syntaxes of
the AV1 specification (5.8.2 - 5.8.4) and the lifetime rules of the header over the OBUs of a
stream; the streams are the golden vectors that carry metadata, and cases spliced into a small
vector."""
import errno

import pytest

from rav1d_amd.av1dec import Av1Decoder, DecoderError, _leb128, stream_events, stream_units
from tests.stream_lib import stream

NONE = (None, None, None)


class _Bits:
    def __init__(self, data):
        self.d, self.p = data, 0

    def f(self, n):
        v = 0
        for _ in range(n):
            if self.p >= 8 * len(self.d):
                raise ValueError("overrun")
            v = (v << 1) | ((self.d[self.p >> 3] >> (7 - (self.p & 7))) & 1)
            self.p += 1
        return v


def obus(unit):
    """(type, has_extension, temporal_id, spatial_id, payload) of every OBU of a decoder input."""
    off = 0
    while off < len(unit):
        h = unit[off]
        typ, ext, has_size = (h >> 3) & 0xf, (h >> 2) & 1, (h >> 1) & 1
        tid, sid = (unit[off + 1] >> 5, (unit[off + 1] >> 3) & 3) if ext else (0, 0)
        off += 1 + ext
        if has_size:
            ln, n = _leb128(unit, off)
            off += n
        else:
            ln = len(unit) - off
        yield typ, ext, tid, sid, unit[off:off + ln]
        off += ln


def seq_facts(payload):
    """(reduced_still_picture_header, operating_point_idc[0]) of a sequence header (5.5.1)."""
    b = _Bits(payload)
    b.f(3)
    b.f(1)
    if b.f(1):
        return 1, 0
    if b.f(1):                       # timing_info_present_flag
        b.f(32)
        b.f(32)
        if b.f(1):                   # equal_picture_interval: uvlc
            z = 0
            while not b.f(1):
                z += 1
            b.f(z)
        if b.f(1):                   # decoder_model_info_present_flag
            b.f(5 + 32 + 5 + 5)
    b.f(1)
    b.f(5)
    return 0, b.f(12)


def parse_metadata(payload):
    """('cll', (max_cll, max_fall)) / ('mdcv', (primaries, white, max, min)) / ('t35', (cc, ext,
    bytes)) / None for what is ignored; ValueError for a CLL / MDCV payload that is too short."""
    typ, n = _leb128(payload, 0)
    b = _Bits(payload[n:])
    if typ == 1:
        v = (b.f(16), b.f(16))
        b.f(1)
        return "cll", v
    if typ == 2:
        pri = tuple((b.f(16), b.f(16)) for _ in range(3))
        v = (pri, (b.f(16), b.f(16)), b.f(32), b.f(32))
        b.f(1)
        return "mdcv", v
    if typ == 4:
        body = payload[n:].rstrip(b"\0")[:-1]        # the trailing-bit byte and what follows it
        if not body:
            return None
        cc, ext, k = body[0], 0, 1
        if cc == 0xff:
            if len(body) < 2:
                return None
            ext, k = body[1], 2
        return ("t35", (cc, ext, bytes(body[k:]))) if len(body) > k else None
    return None


def model(units):
    """The (cll, mdcv, t35) each submitted frame takes, in decode order: the index is the frame's
    picture id, which is what a shown event names."""
    cll = mdcv = t35 = seq = None
    reduced, idc = 0, 0
    pending = tiles = False
    frames = []

    def submit():
        nonlocal t35, pending, tiles
        frames.append((cll, mdcv, t35))
        t35, pending, tiles = None, False, False

    for unit in units:
        for typ, ext, tid, sid, payload in obus(unit):
            if typ not in (1, 2) and ext and idc and not ((idc >> tid) & 1 and (idc >> (sid + 8)) & 1):
                continue
            if pending and tiles and typ != 4:
                submit()                             # (the frame's tile groups have ended)
            if typ == 1:
                if seq is not None and payload != seq:
                    cll = mdcv = None
                seq = payload
                reduced, idc = seq_facts(payload)
            elif typ in (3, 6) or (typ == 7 and not pending):
                if reduced or not payload[0] >> 7:   # not show_existing_frame
                    pending, tiles = True, typ == 6
            elif typ == 4:
                tiles = True
            elif typ == 5:
                m = parse_metadata(payload)
                if m and m[0] == "cll":
                    cll = m[1]
                elif m and m[0] == "mdcv":
                    mdcv = m[1]
                elif m:
                    t35 = m[1]
    if pending and tiles:
        submit()
    return frames


def fields(ev):
    """(cll, mdcv, t35) of an event in the model's terms (copies)."""
    c, m, t = ev.content_light, ev.mastering_display, ev.itut_t35
    cll = (c.max_cll, c.max_fall) if c.present else None
    mdcv = ((tuple((p[0], p[1]) for p in m.primaries), (m.white_point[0], m.white_point[1]), m.max_luminance,
             m.min_luminance) if m.present else None)
    t35 = (t.country_code, t.country_code_ext, ev.t35_payload) if ev.t35_payload is not None else None
    assert (t.size > 0) == (ev.t35_payload is not None) and (t35 is None or len(ev.t35_payload) == t.size)
    return cll, mdcv, t35


def shown(units):
    """[(show_pic, fields)] of the shown events, and {pic_id: fields} of the events that show
    nothing (they report their own frame's)."""
    dec, out, hidden, n = Av1Decoder(), [], {}, 0
    for u in units:
        dec.send(u)
        for ev in dec.events():
            if ev.frame:
                assert ev.pic_id == n
                n += 1
            if ev.show_pic >= 0:
                out.append((ev.show_pic, fields(ev)))
            elif ev.frame:
                hidden[ev.pic_id] = fields(ev)
    return out, hidden, n


@pytest.mark.parametrize("name, kinds", [("itut_t35", {"t35"}), ("itut_t35_10bit", {"t35", "cll", "mdcv"}),
                                         ("av1-1-b8-03-sizeup", {"cll", "mdcv"}), ("test5606", {"cll"}),
                                         ("test15240", {"t35", "mdcv"})])
def test_golden_streams(name, kinds):
    _, data = stream(name)
    units = list(stream_units(data))
    want = model(units)
    got, hidden, n = shown(units)
    assert n == len(want) and got
    seen = set()
    for pic, f in got + sorted(hidden.items()):
        assert f == want[pic], (name, pic)
        seen |= {k for k, v in zip(("cll", "mdcv", "t35"), f) if v is not None}
    # (test15240's T.35 message goes to a frame that is decoded and never shown)
    assert seen == kinds
    # stream_events hands out the same
    again = [(ev.show_pic, fields(ev)) for ev in stream_events(data) if ev.show_pic >= 0]
    assert again == got


# ---- spliced cases ----

BASE = "av1-1-b8-01-size-16x16"


def leb(v):
    out = b""
    while True:
        out += bytes([(v & 0x7f) | (0x80 if v >> 7 else 0)])
        v >>= 7
        if not v:
            return out


def obu(typ, payload):
    return bytes([(typ << 3) | 2]) + leb(len(payload)) + payload


def meta(typ, body, trailing=b"\x80"):
    return obu(5, leb(typ) + body + trailing)


def cll(a, b):
    return meta(1, a.to_bytes(2, "big") + b.to_bytes(2, "big"))


def mdcv(pri, white, mx, mn):
    body = b"".join(v.to_bytes(2, "big") for p in pri for v in p) + b"".join(v.to_bytes(2, "big") for v in white)
    return meta(2, body + mx.to_bytes(4, "big") + mn.to_bytes(4, "big"))


def splice(unit, extra):
    """`extra` in front of the unit's first frame header or frame OBU."""
    off = 0
    while off < len(unit):
        h = unit[off]
        if (h >> 3) & 0xf in (3, 6):
            return unit[:off] + extra + unit[off:]
        ext = (h >> 2) & 1
        ln, n = _leb128(unit, off + 1 + ext)
        off += 1 + ext + n + ln
    raise AssertionError("no frame in the unit")


def base_units():
    units = list(stream_units(stream(BASE)[1]))
    assert len(units) >= 2
    return units


def first_fields(extra, units=None):
    units = base_units() if units is None else units
    got, _, _ = shown([splice(units[0], extra)] + units[1:2])
    assert len(got) == 2
    return [f for _, f in got]


def test_cll_and_mdcv_extremes():
    pri = ((0, 0xffff), (0xffff, 0), (0x1234, 0xfedc))
    for a, b, mx, mn in ((0, 0xffff, 0, 0xffffffff), (0xffff, 0, 0xffffffff, 0), (1000, 400, 1000 << 8, 50)):
        got = first_fields(cll(a, b) + mdcv(pri, (0xffff, 0), mx, mn))
        assert got[0] == ((a, b), (pri, (0xffff, 0), mx, mn), None)
        assert got[1] == got[0]                      # both persist from picture to picture


def test_t35_forms():
    # an extension byte after country code 0xff
    assert first_fields(meta(4, b"\xff\x12\x01\x02\x03"))[0] == (None, None, (0xff, 0x12, b"\x01\x02\x03"))
    # zero bytes in front of the trailing-bit byte belong to the payload; what follows it is cut
    assert first_fields(meta(4, b"\xb5\xab\x00\x00", b"\x80\x00\x00"))[0] == (None, None, (0xb5, 0, b"\xab\x00\x00"))
    # nothing after the country code (and its extension): malformed, ignored, no error
    assert first_fields(meta(4, b"\xb5"))[0] == NONE
    assert first_fields(meta(4, b"\xff\x12"))[0] == NONE
    assert first_fields(meta(4, b""))[0] == NONE


def test_t35_belongs_to_one_frame():
    got = first_fields(meta(4, b"\xb5first") + meta(4, b"\x26second"))
    assert got[0] == (None, None, (0x26, 0, b"second"))      # the last one wins
    assert got[1] == NONE                                     # and is gone with its frame


def test_short_cll_is_an_error():
    units = base_units()
    whole = leb(1) + b"\x03\xe8\x01\x90\x80"
    dec = Av1Decoder()
    with pytest.raises(DecoderError) as e:
        dec.send(splice(units[0], obu(5, whole[:-1])))
    assert e.value.code == -errno.EINVAL
    # an MDCV cut likewise; the whole CLL is fine
    with pytest.raises(DecoderError) as e:
        Av1Decoder().send(splice(units[0], obu(5, leb(2) + bytes(24))))
    assert e.value.code == -errno.EINVAL
    assert first_fields(obu(5, whole))[0] == ((1000, 400), None, None)


def test_other_types_are_ignored():
    extra = meta(3, b"\x00\x01\x02") + meta(5, b"\x12\x34\x56\x78") + meta(31, b"\xde\xad") + meta(0, b"\x01")
    assert first_fields(extra) == [NONE] * 2


def test_cll_survives_a_repeated_sequence_header():
    units = base_units()
    seq = next(obu(1, p) for t, _, _, _, p in obus(units[0]) if t == 1)
    units = [units[0], splice(units[1], seq)]
    assert first_fields(cll(600, 200), units) == [((600, 200), None, None)] * 2


def test_a_changed_sequence_header_clears():
    a, b = base_units(), list(stream_units(stream("av1-1-b8-01-size-66x66")[1]))
    seq = [next(p for t, _, _, _, p in obus(u[0]) if t == 1) for u in (a, b)]
    if seq[0] == seq[1]:
        pytest.skip("the two vectors share one sequence header")
    pri = ((1, 2), (3, 4), (5, 6))
    got, _, _ = shown([splice(a[0], cll(600, 200) + mdcv(pri, (7, 8), 9, 10)), a[1], b[0], b[1]])
    assert [f for _, f in got] == [((600, 200), (pri, (7, 8), 9, 10), None)] * 2 + [NONE] * 2


def test_the_entry_itself():
    """mi_dec_event_metadata: zero before the first event, -EINVAL for a NULL argument, and the
    MiDecEvent struct is left as it was (its metadata is beside it, not inside)."""
    import ctypes

    from rav1d_amd.av1dec import MiDecEvent, MiDecMetadata, dec_lib
    L = dec_lib()
    dec = Av1Decoder()
    md = MiDecMetadata()
    md.content_light.present = 7
    assert L.mi_dec_event_metadata(dec.h, ctypes.byref(md)) == 0
    assert (md.content_light.present, md.mastering_display.present, md.itut_t35.size, md.itut_t35.payload) == (0, 0, 0, None)
    assert L.mi_dec_event_metadata(None, ctypes.byref(md)) == -errno.EINVAL
    assert L.mi_dec_event_metadata(dec.h, None) == -errno.EINVAL
    assert [f[0] for f in MiDecEvent._fields_][-1] == "color"
    units = base_units()
    dec.send(splice(units[0], cll(321, 123) + meta(4, b"\xb5xyz")))
    evs = list(dec.events())
    assert evs and L.mi_dec_event_metadata(dec.h, ctypes.byref(md)) == 0     # still the last event's
    assert (md.content_light.present, md.content_light.max_cll, md.content_light.max_fall) == (1, 321, 123)
    assert ctypes.string_at(md.itut_t35.payload, md.itut_t35.size) == b"xyz" and md.itut_t35.country_code == 0xb5
