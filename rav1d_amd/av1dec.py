"""Host front-end binding: IVF demux (tools/input/ivf.rs) and the C-ABI of
rav1d_amd/libmi_av1dec.so (include/mi_av1dec.h), which parses AV1 OBUs into per-frame work
lists for the gfx950 kernels. No pixels are produced here."""
import ctypes
import os
import struct
import subprocess

from . import MiFilmGrainData

HERE = os.path.dirname(os.path.abspath(__file__))
DEC_PATH = os.environ.get("MI_DEC_LIB") or os.path.join(HERE, "libmi_av1dec.so")

_dec = None


class MiDecFrame(ctypes.Structure):
    _fields_ = [("w", ctypes.c_int32), ("h", ctypes.c_int32), ("up_w", ctypes.c_int32),
                ("render_w", ctypes.c_int32), ("render_h", ctypes.c_int32),
                ("bpc", ctypes.c_int32), ("layout", ctypes.c_int32), ("sb128", ctypes.c_int32),
                ("intra", ctypes.c_void_p), ("intra_tx", ctypes.c_void_p), ("n_intra", ctypes.c_int32),
                ("dep_start", ctypes.c_void_p), ("deps", ctypes.c_void_p), ("n_deps", ctypes.c_int32),
                ("inter_tx", ctypes.c_void_p), ("n_inter_tx", ctypes.c_int32),
                ("coef", ctypes.c_void_p), ("ncoef", ctypes.c_size_t),
                ("idx", ctypes.c_void_p), ("nidx", ctypes.c_size_t),
                ("pal", ctypes.c_void_p), ("npal", ctypes.c_size_t),
                ("filter_y", ctypes.c_int32), ("filter_uv", ctypes.c_int32),
                ("lf_level", ctypes.c_void_p), ("b4_stride", ctypes.c_int32),
                ("lf_masks", ctypes.c_void_p), ("sb128w", ctypes.c_int32), ("sb128h", ctypes.c_int32),
                ("lim_e", ctypes.c_uint8 * 64), ("lim_i", ctypes.c_uint8 * 64),
                ("cdef_on", ctypes.c_int32), ("cdef_damping", ctypes.c_int32),
                ("cdef_y", ctypes.c_uint8 * 8), ("cdef_uv", ctypes.c_uint8 * 8),
                ("lr_mask", ctypes.c_void_p), ("lr_sb128w", ctypes.c_int32), ("restore_planes", ctypes.c_int32),
                ("lr_unit_size", ctypes.c_int32 * 2),
                ("mc", ctypes.c_void_p), ("n_mc", ctypes.c_int32),
                ("obmc_h", ctypes.c_void_p), ("n_obmc_h", ctypes.c_int32),
                ("obmc_v", ctypes.c_void_p), ("n_obmc_v", ctypes.c_int32),
                ("warp", ctypes.c_void_p), ("n_warp", ctypes.c_int32),
                ("scaled", ctypes.c_void_p), ("n_scaled", ctypes.c_int32),
                ("combine_y", ctypes.c_void_p), ("n_combine_y", ctypes.c_int32),
                ("combine_uv", ctypes.c_void_p), ("n_combine_uv", ctypes.c_int32),
                ("masks", ctypes.c_void_p), ("nmasks", ctypes.c_size_t),
                ("ntmp", ctypes.c_size_t),
                ("q_intra", ctypes.c_void_p), ("q_intra_tx", ctypes.c_void_p), ("q_dep_start", ctypes.c_void_p),
                ("q_deps", ctypes.c_void_p), ("q_n_deps", ctypes.c_int32), ("q_strip_start", ctypes.c_void_p),
                ("q_nstrips", ctypes.c_int32), ("q_granules", ctypes.c_int32)]


class MiColorInfo(ctypes.Structure):
    """include/mi_av1out.h: the sequence header's colour description (Dav1dColorPrimaries,
    Dav1dTransferCharacteristics, Dav1dMatrixCoefficients, color_range, Dav1dChromaSamplePosition)."""
    _fields_ = [("pri", ctypes.c_int32), ("trc", ctypes.c_int32), ("mtrx", ctypes.c_int32),
                ("range", ctypes.c_int32), ("chr", ctypes.c_int32)]

    def astuple(self):
        return (self.pri, self.trc, self.mtrx, self.range, self.chr)


class MiSeqInfo(ctypes.Structure):
    """include/mi_av1dec.h: what mi_dec_parse_sequence_header reads from a sequence header."""
    _fields_ = [("profile", ctypes.c_int32), ("max_w", ctypes.c_int32), ("max_h", ctypes.c_int32),
                ("bpc", ctypes.c_int32), ("layout", ctypes.c_int32), ("film_grain_present", ctypes.c_int32),
                ("color", MiColorInfo)]


class MiContentLight(ctypes.Structure):
    """include/mi_av1dec.h: the HDR CLL metadata OBU (Rav1dContentLightLevel), nits."""
    _fields_ = [("present", ctypes.c_int32), ("max_cll", ctypes.c_uint16), ("max_fall", ctypes.c_uint16)]


class MiMasteringDisplay(ctypes.Structure):
    """include/mi_av1dec.h: the HDR MDCV metadata OBU (Rav1dMasteringDisplay): chromaticities in
    0.16 fixed point, max_luminance in 24.8, min_luminance in 18.14."""
    _fields_ = [("present", ctypes.c_int32), ("primaries", (ctypes.c_uint16 * 2) * 3),
                ("white_point", ctypes.c_uint16 * 2),
                ("max_luminance", ctypes.c_uint32), ("min_luminance", ctypes.c_uint32)]


class MiItutT35(ctypes.Structure):
    """include/mi_av1dec.h: an ITU-T T.35 metadata OBU (Rav1dITUTT35); payload is valid until the
    next event (MiDecEvent.t35_payload is the copy)."""
    _fields_ = [("payload", ctypes.c_void_p), ("size", ctypes.c_int32),
                ("country_code", ctypes.c_uint8), ("country_code_ext", ctypes.c_uint8)]


class MiDecMetadata(ctypes.Structure):
    """include/mi_av1dec.h: what mi_dec_event_metadata reports for an event."""
    _fields_ = [("content_light", MiContentLight), ("mastering_display", MiMasteringDisplay),
                ("itut_t35", MiItutT35)]


class MiDecEvent(ctypes.Structure):
    _fields_ = [("frame", ctypes.POINTER(MiDecFrame)), ("pic_id", ctypes.c_int32),
                ("ref_pic", ctypes.c_int32 * 7), ("show_pic", ctypes.c_int32),
                ("fg_present", ctypes.c_int32), ("fg", MiFilmGrainData),
                ("release", ctypes.POINTER(ctypes.c_int32)), ("n_release", ctypes.c_int32),
                ("mtrx_identity", ctypes.c_int32),
                ("temporal_id", ctypes.c_int32), ("spatial_id", ctypes.c_int32),
                ("new_temporal_unit", ctypes.c_int32), ("color", MiColorInfo)]
    # The struct is the header's (ABI 4). Av1Decoder.events() adds, per event, what
    # mi_dec_event_metadata reports for it, as plain attributes: content_light (MiContentLight),
    # mastering_display (MiMasteringDisplay), itut_t35 (MiItutT35) and t35_payload, the T.35
    # message as bytes (a copy). None on an event that did not come from a decoder.
    content_light = mastering_display = itut_t35 = t35_payload = None


def build_dec():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "host")], check=True)


def dec_lib():
    global _dec
    if _dec is None:
        if not os.path.exists(DEC_PATH):
            raise RuntimeError(f"{DEC_PATH} missing: build it with `make -C rav1d_amd/host`")
        d = ctypes.CDLL(DEC_PATH)
        d.mi_dec_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        d.mi_dec_destroy.argtypes = [ctypes.c_void_p]
        d.mi_dec_destroy.restype = None
        d.mi_dec_send.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        d.mi_dec_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(MiDecEvent)]
        d.mi_dec_event_metadata.argtypes = [ctypes.c_void_p, ctypes.POINTER(MiDecMetadata)]
        d.mi_dec_set_threads.argtypes = [ctypes.c_void_p, ctypes.c_int]
        d.mi_dec_set_inloop_filters.argtypes = [ctypes.c_void_p, ctypes.c_int]
        d.mi_dec_set_operating_point.argtypes = [ctypes.c_void_p, ctypes.c_int]
        d.mi_dec_set_all_layers.argtypes = [ctypes.c_void_p, ctypes.c_int]
        d.mi_dec_set_decode_frame_type.argtypes = [ctypes.c_void_p, ctypes.c_int]
        d.mi_dec_set_frame_size_limit.argtypes = [ctypes.c_void_p, ctypes.c_uint]
        d.mi_dec_drain.argtypes = [ctypes.c_void_p]
        d.mi_dec_error.argtypes = [ctypes.c_void_p]
        d.mi_dec_error.restype = ctypes.c_char_p
        d.mi_dec_parse_sequence_header.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(MiSeqInfo)]
        _dec = d
    return _dec


def ivf_frames(path_or_bytes):
    """Yield the frame payloads of an IVF file (32-byte header, then 12-byte frame headers:
    u32 size, u64 timestamp; tools/input/ivf.rs:224)."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if data[:4] != b"DKIF":
        raise ValueError("not an IVF file")
    hdr_len = struct.unpack_from("<H", data, 6)[0]
    off = hdr_len
    while off + 12 <= len(data):
        size = struct.unpack_from("<I", data, off)[0]
        off += 12
        if off + size > len(data):
            break
        yield bytes(data[off:off + size])
        off += size


def _leb128(data, off):
    v, n = 0, 0
    while True:
        if off + n >= len(data) or n >= 8:
            raise ValueError("truncated leb128")
        b = data[off + n]
        v |= (b & 0x7f) << (7 * n)
        n += 1
        if not b & 0x80:
            return v, n


def _obu_type(b):
    return (b >> 3) & 0xf


def _is_annexb(data):
    """annexb_probe (tools/input/annexb.rs; C tools/input/annexb.c): temporal unit, frame unit and
    OBU sizes nest, and the first OBU is an empty temporal delimiter."""
    try:
        tu, n0 = _leb128(data, 0)
        fu, n1 = _leb128(data, n0)
        ou, n2 = _leb128(data, n0 + n1)
    except ValueError:
        return False
    o = n0 + n1 + n2
    if fu + n1 > tu or ou + n2 >= fu or o >= len(data):
        return False
    return _obu_type(data[o]) == 2


def annexb_units(data):
    """Annex B demuxer (tools/input/annexb.rs): temporal_unit(size) > frame_unit(size) >
    obu_length + OBU; yields one OBU at a time, as the reference hands each to the decoder."""
    off = 0
    while off < len(data):
        tu, n = _leb128(data, off)
        off += n
        end_tu = off + tu
        while off < end_tu:
            fu, n = _leb128(data, off)
            off += n
            end_fu = off + fu
            while off < end_fu:
                ln, n = _leb128(data, off)
                off += n
                yield bytes(data[off:off + ln])
                off += ln


def section5_units(data):
    """Low-overhead OBU stream (section 5; tools/input/section5.rs): temporal units split at
    temporal delimiters, every OBU carrying its size field."""
    off, start = 0, 0
    while off < len(data):
        h = data[off]
        if not h & 0x2:
            raise ValueError("section 5 OBU without a size field")
        if _obu_type(h) == 2 and off > start:
            yield bytes(data[start:off])
            start = off
        ext = 1 if h & 0x4 else 0
        ln, n = _leb128(data, off + 1 + ext)
        off += 1 + ext + n + ln
    if off > start:
        yield bytes(data[start:off])


def stream_units(data):
    """The decoder inputs of a file in any of the reference CLI's demuxer formats (IVF, Annex B,
    section 5; tools/input/input.rs probes them in that order)."""
    if data[:4] == b"DKIF":
        return ivf_frames(data)
    if _is_annexb(data):
        return annexb_units(data)
    return section5_units(data)


# Dav1dSettings.inloop_filters bits (include/dav1d/dav1d.rs:28-35; include/mi_av1dec.h)
INLOOPFILTER_NONE, INLOOPFILTER_DEBLOCK, INLOOPFILTER_CDEF, INLOOPFILTER_RESTORATION = 0, 2, 4, 8
INLOOPFILTER_ALL = INLOOPFILTER_DEBLOCK | INLOOPFILTER_CDEF | INLOOPFILTER_RESTORATION
# the CLI's --inloopfilters values (inloop_filters_tbl, tools/dav1d_cli_parse.rs:479-530)
INLOOPFILTER_NAMES = {"none": 0, "deblock": 2, "nodeblock": 12, "cdef": 4, "nocdef": 10,
                      "restoration": 8, "norestoration": 6, "all": 14}
# Dav1dSettings.decode_frame_type (include/dav1d/dav1d.rs:50-70) under the CLI's
# --decodeframetype names
DECODEFRAMETYPE_NAMES = {"all": 0, "reference": 1, "intra": 2, "key": 3}


class DecoderError(RuntimeError):
    """A negative return of the front-end; code is the -errno."""

    def __init__(self, what, code, why=""):
        super().__init__(f"{what}: {code} ({why})")
        self.code = code


class Av1Decoder:
    """One stream. send() one temporal unit, then drain events(); drain() after the last."""

    def __init__(self, threads=1, inloop_filters=INLOOPFILTER_ALL, operating_point=0, all_layers=True,
                 decode_frame_type="all", frame_size_limit=0):
        """threads > 1: intra frames are decoded on that many worker threads (mi_dec_set_threads);
        send a few temporal units ahead of draining events() to overlap them. inloop_filters:
        Dav1dSettings.inloop_filters (an int of INLOOPFILTER_* bits or a CLI name).
        operating_point, all_layers, decode_frame_type (an int or a DECODEFRAMETYPE_NAMES key) and
        frame_size_limit: the Dav1dSettings fields of those names (include/mi_av1dec.h); a value
        the front-end rejects raises ValueError."""
        self.lib = dec_lib()
        self.h = ctypes.c_void_p()
        r = self.lib.mi_dec_create(ctypes.byref(self.h))
        if r:
            raise RuntimeError(f"mi_dec_create: {r}")
        if threads > 1:
            self.lib.mi_dec_set_threads(self.h, threads)
        if isinstance(inloop_filters, str):
            inloop_filters = INLOOPFILTER_NAMES[inloop_filters]
        if inloop_filters != INLOOPFILTER_ALL:
            r = self.lib.mi_dec_set_inloop_filters(self.h, int(inloop_filters))
            if r:
                raise ValueError(f"mi_dec_set_inloop_filters({inloop_filters}): {r}")
        if isinstance(decode_frame_type, str):
            if decode_frame_type not in DECODEFRAMETYPE_NAMES:
                raise ValueError(f"decode_frame_type {decode_frame_type!r}")
            decode_frame_type = DECODEFRAMETYPE_NAMES[decode_frame_type]
        for name, v, default in (("operating_point", int(operating_point), 0),
                                 ("all_layers", int(bool(all_layers)), 1),
                                 ("decode_frame_type", int(decode_frame_type), 0),
                                 ("frame_size_limit", int(frame_size_limit), 0)):
            if v == default:
                continue
            if name == "frame_size_limit" and not 0 <= v < 1 << 32:
                raise ValueError(f"frame_size_limit {v}")
            r = getattr(self.lib, "mi_dec_set_" + name)(self.h, v)
            if r:
                raise ValueError(f"mi_dec_set_{name}({v}): {r}")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.mi_dec_destroy(self.h)
            self.h = None

    def error(self):
        return self.lib.mi_dec_error(self.h).decode()

    @staticmethod
    def parse_sequence_header(data):
        """mi_dec_parse_sequence_header (dav1d_parse_sequence_header, src/lib.rs): the MiSeqInfo of
        the first sequence header among the OBUs of `data`, without decoding. Raises DecoderError
        with code -ENOENT when there is none, -EINVAL when it is malformed."""
        out = MiSeqInfo()
        data = bytes(data)
        r = dec_lib().mi_dec_parse_sequence_header(data, len(data), ctypes.byref(out))
        if r < 0:
            raise DecoderError("mi_dec_parse_sequence_header", r, os.strerror(-r))
        return out

    def send(self, data):
        r = self.lib.mi_dec_send(self.h, data, len(data))
        if r < 0:
            raise DecoderError("mi_dec_send", r, self.error())

    def drain(self):
        """The end of the input (mi_dec_drain): the picture all_layers=False holds back becomes
        a last event. A no-op otherwise."""
        r = self.lib.mi_dec_drain(self.h)
        if r < 0:
            raise DecoderError("mi_dec_drain", r, self.error())

    def events(self):
        """Yield MiDecEvent structs; each is valid only until the next one is requested. Every event
        carries its HDR metadata (mi_dec_event_metadata) as the attributes content_light,
        mastering_display and itut_t35, and t35_payload: the ITU-T T.35 message of the event's frame
        as bytes (a copy the caller may keep), or None."""
        ev = MiDecEvent()
        while True:
            r = self.lib.mi_dec_next(self.h, ctypes.byref(ev))
            if r < 0:
                raise DecoderError("mi_dec_next", r, self.error())
            if r == 0:
                return
            md = MiDecMetadata()
            r = self.lib.mi_dec_event_metadata(self.h, ctypes.byref(md))
            if r < 0:
                raise DecoderError("mi_dec_event_metadata", r, self.error())
            ev.content_light, ev.mastering_display, ev.itut_t35 = md.content_light, md.mastering_display, md.itut_t35
            t = md.itut_t35
            ev.t35_payload = ctypes.string_at(t.payload, t.size) if t.payload and t.size > 0 else None
            yield ev


def stream_events(data, threads=1, lookahead=None, inloop_filters=INLOOPFILTER_ALL, operating_point=0,
                  all_layers=True, decode_frame_type="all", frame_size_limit=0):
    """Decoder events of a stream (IVF, Annex B or section 5) in decode order. With threads > 1 the front-end keeps
    `lookahead` (default 2 * threads) temporal units ahead of the events handed out, so that
    frames decode on the worker threads while the caller consumes earlier ones. Each event is
    valid until the next one is requested. The other settings are Av1Decoder's; the decoder is
    drained after the last unit."""
    dec = Av1Decoder(threads, inloop_filters, operating_point, all_layers, decode_frame_type, frame_size_limit)
    la = 0 if threads <= 1 else (lookahead if lookahead is not None else 2 * threads)
    # (threads > 1 with lookahead 0: one temporal unit at a time, its frame's tiles in parallel)
    sent = 0
    for tu in stream_units(data):
        dec.send(tu)
        sent += 1
        if sent <= la:
            continue
        gen = dec.events()
        if la:
            ev = next(gen, None)     # one event per temporal unit sent: the queue stays `la` deep
            if ev is not None:
                yield ev
        else:
            yield from gen
    dec.drain()
    yield from dec.events()
