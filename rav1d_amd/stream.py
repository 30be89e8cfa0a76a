"""Stream decode on the device: the front-end's per-frame work lists (rav1d_amd/libmi_av1dec.so,
include/mi_av1dec.h) executed by librav1d_amd.so's frame executor (mi_frame_run / mi_frame_end).

This is the host loop rav1d runs in decode.rs:4526-4550 (decode_tile_sbrow, then filter_sbrow)
with the pixel work moved to the GPU: for every decoder event, the frame's reconstruction and
in-loop filters are enqueued on one stream into device pictures; shown pictures are handed to
the caller (on the device). There is no CPU pixel path here.
"""
import ctypes

from . import MiFramePictures, MiFrameTiming, check, lib
from . import frame as F
from .av1dec import MiColorInfo, stream_events


class DevicePictureSet:
    """The four pictures one frame's pass 2 writes (recon, deblocked, cdef, restored)."""

    def __init__(self, w, h, bpc, layout):
        self.frames = [F.Frame(w, h, bpc, layout) for _ in range(4)]
        self.pics = MiFramePictures()
        for i, fr in enumerate(self.frames):
            self.pics.pics[i] = fr.picture()
        self.final = 0

    def output(self):
        return self.frames[self.final]


def run_frame(ctx, fr, stream=None, refs=None):
    """Enqueue one MiDecFrame on the device; returns its DevicePictureSet (output() = the
    reference-quality picture once the stream reaches it). refs: the frame's seven reference
    pictures (Frame or None, in MiDecEvent.ref_pic order) for an inter frame."""
    ps = DevicePictureSet(fr.up_w, fr.h, fr.bpc, fr.layout)   # upscaled geometry with super-resolution
    for i, r in enumerate(refs or []):
        if r is not None:
            ps.pics.refs[i] = r.picture()
    ps.refs = [r for r in (refs or []) if r is not None]       # keep the reference tensors alive
    final = ctypes.c_int(-1)
    check(lib().mi_frame_run(ctx.h, ctypes.byref(fr), ctypes.byref(ps.pics), ctypes.byref(final),
                             F._stream_ptr(stream)), "mi_frame_run")
    ps.final = final.value
    return ps


def frame_end(ctx, stream=None):
    check(lib().mi_frame_end(ctx.h, F._stream_ptr(stream)), "mi_frame_end")


def _refs(pics, ev, key=lambda p: p):
    """The reference pictures (final Frames) of an event's frame, in ref_pic order."""
    out = []
    for r in ev.ref_pic:
        out.append(key(pics[r]).output() if r >= 0 and r in pics else None)
    return out


def decode_ivf(ctx, data, stream=None, sync_each=True, inloop_filters=14, threads=1, operating_point=0,
               all_layers=True, decode_frame_type="all", frame_size_limit=0):
    """Decode a stream (IVF, Annex B or section 5) on the device; yields the shown pictures (Frame, device planes) in
    output order. With sync_each, every frame is checked with mi_frame_end before it is shown.
    inloop_filters: Dav1dSettings.inloop_filters (rav1d_amd.av1dec.INLOOPFILTER_*). threads > 1: the
    front-end's frame and tile threads (mi_dec_set_threads). operating_point, all_layers,
    decode_frame_type, frame_size_limit: the Dav1dSettings fields of those names
    (rav1d_amd.av1dec.Av1Decoder). A picture the front-end holds back (all_layers=False) stays in
    `pics` until the event that shows or drops it: the front-end lists it in no release[] before."""
    for _, frame in shown_pictures(ctx, data, stream, sync_each, threads=threads, inloop_filters=inloop_filters,
                                   operating_point=operating_point, all_layers=all_layers,
                                   decode_frame_type=decode_frame_type, frame_size_limit=frame_size_limit):
        yield frame


def shown_pictures(ctx, data, stream=None, sync_each=True, **settings):
    """The decode loop of the generators of this module: every frame of the stream enqueued on
    the device, and per shown picture, in output order, (ev, frame): the MiDecEvent that shows it
    (valid until the generator is resumed) and the device Frame. With sync_each every frame is
    checked with mi_frame_end before anything of it is shown; one mi_frame_end follows the last
    event. The pictures an event releases are dropped when the consumer resumes the generator: it
    has taken the shown one by then. settings: stream_events's (threads and the Dav1dSettings
    fields); the front-end is never more than the current temporal unit ahead."""
    pics = {}
    for ev in stream_events(data, lookahead=0, **settings):
        if ev.frame:
            pics[ev.pic_id] = run_frame(ctx, ev.frame.contents, stream, _refs(pics, ev))
            if sync_each:
                frame_end(ctx, stream)
        if ev.show_pic >= 0:
            yield ev, pics[ev.show_pic].output()
        for i in range(ev.n_release):
            pics.pop(ev.release[i], None)
    frame_end(ctx, stream)


def _grain(ev, apply_grain):
    """The film grain parameters a shown picture is output with, or None."""
    return ev.fg if (ev.fg_present and apply_grain) else None


def _shown_colour(ev, src, matrix, tonemap, primaries, transfer, rgb):
    """The MiColorInfo a shown picture is converted with (decode_to_tensors's rules): a copy of the
    event's; for an RGB output with the matrix override, or the size's default when the stream
    leaves mtrx unspecified; then with the primaries / transfer overrides."""
    color = MiColorInfo(*ev.color.astuple())
    if rgb:
        if matrix is not None:
            color.mtrx = int(matrix)
        elif color.mtrx == 2:
            color.mtrx = 1 if (src.w >= 1280 or src.h > 576) else 6
    _source_colour(color, tonemap, primaries, transfer)
    return color


def _source_colour(color, tonemap, primaries, transfer):
    """Apply the primaries / transfer overrides to `color`; with a tone map the source must be
    described: nothing is guessed."""
    if primaries is not None:
        color.pri = int(primaries)
    if transfer is not None:
        color.trc = int(transfer)
    if tonemap is not None and (color.pri == 2 or color.trc == 2):
        raise ValueError(f"tonemap needs the source's primaries and transfer: the stream has pri {color.pri}, "
                         f"trc {color.trc} (2: unspecified); pass primaries= / transfer=")


class PeakTracker:
    """The smoothing of peak="measured": per picture, update(m) takes the measured light level m
    (nits) and returns the src_peak to map that picture with. The state s follows m at once
    upwards and by a sixteenth of the distance downwards (s = m if m >= s else s + (m - s) / 16,
    in float64; the first m sets it), the result is s raised to a multiple of 100 nits and clamped
    to [max(100, dst_peak), 10000]. The quantum keeps the result, and so the device tables, the
    same from picture to picture within a scene. No GPU is involved."""

    QUANTUM, RELEASE = 100.0, 16.0

    def __init__(self, dst_peak=100.0):
        self.lo = max(100.0, float(dst_peak))
        self.s = None

    def update(self, m):
        import math
        m = float(m)
        self.s = m if self.s is None or m >= self.s else self.s + (m - self.s) / self.RELEASE
        q = math.ceil(self.s / self.QUANTUM) * self.QUANTUM
        return min(max(q, self.lo), 10000.0)


def metadata_peak(ev, tonemap):
    """The src_peak peak="metadata" takes from a decoder event: the mastering display's
    max_luminance / 256 (24.8 fixed point) when the event has one with max_luminance > 0, else
    max_cll when content light is present and > 0, else the tone map's own src_peak. Not clamped
    (_with_peak does that)."""
    md, cl = ev.mastering_display, ev.content_light      # (None: an event without metadata attached)
    if md is not None and md.present and md.max_luminance > 0:
        return md.max_luminance / 256.0
    if cl is not None and cl.present and cl.max_cll > 0:
        return float(cl.max_cll)
    return float(tonemap.src_peak)


PEAK_MODES = (None, "metadata", "measured")


def _check_peak(peak, tonemap):
    if peak not in PEAK_MODES:
        raise ValueError(f"peak {peak!r}: want None, 'metadata' or 'measured'")
    if peak is not None and tonemap is None:
        raise ValueError("peak needs a tonemap: it chooses the tone map's src_peak")


def _with_peak(tonemap, nits):
    """A copy of `tonemap` with src_peak = nits clamped to [dst_peak, 10000] (the stage wants
    peaks in [1, 10000]; a source peak below the target's has nothing to compress)."""
    from .display import MiToneMap
    lo = max(1.0, float(tonemap.dst_peak))
    return MiToneMap(tonemap.dst_pri, tonemap.dst_trc, tonemap.dst_bpc, min(max(float(nits), lo), 10000.0),
                     tonemap.dst_peak)


def _picture_tonemap(ctx, ev, src, color, tonemap, peak, tracker, stream):
    """The tone map a shown picture's output call gets: `tonemap` itself for peak=None, else a copy
    whose src_peak comes from the event's metadata or from the picture (light_level, then
    light_stats: a synchronisation per picture, the stated cost of "measured")."""
    if peak is None:
        return tonemap
    if color.trc != 16:
        raise ValueError(f"peak={peak!r} needs a PQ source (trc 16): the picture has trc {color.trc}")
    if peak == "metadata":
        return _with_peak(tonemap, metadata_peak(ev, tonemap))
    from .display import light_level, light_stats
    return _with_peak(tonemap, tracker.update(light_stats(light_level(ctx, src, color, stream), src.bpc, 99.99).pct_nits))


def decode_to_tensors(ctx, data, format="nv12", apply_grain=True, matrix=None, stream=None, inloop_filters=14,
                      threads=1, operating_point=0, all_layers=True, decode_frame_type="all", frame_size_limit=0,
                      tonemap=None, primaries=None, transfer=None, peak=None):
    """Decode a stream (IVF, Annex B or section 5) on the device and yield, per shown picture in
    output order, (DisplayImage, MiColorInfo): the picture as a tight device tensor in `format`
    ("nv12": semi-planar at the stream's own subsampling and bit depth; "rgb": planar R'G'B';
    "rgba": packed with alpha; rav1d_amd.display.DisplayImage) through mi_display_picture, with
    film grain when the frame carries it and apply_grain is set, and the colour description of
    its sequence header. Every image is a fresh allocation the caller owns; its frame has been
    checked with mi_frame_end before the conversion is enqueued, and the conversion has been
    enqueued on `stream` (synchronise it, or stay on it, before reading).

    matrix: the Dav1dMatrixCoefficients value the RGB formats convert with; an explicit value
    overrides the stream's. With matrix=None the stream's own mtrx is used, and a stream that
    leaves it unspecified (mtrx 2) gets BT.709 (1) when w >= 1280 or h > 576 and BT.601 (6)
    otherwise, the usual rule for untagged video. The MiColorInfo yielded carries the matrix that
    was used.

    tonemap: a rav1d_amd.display.ToneMap(): the RGB formats go through mi_display_picture_tm and
    the image holds samples of tonemap.dst_bpc bits in the tone map's primaries and transfer.
    primaries, transfer: Dav1dColorPrimaries / Dav1dTransferCharacteristics values that override
    the stream's (as matrix does; the MiColorInfo yielded carries them). With tonemap, a stream
    that leaves either unspecified and has no override raises ValueError. An HLG source (trc 18,
    the stream's or transfer=18) is taken only by a context the caller has opted in with
    rav1d_amd.display.enable_hlg(ctx): the helpers of this module never switch it on themselves, and
    on any other context the call raises MiError (ENOTSUP), as it always did. tonemap.dst_peak is
    then the peak of the display the picture is rendered for, and src_peak is not read.

    peak: where a PQ source's src_peak comes from (read with tonemap only, and for a source whose
    trc after the overrides is 16: a ValueError otherwise when it is not None, HLG included, which
    reads no src_peak for the modes to choose). None: the tone
    map's own. "metadata": per shown picture, the stream's mastering display or content light
    (metadata_peak). "measured": per shown picture, the 99.99th percentile of max(R', G', B') of
    the picture itself (rav1d_amd.display.light_level, without grain) through a PeakTracker; this
    synchronises once per picture. Either value is clamped to [dst_peak, 10000] and goes to the
    call in a copy of `tonemap`. The other settings are decode_ivf's."""
    from .display import FORMATS, OUT_SEMIPLANAR, DisplayImage, display_picture
    fmt = FORMATS[format] if isinstance(format, str) else int(format)
    _check_peak(peak, tonemap)
    tracker = PeakTracker(tonemap.dst_peak) if peak == "measured" else None
    for ev, src in shown_pictures(ctx, data, stream, threads=threads, inloop_filters=inloop_filters,
                                  operating_point=operating_point, all_layers=all_layers,
                                  decode_frame_type=decode_frame_type, frame_size_limit=frame_size_limit):
        color = _shown_colour(ev, src, matrix, tonemap, primaries, transfer, rgb=fmt != OUT_SEMIPLANAR)
        image = DisplayImage(src.w, src.h, src.bpc, src.layout, fmt,
                             out_bpc=tonemap.dst_bpc if tonemap is not None else None)
        tm = _picture_tonemap(ctx, ev, src, color, tonemap, peak, tracker, stream)
        display_picture(ctx, src, image, color, _grain(ev, apply_grain), stream, tm)
        yield image, color


def fit_crop(w, h, W, H, fit):
    """The crop (x, y, cw, ch) of a w x h picture for a W x H target: "stretch" takes the whole
    picture, "crop" the largest centred rectangle of the target's aspect."""
    if fit == "stretch":
        return 0, 0, w, h
    if fit != "crop":
        raise ValueError(f"fit {fit!r}")
    if w * H >= h * W:
        cw = max(1, (h * W) // H)
        return (w - cw) // 2, 0, cw, h
    ch = max(1, (w * H) // W)
    return 0, (h - ch) // 2, w, ch


def decode_to_batches(ctx, data, size, batch=8, dtype=None, channels_last=False, mean=None, std=None, fit="stretch",
                      every=1, apply_grain=True, matrix=None, stream=None, inloop_filters=14, threads=1,
                      operating_point=0, all_layers=True, decode_frame_type="all", frame_size_limit=0,
                      tonemap=None, primaries=None, transfer=None, resample=None, peak=None):
    """Decode a stream on the device and yield (tensor, [MiColorInfo, ...]) batches for an ML
    consumer: the tensor is (n, 3, H, W) with size = (W, H), n = batch except for a shorter last
    one, of `dtype` (torch.float16 by default; bfloat16, float32 or uint8), contiguous or, with
    channels_last, in torch.channels_last memory format. Every `every`-th shown picture (the
    first, then each every-th after it) goes through mi_display_tensor (rav1d_amd.display
    .display_tensor) into its slot: cropped per `fit` (fit_crop; pictures of different sizes in a
    stream each get their own crop), resized, normalised with mean / std per channel, with film
    grain when the frame carries it and apply_grain is set. The list holds the colour description
    used for each slot; matrix, tonemap, primaries and transfer follow decode_to_tensors's rules
    (with tonemap the slot is mi_display_tensor_tm's: the tone-mapped picture, resized; an HLG
    source needs a context the caller has opted in with rav1d_amd.display.enable_hlg). resample: a
    MiResample (rav1d_amd.display.Resample, "catmull_rom" for models trained on bicubic-resized
    inputs): the filter of the resize, None the triangle. peak: decode_to_tensors's, per picture that
    is output (a skipped picture is not measured). Each tensor is a fresh allocation
    the caller owns, filled by work enqueued on `stream` (synchronise it, or stay on it, before
    reading). The other settings are decode_ivf's."""
    import torch

    from .display import display_tensor
    W, H = (int(v) for v in size)
    if batch < 1 or every < 1:
        raise ValueError("batch and every must be at least 1")
    fit_crop(1, 1, W, H, fit)      # (an unknown fit fails before any decoding)
    dtype = torch.float16 if dtype is None else dtype
    _check_peak(peak, tonemap)
    tracker = PeakTracker(tonemap.dst_peak) if peak == "measured" else None
    tensor, colors = None, []
    shown = enumerate(shown_pictures(ctx, data, stream, threads=threads, inloop_filters=inloop_filters,
                                     operating_point=operating_point, all_layers=all_layers,
                                     decode_frame_type=decode_frame_type, frame_size_limit=frame_size_limit))
    for k, (ev, src) in shown:
        if k % every:
            continue
        color = _shown_colour(ev, src, matrix, tonemap, primaries, transfer, rgb=True)
        if tensor is None:
            fmt = torch.channels_last if channels_last else torch.contiguous_format
            tensor, colors = torch.empty((batch, 3, H, W), dtype=dtype, device="cuda", memory_format=fmt), []
        tm = _picture_tonemap(ctx, ev, src, color, tonemap, peak, tracker, stream)
        display_tensor(ctx, src, tensor[len(colors)], color, _grain(ev, apply_grain),
                       fit_crop(src.w, src.h, W, H, fit), mean, std, stream, tonemap=tm, resample=resample)
        colors.append(color)
        if len(colors) == batch:
            yield tensor, colors
            tensor = None
    if tensor is not None:
        yield tensor[:len(colors)], colors


def decode_to_ladder(ctx, data, sizes, bpc=None, fit="stretch", apply_grain=True, stream=None, inloop_filters=14,
                     threads=1, operating_point=0, all_layers=True, decode_frame_type="all", frame_size_limit=0,
                     resample=None, tonemap=None, target=None, primaries=None, transfer=None, matrix=None, peak=None):
    """Decode a stream on the device and yield, per shown picture in output order, (event, rungs):
    the decoder event that showed it and a list with one (Y, UV) pair of device tensors per entry
    of `sizes` ((W, H) luma sizes), the picture as semi-planar YUV at the stream's own subsampling
    through one mi_display_scaled call (rav1d_amd.display.display_scaled): Y is (H, W), UV is
    (ch, cw, 2), None for 4:0:0. bpc: the depth of every rung (8, 10 or 12; None keeps the
    stream's); uint8 at 8 bits, else 16-bit words MSB-aligned in int16 storage. fit: fit_crop's,
    per size, moved onto the chroma grid (rav1d_amd.display.even_crop); pictures of different sizes
    in a stream each get their own crops. Film grain is applied once per picture when the frame
    carries it and apply_grain is set; the chroma siting is the sequence header's. resample: a
    MiResample (rav1d_amd.display.Resample, "mitchell" for instance) for every rung and plane, None
    the triangle. tonemap: a rav1d_amd.display.ToneMap(): the call is mi_display_scaled_tm, every rung
    is resized from the tone-mapped picture as Y'CbCr in `target` (a rav1d_amd.display.YuvTarget();
    None: BT.709, limited range), and bpc=None means tonemap.dst_bpc
    (rav1d_amd.display.output_colour gives the tags of the rungs). primaries, transfer, matrix: the
    overrides of decode_to_tensors, by its rules: with tonemap, a stream that leaves primaries or
    transfer unspecified and has no override raises ValueError before any device work of the
    picture, and an HLG source (trc 18) needs a context the caller has opted in with
    rav1d_amd.display.enable_hlg (this helper never does; peak stays a ValueError for it). Without tonemap the overrides are not read and nothing changes (a target on its own is a
    ValueError: there is no matrix or range conversion without a tone map). peak: decode_to_tensors's:
    where a PQ source's src_peak comes from, per shown picture. Every tensor is
    a fresh allocation the caller owns, filled by work enqueued on `stream` (synchronise it, or
    stay on it, before reading). The other settings are decode_ivf's."""
    from .display import ScaledImage, display_scaled, even_crop
    sizes = [(int(W), int(H)) for W, H in sizes]
    if not 1 <= len(sizes) <= 8:
        raise ValueError("1 to 8 sizes")
    for W, H in sizes:
        fit_crop(1, 1, W, H, fit)      # (an unknown fit fails before any decoding)
    _check_peak(peak, tonemap)
    tracker = PeakTracker(tonemap.dst_peak) if peak == "measured" else None
    for ev, src in shown_pictures(ctx, data, stream, threads=threads, inloop_filters=inloop_filters,
                                  operating_point=operating_point, all_layers=all_layers,
                                  decode_frame_type=decode_frame_type, frame_size_limit=frame_size_limit):
        if tonemap is None:
            color, depth = MiColorInfo(*ev.color.astuple()), src.bpc
        else:
            color, depth = _shown_colour(ev, src, matrix, tonemap, primaries, transfer, rgb=True), tonemap.dst_bpc
        images = [ScaledImage(W, H, depth if bpc is None else bpc, src.layout,
                              even_crop(fit_crop(src.w, src.h, W, H, fit), src.w, src.h, src.layout))
                  for W, H in sizes]
        tm = _picture_tonemap(ctx, ev, src, color, tonemap, peak, tracker, stream)
        display_scaled(ctx, src, images, color, _grain(ev, apply_grain), stream, resample=resample, tonemap=tm,
                       target=target)
        yield ev, [im.tensors() for im in images]


_extra_lanes = {}


def _lanes(ctx, stream, n):
    """n (context, stream) pairs for frames in flight: the caller's first, then cached extra
    contexts with their own streams (a context's calls stay on one stream)."""
    import torch
    lanes = [(ctx, stream)]
    key = id(ctx)
    extra = _extra_lanes.setdefault(key, [])
    while len(extra) < n - 1:
        from .frame import Context
        extra.append((Context(torch.cuda.current_device()), torch.cuda.Stream()))
    return lanes + extra[:n - 1]


def _lane_timing(lanes):
    """The mi_ctx_timing figures of every lane's context summed under decode_to_muxer's stats
    keys; switches the contexts' timing off again."""
    tot = dict(frames=0, run_host_ms=0.0, upload_ms=0.0, inter_ms=0.0, intra_ms=0.0, filter_ms=0.0,
               upload_bytes=0, run_stage_ms=0.0, run_levels_ms=0.0)
    for lctx, _ in lanes:
        tm = MiFrameTiming()
        check(lib().mi_ctx_timing(lctx.h, ctypes.byref(tm)), "mi_ctx_timing")
        check(lib().mi_ctx_set_timing(lctx.h, 0), "mi_ctx_set_timing")
        tot["frames"] += tm.frames
        tot["run_host_ms"] += tm.host_ms
        tot["run_stage_ms"] += tm.stage_ms
        tot["run_levels_ms"] += tm.strips_ms
        for f in ("upload_ms", "inter_ms", "intra_ms", "filter_ms", "upload_bytes"):
            tot[f] += getattr(tm, f)
    return tot


def decode_to_muxer(ctx, data, muxer, stream=None, apply_grain=True, pipelined=True, threads=8, in_flight=2,
                    inloop_filters=14, stats=None, operating_point=0, all_layers=True, decode_frame_type="all",
                    frame_size_limit=0):
    """Decode an IVF stream on the device and write every shown picture through `muxer`
    (rav1d_amd.output.Muxer): the picture leaves HBM once, via mi_output_picture into pinned
    host memory, with film grain applied in that same pass when the frame carries grain and
    apply_grain is set (Dav1dSettings.apply_grain, src/lib.rs). Returns the pictures written.

    pipelined: rav1d's frame threading on this path (src/thread_task.rs):
      * the host front-end decodes frames on `threads` worker threads (each frame's tiles on
        their own threads too), a few temporal units ahead of the device (mi_dec_set_threads);
      * frames are reconstructed `in_flight` at a time, frame k on (context, stream) k % in_flight;
        a frame whose prediction reads other pictures waits for their events first (allintra:
        80 -> 49 ms with 2 lanes; inter streams whose front-end is the bound: unchanged);
      * a shown picture goes to the muxer once its output copy has landed (an event, not a
        stream sync), one picture behind; host pictures rotate.
    Device failures of any frame are reported by the mi_frame_end calls at the end of the
    stream. Without pipelined: one frame at a time, each checked by mi_frame_end before it is
    shown, the front-end one temporal unit at a time (its tiles still on `threads` threads).

    operating_point, all_layers, decode_frame_type, frame_size_limit: the Dav1dSettings fields of
    those names (rav1d_amd.av1dec.Av1Decoder). A picture held back by all_layers=False is shown by
    a later event than its frame's: it is copied out on the lane that reconstructed it, and stays
    in the pools until that event (the front-end releases it no earlier).

    stats: a dict to receive the per-stage breakdown: host time waiting for the
    front-end's events (front_end_ms), host time inside mi_frame_run (run_host_ms), the device
    stages of every frame from mi_ctx_timing (upload_ms / inter_ms / intra_ms / filter_ms,
    upload_bytes), the output copies into host memory (d2h_ms, HIP events) and the muxer's host
    time (mux_ms)."""
    import time

    from .output import HostPicture, output_picture
    import torch
    if not pipelined:
        in_flight = 1
    lanes = _lanes(ctx, stream, max(1, in_flight))
    streams = [st if st is not None else torch.cuda.current_stream() for _, st in lanes]
    if len(lanes) > 1:
        for st in streams[1:]:
            st.wait_stream(streams[0])
    pics, done_ev, n = {}, {}, 0
    hosts = [None] * (len(lanes) + 1)
    pending = []                        # (slot, event) of pictures awaiting the muxer, in order
    k = 0
    clock = time.perf_counter
    acc = dict(front_end_ms=0.0, mux_ms=0.0, d2h_ms=0.0)
    out_ev = []
    if stats is not None:
        for lctx, _ in lanes:
            check(lib().mi_ctx_set_timing(lctx.h, 1), "mi_ctx_set_timing")

    def flush(keep):
        nonlocal n
        while len(pending) > keep:
            slot, ev = pending.pop(0)
            ev.synchronize()
            t = clock()
            muxer.write(hosts[slot].pic)
            acc["mux_ms"] += (clock() - t) * 1e3
            n += 1

    slot = 0
    # (without pipelined the front-end still decodes each frame's tiles on `threads` threads,
    # but no temporal unit ahead of the one the device is given)
    events = iter(stream_events(data, threads, lookahead=None if pipelined else 0, inloop_filters=inloop_filters,
                                operating_point=operating_point, all_layers=all_layers,
                                decode_frame_type=decode_frame_type, frame_size_limit=frame_size_limit))
    while True:
        t = clock()
        ev = next(events, None)
        acc["front_end_ms"] += (clock() - t) * 1e3
        if ev is None:
            break
        if ev.frame:
            li = k % len(lanes)
            k += 1
            lctx, lst = lanes[li]
            for r in ev.ref_pic:          # pictures this frame's prediction reads
                if r >= 0 and r in done_ev:
                    streams[li].wait_event(done_ev[r])
            # the pictures are allocated (and zero-filled) on the lane's own stream
            with torch.cuda.stream(streams[li]):
                ps = run_frame(lctx, ev.frame.contents, lst, _refs(pics, ev, key=lambda p: p[0]))
            pics[ev.pic_id] = (ps, li)
            e = torch.cuda.Event()
            e.record(streams[li])
            done_ev[ev.pic_id] = e
            if not pipelined:
                frame_end(lctx, lst)
        if ev.show_pic >= 0:
            ps, li = pics[ev.show_pic]
            out = ps.output()
            lctx, lst = lanes[li]
            if any(p[0] == slot for p in pending):
                flush(0)
            h = hosts[slot]
            if h is None or (h.pic.w, h.pic.h, h.pic.bpc, h.pic.layout) != (out.w, out.h, out.bpc, out.layout):
                hosts[slot] = h = HostPicture(out.w, out.h, out.bpc, out.layout)
            fg = _grain(ev, apply_grain)
            if stats is not None:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(streams[li])
            output_picture(lctx, out, h, fg, ev.mtrx_identity, lst)
            if stats is not None:
                b.record(streams[li])
                out_ev.append((a, b))
            done = torch.cuda.Event()
            done.record(streams[li])
            pending.append((slot, done))
            flush(len(lanes) if pipelined else 0)
            slot = (slot + 1) % len(hosts)
        for i in range(ev.n_release):
            pics.pop(ev.release[i], None)
            done_ev.pop(ev.release[i], None)
    flush(0)
    for lctx, lst in lanes:
        frame_end(lctx, lst)
    if stats is not None:
        tot = _lane_timing(lanes)
        acc["d2h_ms"] = sum(a.elapsed_time(b) for a, b in out_ev)
        stats.update(tot)
        stats.update(acc)
    return n
