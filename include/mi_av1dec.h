/*
 * mi_av1dec.h — C-ABI of the host front-end: AV1 OBUs in, pass-2 work lists out.
 *
 * This is the CPU side north_star keeps on the host (rav1d's OBU / msac / mode and
 * coefficient decoding: src/obu.rs:2662, src/msac.rs, src/decode.rs:1131-4067,
 * src/recon.rs:478-2023, src/lf_mask.rs:380-723), restated in C++ (rav1d_amd/host/) and built
 * as rav1d_amd/libmi_av1dec.so. Instead of reconstructing pixels it emits, per frame, the
 * descriptor lists of mi_av1dsp.h (MiIntraBlock / MiTxBlock, coefficient arena, Av1Filter
 * masks and levels, Av1Restoration units, film-grain data) that the gfx950 kernels execute.
 *
 * Threading: one MiDec per stream; calls on one MiDec are serialised by the caller.
 * Errors: 0 / positive counts, or a negative errno (-EINVAL bitstream error, -ENOMEM,
 * -ENOTSUP for a coding tool this front-end does not decode yet); mi_dec_error() explains.
 */
#ifndef MI_AV1DEC_H
#define MI_AV1DEC_H

#include <stddef.h>
#include <stdint.h>

#include "mi_av1dsp.h"
#include "mi_av1out.h"   /* MiColorInfo */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_AV1DEC_ABI_VERSION 4

/* The pass-2 work of one decoded frame. All pointers stay valid until the next
 * mi_dec_next() / mi_dec_destroy() on the same decoder. */
typedef struct MiDecFrame {
    int32_t w, h;                 /* coded luma size (frame_hdr.width[0], height) */
    int32_t up_w;                 /* luma width after super-resolution (width[1]); == w without */
    int32_t render_w, render_h;
    int32_t bpc, layout, sb128;
    /* intra path, decode order: blocks[i] predicted then tx[i] added (eob < 0: no residual);
     * deps[dep_start[i] .. dep_start[i + 1]) = earlier blocks owning pixels blocks[i] reads */
    const MiIntraBlock *intra;
    const MiTxBlock *intra_tx;
    int32_t n_intra;
    const int32_t *dep_start;     /* n_intra + 1 entries */
    const int32_t *deps;
    int32_t n_deps;
    /* residuals of inter blocks (added after motion compensation, before the intra path) */
    const MiTxBlock *inter_tx;
    int32_t n_inter_tx;
    /* coefficient arena: int16_t (8 bpc) or int32_t (10/12 bpc), ncoef entries. Entries
     * 0..15 are a reserved zero block: a transform block without residual (skip, or an
     * all-zero block) has eob < 0 and coef_off 0, so any consumer adds nothing. */
    const void *coef;
    size_t ncoef;
    const uint8_t *idx;           /* palette indices (MI_IPRED_PAL aux_off) */
    size_t nidx;
    const void *pal;              /* palette colours, pixels of bpc (MI_IPRED_PAL pal_off) */
    size_t npal;
    /* deblocking (MiLoopFilter inputs) */
    int32_t filter_y, filter_uv;
    const uint8_t *lf_level;      /* [rows][b4_stride][4] */
    int32_t b4_stride;
    const MiAv1Filter *lf_masks;  /* [sb128h][sb128w], tile fixups applied */
    int32_t sb128w, sb128h;
    uint8_t lim_e[64], lim_i[64];
    /* CDEF (seq_hdr.cdef) */
    int32_t cdef_on, cdef_damping;
    uint8_t cdef_y[8], cdef_uv[8];
    /* loop restoration */
    const MiAv1Restoration *lr_mask;   /* [sb128h][lr_sb128w] */
    int32_t lr_sb128w, restore_planes, lr_unit_size[2];
    /* inter prediction (recon_b_inter, recon.rs:3162-4045), run before the residuals: every count
     * is 0 in an intra frame. MiMcBlock / MiWarpBlock refs index the frame's seven references
     * (LAST .. ALTREF = MiDecEvent.ref_pic[0..6]). */
    const MiMcBlock *mc;              /* put / compound / MI_MC_PREP units, any order */
    int32_t n_mc;
    const MiMcBlock *obmc_h;          /* OBMC laps of above neighbours (blended first) */
    int32_t n_obmc_h;
    const MiMcBlock *obmc_v;          /* OBMC laps of left neighbours */
    int32_t n_obmc_v;
    const MiWarpBlock *warp;          /* warp8x8 / warp8x8t blocks */
    int32_t n_warp;
    const MiMcBlock *scaled;          /* units whose reference differs in size (put or MI_MC_PREP) */
    int32_t n_scaled;
    const MiMcCombine *combine_y;     /* compounds with a warped / scaled side: luma ... */
    int32_t n_combine_y;
    const MiMcCombine *combine_uv;    /* ... then chroma (its MASK units read what luma SEG wrote) */
    int32_t n_combine_uv;
    const uint8_t *masks;             /* wedge masks (MASK inputs) and room for SEG outputs */
    size_t nmasks;
    size_t ntmp;                      /* int16 elements of the arena the prep sides write */
    /* Optional: the intra queue mi_frame_run would plan (intra_plan.h), made off its critical
     * path (the front-end's frame jobs fill it): the n_intra blocks / transforms in queue order
     * (vertical strips, one per XCD, each by dependency level), dependencies as queue positions
     * (CSR, q_dep_start has n_intra + 1 entries), q_nstrips > 1: strip k = queue entries
     * [q_strip_start[k], q_strip_start[k + 1]); q_granules: edges handed over as granules (an
     * intra-only frame without inter-intra items). NULL q_intra: mi_frame_run plans. */
    const MiIntraBlock *q_intra;
    const MiTxBlock *q_intra_tx;
    const int32_t *q_dep_start;
    const int32_t *q_deps;
    int32_t q_n_deps;
    const int32_t *q_strip_start;
    int32_t q_nstrips;
    int32_t q_granules;
} MiDecFrame;

/* HDR metadata OBUs (OBU_METADATA, AV1 5.8; obu.rs, the Rav1dObuType::Metadata arm), as rav1d's
 * Rav1dContentLightLevel, Rav1dMasteringDisplay and Rav1dITUTT35 carry them with every picture.
 *
 * The OBU's payload starts with metadata_type, a leb128:
 *   1 (HDR CLL): max_cll, max_fall, 16 bits each.
 *   2 (HDR MDCV): the primaries (x, y) of three colours, 16 bits each (0.16 fixed point), the white
 *     point (x, y), then max_luminance (24.8 fixed point, cd/m2) and min_luminance (18.14), 32 bits
 *     each.
 *   After the fields of either come the trailing one bit and the byte alignment; a payload too
 *   short for all of that fails mi_dec_send with -EINVAL (check_for_overrun).
 *   4 (ITU-T T.35): itu_t_t35_country_code, one byte, then country_code_ext when the code is 0xff;
 *     the payload is every byte after that up to, not including, the last non-zero byte of the
 *     OBU (the trailing-bit byte 0x80; zero bytes after it are cut with it, zero bytes before it
 *     belong to the payload). A payload of no bytes is malformed: the OBU is ignored, no error.
 *     The bytes are delivered, not interpreted (HDR10+, Dolby Vision RPUs: the caller's).
 *   3 (scalability), 5 (timecode) and every other type are ignored without error.
 * Lifetime: content light and mastering display stay in force from picture to picture and are
 * forgotten when a sequence header arrives that differs from the current one (where the
 * reference slots are dropped too). A T.35 message belongs to the next frame submitted and is
 * then gone; a second one before that frame replaces the first.
 * Attachment: a frame takes the state in force when it is submitted (its last tile group has
 * arrived) and its picture keeps it: the event that shows the picture, a show_existing_frame
 * event included, reports what that frame took.
 * Delivery: MiDecEvent itself is unchanged (ABI 4: callers built against it stay binary
 * compatible); the metadata of an event is read with mi_dec_event_metadata() below, between the
 * mi_dec_next that returned the event and the next one. */
typedef struct MiContentLight { int32_t present; uint16_t max_cll, max_fall; } MiContentLight;
typedef struct MiMasteringDisplay { int32_t present; uint16_t primaries[3][2], white_point[2];
                                    uint32_t max_luminance, min_luminance; } MiMasteringDisplay;   /* 0.16, 24.8, 18.14 */
typedef struct MiItutT35 { const uint8_t *payload; int32_t size; uint8_t country_code, country_code_ext; } MiItutT35;
/* The HDR metadata of the shown picture's frame (show_pic >= 0; else of `frame`) of one event:
 * present 0 when the frame took none; itut_t35.payload NULL and size 0 without a T.35 message,
 * else `size` bytes valid until the next mi_dec_next, as release[] is. */
typedef struct MiDecMetadata {
    MiContentLight content_light;
    MiMasteringDisplay mastering_display;
    MiItutT35 itut_t35;
} MiDecMetadata;

/* One decoder event: a frame to reconstruct into picture `pic_id` (frame != NULL; its inter
 * prediction reads pictures ref_pic[]), and/or a picture to output (show_pic >= 0, with film
 * grain when fg_present). Pictures listed in release[] are no longer referenced.
 * show_pic need not be pic_id: a show_existing_frame names an earlier picture, and with
 * mi_dec_set_all_layers(d, 0) a shown frame's event has show_pic -1 (or the picture held back
 * before it) and the frame's picture is shown by a later event, or by none. A picture held
 * back is in no release[] before the event that shows or drops it. */
typedef struct MiDecEvent {
    const MiDecFrame *frame;
    int32_t pic_id;
    int32_t ref_pic[7];
    int32_t show_pic;
    int32_t fg_present;
    MiFilmGrainData fg;
    const int32_t *release;
    int32_t n_release;
    int32_t mtrx_identity;   /* seq_hdr.mtrx == DAV1D_MC_IDENTITY (the grain's chroma clip, fg_apply.rs) */
    /* (ABI 3) the OBU extension's layer ids of the shown picture's frame (show_pic >= 0; else
     * of `frame`), and whether that frame was the first decoded of its temporal unit */
    int32_t temporal_id, spatial_id;
    int32_t new_temporal_unit;
    /* (ABI 4) the colour description of the sequence header of the shown picture's frame
     * (show_pic >= 0; else of `frame`) */
    MiColorInfo color;
} MiDecEvent;

/* ---- device execution of a decoded frame (these two live in librav1d_amd.so) ----
 *
 * The pictures one frame's pass 2 writes (device planes, all of one geometry):
 * recon = prediction + residual, deblocked (recon -> deblocked), cdef (deblocked -> cdef),
 * restored ((cdef, deblocked) -> restored). Stages the frame header switches off are skipped,
 * not copied: *final receives the index (0 recon .. 3 restored) of the picture holding the
 * frame's reference-quality output (the picture rav1d leaves in f.sr_cur after
 * filter_sbrow: recon.rs:4019-4211).
 * `recon` is an intermediate, not an output: for an inter frame without intra blocks whose
 * deblocking is on and runs out of place (recon != deblocked), the DC-only residual blocks'
 * constants are added while deblocking (MI_ITX_DC_DEFER, mi_av1dsp.h), so `recon` lacks them
 * after the call; `deblocked` and every later picture are complete. */
typedef struct MiFramePictures {
    MiPicture recon, deblocked, cdef, restored;
    MiPicture refs[7];    /* the reference pictures of an inter frame (MiDecEvent.ref_pic order,
                             each the reference's final picture); unused for intra frames */
} MiFramePictures;

/* Enqueue one frame's reconstruction and in-loop filters on `stream` (recon_b_intra over the
 * intra work list in one persistent launch, blocks reordered by dependency level; then
 * mi_deblock_frame_to / mi_cdef_frame / mi_lr_frame). The host arrays of `f` are copied during
 * the call (pinned staging + async upload), so `f` may be released on return. Calls on one
 * context must use one stream. 0 or -errno (-EINVAL malformed work list, -ENOMEM, -EIO). */
int mi_frame_run(MiCtx *ctx, const MiDecFrame *f, const MiFramePictures *pics, int *final, void *stream);

/* The host-side checks mi_frame_run applies before enqueuing anything, without a device: 0, or
 * -EINVAL with *why (if non-NULL) naming the failed check. */
int mi_frame_validate(const MiDecFrame *f, const MiFramePictures *pics, const char **why);
/* Diagnostic: mean host time (ms) of mi_frame_run's planning pass over `f` (intra queue order,
 * dependency lists, inter unit buckets, residual bands), reps times; no device work. -1.0 when
 * the work list fails mi_frame_validate's checks (the pictures are not checked). */
double mi_frame_plan_ms(const MiDecFrame *f, int reps);

/* Wait for the work enqueued on `stream` and report device-side failures of the frame(s):
 * 0; -EINVAL when a kernel rejected (skipped) a descriptor no valid stream produces; -EIO
 * when a block's dependency wait gave up or a block was never reconstructed (the pictures
 * are then not valid). rav1d reports such a frame as a decode error (Dav1dResult,
 * src/error.rs). */
int mi_frame_end(MiCtx *ctx, void *stream);

/* Per-stage timing of mi_frame_run on one context (the §8(d) breakdown of a stream decode).
 * With timing on, every mi_frame_run records five HIP events on its stream; mi_ctx_timing
 * waits for them, sums the stages over the frames run since the last read, and resets.
 * Timing adds no synchronisation to mi_frame_run itself. */
typedef struct MiFrameTiming {
    int32_t frames;        /* frames run since the last read */
    int32_t reserved;
    double host_ms;        /* host time inside mi_frame_run: checks, dependency-level sort,
                              bucketing, staging copy (and any wait for the staging buffer) */
    double upload_ms;      /* device time of the descriptor + coefficient upload (H2D) */
    double inter_ms;       /* MC, warp, scaled, combine, OBMC laps, inter residuals */
    double intra_ms;       /* the persistent intra reconstruction launch */
    double filter_ms;      /* deblock, CDEF, super-resolution, loop restoration */
    int64_t upload_bytes;  /* bytes uploaded */
    double stage_ms;       /* of host_ms: the staging copy into pinned memory, with any wait for
                              the previous frame's upload to leave the staging buffer */
    double strips_ms;      /* of host_ms: the dependency levels and the XCD strip split */
} MiFrameTiming;
int mi_ctx_set_timing(MiCtx *ctx, int on);
int mi_ctx_timing(MiCtx *ctx, MiFrameTiming *out);

typedef struct MiDec MiDec;

int  mi_dec_create(MiDec **out);
void mi_dec_destroy(MiDec *d);
/* Frame threads (rav1d's Dav1dSettings.n_frame_threads, src/lib.rs): with n > 1, intra frames
 * are entropy-decoded on up to n worker threads while mi_dec_send parses on; mi_dec_next
 * still returns events in decode order and waits for the oldest frame's worker, so a caller
 * that wants the overlap sends a few temporal units ahead before draining. A worker's failure
 * is returned by the mi_dec_next of its frame. Default 1 (synchronous). 0 or -EINVAL. */
int  mi_dec_set_threads(MiDec *d, int n);
/* Dav1dSettings.inloop_filters (include/dav1d/dav1d.rs:17-35, src/lib.rs:136,218; the CLI's
 * --inloopfilters): the in-loop filters the frames this decoder emits ask mi_frame_run to
 * apply. A filter left out is skipped as rav1d's filter_sbrow_* skip it (recon.rs:4054, 4162,
 * 4178, 4290): the frame's filter_y / cdef_on / restore_planes are cleared, super-resolution
 * still runs, and the unfiltered picture is the reference later frames predict from. The bit
 * values are rav1d's. Default MI_INLOOPFILTER_ALL. 0 or -EINVAL. */
#define MI_INLOOPFILTER_NONE 0
#define MI_INLOOPFILTER_DEBLOCK (1 << 1)
#define MI_INLOOPFILTER_CDEF (1 << 2)
#define MI_INLOOPFILTER_RESTORATION (1 << 3)
#define MI_INLOOPFILTER_ALL (MI_INLOOPFILTER_DEBLOCK | MI_INLOOPFILTER_CDEF | MI_INLOOPFILTER_RESTORATION)
int  mi_dec_set_inloop_filters(MiDec *d, int flags);
/* The remaining decode controls of Dav1dSettings (src/lib.rs:199-219), each set before the
 * first mi_dec_send, each 0 or -EINVAL.
 *
 * operating_point (0..31, the CLI's --oppoint): at every sequence header the operating point
 * decoded is `op`, or 0 when the sequence has no more than `op` of them; OBUs whose extension
 * names a temporal or spatial layer outside its idc are dropped (sequence headers and temporal
 * delimiters excepted, obu.rs:2195-2205). Default 0.
 *
 * all_layers (--alllayers; default 1): with 0 and an operating point of more than one spatial
 * layer, only the highest spatial layer's picture of each temporal unit is shown; every frame
 * is still decoded, the lower layers being the references of the upper (output_picture_ready,
 * src/lib.rs:412-438). A shown picture waits in a one-picture cache: when the next one arrives
 * the cached picture is shown if it is of the operating point's highest spatial layer or the
 * new picture starts a temporal unit, and dropped otherwise. mi_dec_drain() at the end of the
 * input queues the last picture held back; it does nothing otherwise, with any settings.
 *
 * decode_frame_type (--decodeframetype): frames left out by type are neither reconstructed nor
 * shown (obu.rs:2493-2515, 2629-2648): REFERENCE leaves out inter, switch and intra-only frames
 * that refresh no slot, INTRA every inter and switch frame, KEY everything but key frames. The
 * slots such a frame refreshes keep its header and no picture: a later show_existing_frame of
 * one, or an inter frame predicting from one, is -EINVAL. Default ALL.
 *
 * frame_size_limit (--sizelimit): a frame header whose upscaled width * height exceeds `pixels`
 * makes mi_dec_send return -ERANGE (obu.rs:2342-2352). 0 (default): no limit. */
#define MI_DECODEFRAMETYPE_ALL 0
#define MI_DECODEFRAMETYPE_REFERENCE 1
#define MI_DECODEFRAMETYPE_INTRA 2
#define MI_DECODEFRAMETYPE_KEY 3
int  mi_dec_set_operating_point(MiDec *d, int op);
int  mi_dec_set_all_layers(MiDec *d, int on);
int  mi_dec_set_decode_frame_type(MiDec *d, int type);
int  mi_dec_set_frame_size_limit(MiDec *d, unsigned pixels);
int  mi_dec_drain(MiDec *d);
/* Feed one temporal unit (any whole number of OBUs). */
int  mi_dec_send(MiDec *d, const uint8_t *data, size_t size);
/* Next event: 1 and *ev filled, 0 when none is pending, or -errno. */
int  mi_dec_next(MiDec *d, MiDecEvent *ev);
/* The HDR metadata (MiDecMetadata above) of the event the last mi_dec_next on `d` returned with 1;
 * all zero before the first event. 0, or -EINVAL for a NULL argument. */
int  mi_dec_event_metadata(const MiDec *d, MiDecMetadata *out);
const char *mi_dec_error(const MiDec *d);

/* What a sequence header says about the pictures to come (Dav1dSequenceHeader's profile,
 * max_width / max_height, hbd, layout, film_grain_present and colour description). */
typedef struct MiSeqInfo {
    int32_t profile, max_w, max_h, bpc, layout, film_grain_present;
    MiColorInfo color;
} MiSeqInfo;
/* dav1d_parse_sequence_header (src/lib.rs): scan the OBUs of `data` and fill *out from the first
 * sequence header, without decoding anything. 0; -ENOENT when there is none; -EINVAL for null
 * arguments, a malformed OBU or a malformed sequence header. No decoder is needed. */
int  mi_dec_parse_sequence_header(const uint8_t *data, size_t size, MiSeqInfo *out);

#ifdef __cplusplus
}
#endif
#endif /* MI_AV1DEC_H */
