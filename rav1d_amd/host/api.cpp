// api.cpp — the C-ABI of the front-end (include/mi_av1dec.h).
#include <cerrno>
#include <new>

#include "decoder.h"
#include "mi_av1dec.h"

struct MiDec {
    av1::Decoder dec;
    av1::DecEvent cur;
    MiDecFrame frame;
    std::vector<int32_t> release;
    std::string err;
    int inloop = MI_INLOOPFILTER_ALL;
    bool has_cur = false;   // `cur` is an event mi_dec_next returned
};

extern "C" {

int mi_dec_create(MiDec **out) {
    if (!out) return -EINVAL;
    MiDec *d = new (std::nothrow) MiDec;
    if (!d) return -ENOMEM;
    *out = d;
    return 0;
}

void mi_dec_destroy(MiDec *d) { delete d; }

int mi_dec_set_threads(MiDec *d, int n) {
    if (!d || n < 1) return -EINVAL;
    d->dec.set_threads(n);
    return 0;
}

int mi_dec_set_inloop_filters(MiDec *d, int flags) {
    if (!d || (flags & ~MI_INLOOPFILTER_ALL)) return -EINVAL;
    d->inloop = flags;
    return 0;
}

int mi_dec_set_operating_point(MiDec *d, int op) {
    if (!d || op < 0 || op > 31) return -EINVAL;
    d->dec.operating_point = op;
    return 0;
}

int mi_dec_set_all_layers(MiDec *d, int on) {
    if (!d) return -EINVAL;
    d->dec.all_layers = on != 0;
    return 0;
}

int mi_dec_set_decode_frame_type(MiDec *d, int type) {
    if (!d || type < MI_DECODEFRAMETYPE_ALL || type > MI_DECODEFRAMETYPE_KEY) return -EINVAL;
    d->dec.decode_frame_type = type;
    return 0;
}

int mi_dec_set_frame_size_limit(MiDec *d, unsigned pixels) {
    if (!d) return -EINVAL;
    d->dec.frame_size_limit = pixels;
    return 0;
}

int mi_dec_drain(MiDec *d) {
    if (!d) return -EINVAL;
    try {
        d->dec.drain();
    } catch (const std::bad_alloc &) {
        d->dec.error = "out of memory";
        return -ENOMEM;
    }
    return 0;
}

const char *mi_dec_error(const MiDec *d) { return d ? d->dec.error.c_str() : "null decoder"; }

int mi_dec_send(MiDec *d, const uint8_t *data, size_t size) {
    if (!d || (!data && size)) return -EINVAL;
    try {
        const int r = d->dec.send(data, size);
        if (r < 0 && d->dec.error.find("not supported") != std::string::npos) return -ENOTSUP;
        return r;
    } catch (const std::bad_alloc &) {
        d->dec.error = "out of memory";
        return -ENOMEM;
    } catch (const std::exception &e) {
        // e.g. std::system_error from a frame thread that could not be started: no C++
        // exception crosses the C ABI
        d->dec.error = e.what();
        return -EAGAIN;
    }
}

int mi_dec_next(MiDec *d, MiDecEvent *ev) {
    if (!d || !ev) return -EINVAL;
    int r;
    try {
        r = d->dec.pop(d->cur);
    } catch (const std::exception &e) {
        d->dec.error = e.what();
        return -EAGAIN;
    }
    if (r <= 0) {
        if (r < 0) d->has_cur = false;   // (`cur` is the frame that failed)
        if (r < 0 && d->dec.error.find("not supported") != std::string::npos) return -ENOTSUP;
        return r;
    }
    d->has_cur = true;
    const av1::DecEvent &e = d->cur;
    memset(ev, 0, sizeof(*ev));
    ev->pic_id = e.pic_id;
    for (int i = 0; i < 7; i++) ev->ref_pic[i] = e.ref_pic[i];
    ev->show_pic = e.show_pic;
    ev->fg_present = e.fg_present;
    ev->fg = e.fg;
    ev->mtrx_identity = e.mtrx_identity;
    ev->temporal_id = e.temporal_id;
    ev->spatial_id = e.spatial_id;
    ev->new_temporal_unit = e.new_tu;
    ev->color = e.color;
    d->release.assign(e.release.begin(), e.release.end());
    ev->release = d->release.data();
    ev->n_release = (int32_t)d->release.size();
    if (e.work) {
        MiDecFrame &f = d->frame;
        av1::frame_view(*e.work, f);
        // Dav1dSettings.inloop_filters: a filter switched off is skipped for the whole frame
        if (!(d->inloop & MI_INLOOPFILTER_DEBLOCK)) f.filter_y = f.filter_uv = 0;
        if (!(d->inloop & MI_INLOOPFILTER_CDEF)) f.cdef_on = 0;
        if (!(d->inloop & MI_INLOOPFILTER_RESTORATION)) f.restore_planes = 0;
        ev->frame = &f;
    }
    return 1;
}

int mi_dec_event_metadata(const MiDec *d, MiDecMetadata *out) {
    if (!d || !out) return -EINVAL;
    memset(out, 0, sizeof(*out));
    if (!d->has_cur) return 0;
    const av1::FrameMeta &m = d->cur.meta;
    out->content_light = m.cll;
    out->mastering_display = m.mdcv;
    if (m.t35) {   // (d->cur keeps the bytes until the next mi_dec_next)
        out->itut_t35.payload = m.t35->payload.data();
        out->itut_t35.size = (int32_t)m.t35->payload.size();
        out->itut_t35.country_code = m.t35->country_code;
        out->itut_t35.country_code_ext = m.t35->country_code_ext;
    }
    return 0;
}

int mi_dec_parse_sequence_header(const uint8_t *data, size_t size, MiSeqInfo *out) {
    if (!data || !out) return -EINVAL;
    av1::SeqHdr s;
    const int r = av1::Decoder::find_seq_hdr(data, size, s);
    if (r < 0) return r;
    out->profile = s.profile;
    out->max_w = s.max_width;
    out->max_h = s.max_height;
    out->bpc = s.bpc;
    out->layout = s.layout;
    out->film_grain_present = s.film_grain_present;
    out->color = av1::color_info(s);
    return 0;
}

}  // extern "C"
