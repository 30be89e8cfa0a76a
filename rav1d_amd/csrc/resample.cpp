// resample.cpp — the host-only entries of the resampling filters (include/mi_av1out.h):
// mi_resample_plan, the sizes the device passes use for an axis, and mi_resample_taps, the axis's
// tap table from the generators of resize.h, the source the table kernel runs on the device. No
// device and no context, as mi_tonemap_tables: a CPU test can pin the tables and show that a
// segment's reach fits the tile before anything is launched.
#include <new>

#include "resize.h"

namespace {

int axis_check(const MiResample *rs, int n_in, int n_out, mi::Filter &f) {
    if (int e = mi::resample_check(rs, f)) return e;
    if (n_in < 1 || n_out < 1 || n_in > 65536 || n_out > 65536) return -EINVAL;
    if ((int64_t)n_in > 64 * (int64_t)n_out) return -EINVAL;
    return 0;
}

}  // namespace

extern "C" int mi_resample_plan(const MiResample *rs, int n_in, int n_out, int *cap, int *seg_outputs) {
    if (!cap || !seg_outputs) return -EINVAL;
    mi::Filter f;
    if (int e = axis_check(rs, n_in, n_out, f)) return e;
    *cap = mi::tap_cap(n_in, n_out, mi::filter_radius(f));
    *seg_outputs = mi::seg_outputs(n_in, n_out, mi::filter_radius(f));
    return 0;
}

extern "C" int mi_resample_taps(const MiResample *rs, int n_in, int n_out, int phase, int cap, int32_t *start,
                                int32_t *count, int32_t *k) {
    if (!start || !count || !k) return -EINVAL;
    mi::Filter f;
    if (int e = axis_check(rs, n_in, n_out, f)) return e;
    if (phase != 2 && phase != 4) return -EINVAL;
    const int need = mi::tap_cap(n_in, n_out, mi::filter_radius(f));
    if (cap < need) return -EINVAL;
    // the generators write one table start[n_out] count[n_out] k[need][n_out]
    int *tab = new (std::nothrow) int[(size_t)(need + 2) * n_out];
    if (!tab) return -ENOMEM;
    const mi::TapAxis ax{n_in, n_out, phase, need, tab};
    for (int o = 0; o < n_out; o++) {
        if (f.filter == MI_RS_CUBIC)
            mi::cubic_taps(ax, f.b, f.c, o);
        else
            mi::sited_taps(ax, o);
    }
    memcpy(start, tab, sizeof(int) * n_out);
    memcpy(count, tab + n_out, sizeof(int) * n_out);
    memcpy(k, tab + 2 * (size_t)n_out, sizeof(int) * (size_t)need * n_out);
    memset(k + (size_t)need * n_out, 0, sizeof(int) * (size_t)(cap - need) * n_out);
    delete[] tab;
    return 0;
}
