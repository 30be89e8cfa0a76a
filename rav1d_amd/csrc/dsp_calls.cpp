// dsp_calls.cpp — the table-compatible per-call entry points of include/mi_av1dsp.h (mi_dsp_*),
// which dsp_table.cpp wraps into the Rav1dDSPContext slots.
//
// The entries keep the reference's contract (caller owns buffers, callee zeroes the consumed
// coefficients, src/itx.rs:152-158) and accept host or device pointers with either stride sign.
// Each checks its arguments without touching the GPU, then runs a one-block launch synchronously
// through a Call: the process-wide lock, device 0 with its private stream, and device scratch
// handed out piece by piece.
#include <errno.h>
#include <initializer_list>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "ctx.h"

namespace {

// 1 MiB is the most an entry takes (mi_dsp_mc_resize, by its own check); the rest is what
// aligning its pieces can add.
constexpr size_t kScratch0 = (1 << 20) + 4096;

// Process-wide state of the per-call entries, on device 0; used under `mu` (Call).
struct CallState {
    std::mutex mu;
    bool ready = false;
    int err = 0;
    hipStream_t stream = nullptr;
    uint8_t *scratch = nullptr;     // pixels / coefficients / descriptors
    uint8_t *host = nullptr;        // as large: where windows of host callers are packed (Call::in / out)
    size_t scratch_bytes = 0;
    int init() {
        if (ready) return err;
        ready = true;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return err = -ENODEV;
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return err = -EIO;
        return err = alloc(kScratch0);
    }
    int alloc(size_t n) {
        host = (uint8_t *)malloc(n);
        if (!host || hipMalloc(&scratch, n) != hipSuccess) return -ENOMEM;
        scratch_bytes = n;
        return 0;
    }
    int reserve(size_t n) {   // grow the scratch (only ever grows)
        if (n <= scratch_bytes) return 0;
        if (hipStreamSynchronize(stream) != hipSuccess) return -EIO;
        auto drop = [this] {
            (void)hipFree(scratch);
            free(host);
            scratch = host = nullptr;
            scratch_bytes = 0;
        };
        drop();
        if (alloc(n)) {
            drop();
            if (alloc(kScratch0)) drop();
            return -ENOMEM;
        }
        return 0;
    }
};
CallState g_call;

// Rows [r0, r1) x bytes [b0, b1) around a base pointer, packed in device scratch.
struct Win {
    uint8_t *dev;
    int r0, r1;
    ptrdiff_t b0, b1;
    ptrdiff_t pitch() const { return b1 - b0; }
    uint8_t *origin() const { return dev + (size_t)(-r0) * pitch() - b0; }   // row 0, byte 0
};

// One per-call entry's turn, constructed after the argument checks that need no GPU. It holds
// the lock, has device 0 current on the calling thread until it goes out of scope (the caller's
// device is then current again), and hands out the scratch from its start. `err` is the call's
// first failure as -errno; once it is set the staging steps do nothing, so an entry checks it
// once before it launches.
struct Call {
    std::lock_guard<std::mutex> lk{g_call.mu};
    int err = 0;
    hipStream_t stream = nullptr;

    Call() {
        if (hipGetDevice(&prev) != hipSuccess) prev = 0;   // (no device: init() says so)
        if (prev != 0 && hipSetDevice(0) != hipSuccess) {
            prev = 0;
            err = -ENODEV;
            return;
        }
        err = g_call.init();
        stream = g_call.stream;
    }
    ~Call() {
        if (prev != 0) (void)hipSetDevice(prev);
    }

    // The next `bytes` of the scratch, aligned to 256. The allocation never moves under a
    // pointer handed out: a call that needs more than the scratch holds reserves it first.
    uint8_t *take(size_t bytes) {
        const size_t at = (used + 255) & ~(size_t)255;
        if (!err && at + bytes > g_call.scratch_bytes) err = -ENOMEM;
        if (err) return nullptr;
        used = at + bytes;
        return g_call.scratch + at;
    }
    // Before the first take: room for pieces of these sizes (the scratch's one growth point).
    int reserve(std::initializer_list<size_t> pieces) {
        size_t total = 0;
        for (size_t n : pieces) total += (n + 255) & ~(size_t)255;
        if (!err && !used) err = g_call.reserve(total);
        return err;
    }
    Win win(int r0, int r1, ptrdiff_t b0, ptrdiff_t b1) { return Win{take((size_t)(r1 - r0) * (b1 - b0)), r0, r1, b0, b1}; }

    // caller (host or device) -> scratch
    void copy_in(void *dev, const void *src, size_t n) {
        if (!err && hipMemcpyAsync(dev, src, n, hipMemcpyDefault, stream) != hipSuccess) err = -EIO;
    }
    uint8_t *stage(const void *src, size_t n) {   // a piece of the scratch holding n bytes of the caller's
        uint8_t *dev = take(n);
        copy_in(dev, src, n);
        return dev;
    }
    // (a window in host memory is packed by the CPU and crosses in one copy, here and in out(): a
    // copy per row costs more than a small block's kernel)
    void in(const Win &w, const void *base, ptrdiff_t stride) {
        if (err) return;
        const size_t n = w.pitch();
        const bool dev = on_device(base);
        uint8_t *to = dev ? w.dev : packed(w);
        for (int r = w.r0; r < w.r1; r++, to += n) {
            const uint8_t *row = (const uint8_t *)base + r * stride + w.b0;
            if (dev) copy_in(to, row, n);
            else memcpy(to, row, n);
        }
        if (!dev) copy_in(w.dev, packed(w), (size_t)(w.r1 - w.r0) * n);
    }
    // The samples a filter reaches around a source block: rows [-lead, r1) x samples [-lead, c1)
    // of `src`, staged; origin() is sample (0, 0).
    Win reach_in(const void *src, ptrdiff_t stride, int lead, int r1, int c1, int px) {
        const Win w = win(-lead, r1, (ptrdiff_t)-lead * px, (ptrdiff_t)c1 * px);
        in(w, src, stride);
        return w;
    }
    // A few bytes the host needs before it can stage the rest (masks, levels, parameters).
    void peek(void *host, const void *src, size_t n) {
        if (!err && hipMemcpy(host, src, n, hipMemcpyDefault) != hipSuccess) err = -EIO;
    }

    // scratch -> caller; the call's work is complete when finish() returns
    void copy_out(void *dst, const void *dev, size_t n) {
        if (!err && hipMemcpyAsync(dst, dev, n, hipMemcpyDefault, stream) != hipSuccess) err = -EIO;
    }
    int finish() {
        if (!err && hipStreamSynchronize(stream) != hipSuccess) err = -EIO;
        return err;
    }
    int result(void *dst, const void *dev, size_t n) {
        copy_out(dst, dev, n);
        return finish();
    }
    int out(void *base, ptrdiff_t stride, const Win &w) {
        if (err) return err;
        const size_t n = w.pitch();
        const bool dev = on_device(base);
        if (!dev) copy_out(packed(w), w.dev, (size_t)(w.r1 - w.r0) * n);
        if (!dev && finish()) return err;
        const uint8_t *from = dev ? w.dev : packed(w);
        for (int r = w.r0; r < w.r1; r++, from += n) {
            uint8_t *row = (uint8_t *)base + r * stride + w.b0;
            if (dev) copy_out(row, from, n);
            else memcpy(row, from, n);
        }
        return dev ? finish() : 0;
    }

  private:
    int prev = 0;
    size_t used = 0;
    uint8_t *packed(const Win &w) const { return g_call.host + (w.dev - g_call.scratch); }
    static bool on_device(const void *p) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess) {
            (void)hipGetLastError();   // plain host memory is unknown to the runtime
            return false;
        }
        return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
    }
};

int bpc_of(int bitdepth_max) {
    return bitdepth_max == 255 ? 8 : bitdepth_max == 1023 ? 10 : bitdepth_max == 4095 ? 12 : 0;
}

}  // namespace

extern "C" {

int mi_dsp_itxfm_add(int tx, int txtp, void *dst, ptrdiff_t stride, void *coeff, int eob,
                     int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (tx < 0 || tx >= MI_N_RECT_TX_SIZES || !mi::itx_type_valid(tx, txtp) || !dst || !coeff ||
        eob < 0 || !bpc)
        return -EINVAL;
    const mi::TxDim d = mi::tx_dim(tx);
    const int px = bpc == 8 ? 1 : 2;
    const size_t coef_bytes = (size_t)mi::imin_c(d.w, 32) * mi::imin_c(d.h, 32) * (bpc == 8 ? 2 : 4);
    MiTxBlock hb{};
    hb.tx = (uint8_t)tx;
    hb.txtp = (uint8_t)txtp;
    hb.eob = eob;
    Call c;
    const Win pix = c.win(0, d.h, 0, (ptrdiff_t)d.w * px);
    uint8_t *dcoef = c.stage(coeff, coef_bytes);
    MiTxBlock *dblk = (MiTxBlock *)c.stage(&hb, sizeof(hb));
    int *derr = (int *)c.take(sizeof(int));   // scratch word: the host checked tx / txtp above
    c.in(pix, dst, stride);
    if (c.err) return c.err;

    mi::ItxArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < 3; p++) { a.plane[p] = pix.dev; a.stride[p] = pix.pitch(); }
    a.blocks = dblk;
    a.coef = dcoef;
    a.bdmax = bitdepth_max;
    a.zero_coefs = 1;
    a.pw[0] = d.w;
    a.ph[0] = d.h;
    a.err = derr;
    uint32_t ss1[MI_N_RECT_TX_SIZES + 1];
    for (int k = 0; k <= MI_N_RECT_TX_SIZES; k++) ss1[k] = k > tx ? 1 : 0;
    const int nwg = mi::itx_fill_schedule(a, ss1);
    if (mi::launch_itx_frame(a, nwg, bpc, c.stream)) return -EIO;
    c.copy_out(coeff, dcoef, coef_bytes);   // zeroed: the caller's buffer is consumed
    return c.out(dst, stride, pix);
}

namespace {
// one block through the batched intra-prediction kernel, and its hb.w x hb.h pixels to the caller
int ipred_call(Call &c, void *dst, ptrdiff_t stride, const MiIpredBlock &hb, const uint8_t *dedge, const void *dac,
               const uint8_t *didx, int bpc, int bitdepth_max) {
    const Win pix = c.win(0, hb.h, 0, (ptrdiff_t)hb.w * (bpc == 8 ? 1 : 2));
    MiIpredBlock *dblk = (MiIpredBlock *)c.stage(&hb, sizeof(hb));
    if (c.err) return c.err;
    mi::IpredArgs a;
    memset(&a, 0, sizeof(a));
    for (int p = 0; p < 3; p++) a.dst[p] = pix.dev;
    a.stride[0] = a.stride[1] = pix.pitch();
    a.blocks = dblk;
    a.edges = dedge;
    a.ac = (const int16_t *)dac;
    a.idx = didx;
    a.bpc = bpc;
    a.bdmax = bitdepth_max;
    if (mi::launch_ipred(a, 1, c.stream)) return -EIO;
    return c.out(dst, stride, pix);
}
}  // namespace

int mi_dsp_intra_pred(int mode, void *dst, ptrdiff_t stride, const void *topleft, int w, int h,
                      int angle, int max_width, int max_height, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (mode < 0 || mode > 13 || !dst || !topleft || w < 4 || h < 4 || w > 64 || h > 64 ||
        (w & (w - 1)) || (h & (h - 1)) || (mode == 13 && (w > 32 || h > 32)) || !bpc)
        return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    const int ext = w + h;                      // samples read on each side of topleft
    Call c;
    uint8_t *dedge = c.stage((const uint8_t *)topleft - (ptrdiff_t)ext * px, (size_t)(2 * ext + 1) * px);
    MiIpredBlock hb{};
    hb.edge_off = (uint32_t)ext;
    hb.w = (uint8_t)w;
    hb.h = (uint8_t)h;
    hb.mode = (uint8_t)mode;
    hb.angle = (uint16_t)angle;
    hb.max_w = (uint16_t)max_width;
    hb.max_h = (uint16_t)max_height;
    return ipred_call(c, dst, stride, hb, dedge, nullptr, nullptr, bpc, bitdepth_max);
}

int mi_dsp_cfl_pred(int mode, void *dst, ptrdiff_t stride, const void *topleft, int w, int h, const int16_t *ac,
                    int alpha, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !dst || !topleft || !ac || (mode != 0 && mode != 3 && mode != 4 && mode != 5) || w < 4 || h < 4 ||
        w > 32 || h > 32 || (w & (w - 1)) || (h & (h - 1)))
        return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    Call c;
    uint8_t *dedge = c.stage((const uint8_t *)topleft - (ptrdiff_t)h * px, (size_t)(w + h + 1) * px);
    uint8_t *dac = c.stage(ac, (size_t)w * h * 2);
    MiIpredBlock hb{};
    hb.edge_off = (uint32_t)h;
    hb.w = (uint8_t)w;
    hb.h = (uint8_t)h;
    hb.mode = (uint8_t)(MI_IPRED_CFL + mode);
    hb.alpha = (int8_t)alpha;
    return ipred_call(c, dst, stride, hb, dedge, dac, nullptr, bpc, bitdepth_max);
}

int mi_dsp_pal_pred(void *dst, ptrdiff_t stride, const void *pal, const uint8_t *idx, int w, int h, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !dst || !pal || !idx || w < 4 || h < 4 || w > 64 || h > 64) return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    Call c;
    uint8_t *dpal = c.stage(pal, 8 * (size_t)px), *didx = c.stage(idx, (size_t)w * h);
    MiIpredBlock hb{};
    hb.w = (uint8_t)w;
    hb.h = (uint8_t)h;
    hb.mode = MI_IPRED_PAL;
    return ipred_call(c, dst, stride, hb, dpal, nullptr, didx, bpc, bitdepth_max);
}

int mi_dsp_cfl_ac(int layout, int16_t *ac, const void *y, ptrdiff_t stride, int w_pad, int h_pad, int cw, int ch,
                  int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !ac || !y || layout < 1 || layout > 3 || cw < 4 || ch < 4 || cw > 32 || ch > 32 ||
        (cw & (cw - 1)) || (ch & (ch - 1)) || w_pad < 0 || h_pad < 0 || 4 * w_pad >= cw || 4 * h_pad >= ch)
        return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    const int ss_hor = layout != 3, ss_ver = layout == 1;
    const int rows = (ch - 4 * h_pad) << ss_ver, cols = (cw - 4 * w_pad) << ss_hor;
    Call c;
    const Win luma = c.win(0, rows, 0, (ptrdiff_t)cols * px);
    int16_t *dac = (int16_t *)c.take((size_t)cw * ch * 2);
    c.in(luma, y, stride);
    if (c.err) return c.err;
    mi::CflAcArgs a;
    a.ac = dac;
    a.y = luma.dev;
    a.stride = luma.pitch();
    a.w_pad = w_pad;
    a.h_pad = h_pad;
    a.cw = cw;
    a.ch = ch;
    a.ss_hor = ss_hor;
    a.ss_ver = ss_ver;
    if (mi::launch_cfl_ac(a, bpc, c.stream)) return -EIO;
    return c.result(ac, dac, (size_t)cw * ch * 2);
}

int mi_dsp_loop_filter_sb(int cls, int dir, void *dst, ptrdiff_t stride, const uint32_t *vmask,
                          const uint8_t (*lvl)[4], ptrdiff_t b4_stride, const void *lut, int wh, int bitdepth_max) {
    (void)wh;
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || cls < 0 || cls > 1 || dir < 0 || dir > 1 || !dst || !vmask || !lvl || !lut) return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    Call c;
    mi::LfCallArgs a;
    memset(&a, 0, sizeof(a));
    c.peek(a.vmask, vmask, (cls ? 2 : 3) * sizeof(uint32_t));
    if (c.err) return c.err;
    const unsigned vm = a.vmask[0] | a.vmask[1] | a.vmask[2];
    if (!vm) return 0;
    const int nu = 32 - __builtin_clz(vm);                 // units up to the highest set bit
    // level pairs {unit, neighbour}: the caller's map is strided (b4_stride entries per row)
    uint8_t lv[64] = {0};
    const ptrdiff_t ul = dir == 0 ? b4_stride : 1, pl = dir == 0 ? -1 : -b4_stride;
    for (int k = 0; k < nu; k++) {
        if (!(vm & (1u << k))) continue;
        c.peek(&lv[2 * k], &lvl[k * ul][0], 1);
        c.peek(&lv[2 * k + 1], &lvl[k * ul + pl][0], 1);
    }
    uint8_t lt[128];
    c.peek(lt, lut, 128);   // Av1FilterLUT.e, .i
    memcpy(a.lim_e, lt, 64);
    memcpy(a.lim_i, lt + 64, 64);
    // the pixel window: 8 samples either side of the edge, 4 * nu along it
    const Win pix = dir == 0 ? c.win(0, 4 * nu, -8 * px, 8 * px) : c.win(-8, 8, 0, (ptrdiff_t)4 * nu * px);
    uint8_t *dlv = c.stage(lv, sizeof(lv));
    c.in(pix, dst, stride);
    if (c.err) return c.err;
    a.dst = pix.origin();
    a.stride = pix.pitch();
    a.lvl = dlv;
    a.cls = cls;
    a.dir = dir;
    a.bdm8 = bpc - 8;
    a.bdmax = bitdepth_max;
    if (mi::launch_lf_sb_call(a, bpc, c.stream)) return -EIO;
    return c.out(dst, stride, pix);
}

int mi_dsp_cdef_filter(int fb, void *dst, ptrdiff_t stride, const void *left, const void *top, const void *bottom,
                       int pri, int sec, int dir, int damping, int edges, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || fb < 0 || fb > 2 || !dst || dir < 0 || dir > 7 || pri < 0 || sec < 0) return -EINVAL;
    const int w = fb == 0 ? 8 : 4, h = fb == 2 ? 4 : 8;
    if (((edges & 1) && !left) || ((edges & 4) && !top) || ((edges & 8) && !bottom)) return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    Call c;
    // one packed window, rows -2 .. h + 2 of samples -2 .. w + 2: the block, two rows of top above
    // and of bottom below it; only the columns the edge flags allow are read from the caller
    const Win win = c.win(-2, h + 2, -2 * px, (ptrdiff_t)(w + 2) * px);
    uint8_t *dleft = c.take((size_t)h * 2 * px);
    const Win res = c.win(0, h, 0, (ptrdiff_t)w * px);
    if (c.err) return c.err;
    const ptrdiff_t x0 = (edges & 1) ? -2 * px : 0, x1 = (ptrdiff_t)(w + ((edges & 2) ? 2 : 0)) * px;
    auto rows = [&](const void *src, int r0, int n, ptrdiff_t c0) {   // src rows 0 .. n to window rows r0 ..
        for (int r = 0; r < n; r++)
            c.copy_in(win.origin() + (r0 + r) * win.pitch() + c0, (const uint8_t *)src + r * stride + c0, x1 - c0);
    };
    rows(dst, 0, h, 0);
    if (edges & 4) rows(top, -2, 2, x0);
    if (edges & 8) rows(bottom, h, 2, x0);
    if (edges & 1) c.copy_in(dleft, left, (size_t)h * 2 * px);
    if (c.err) return c.err;
    mi::CdefCallArgs a;
    memset(&a, 0, sizeof(a));
    a.top = win.origin() - 2 * win.pitch();
    a.dst = win.origin();
    a.bottom = win.origin() + h * win.pitch();
    a.left = dleft;
    a.out = res.dev;
    a.stride = win.pitch();
    a.w = w;
    a.h = h;
    a.pri = pri;
    a.sec = sec;
    a.dir = dir;
    a.damping = damping;
    a.edges = edges;
    a.bdm8 = bpc - 8;
    if (mi::launch_cdef_call(a, bpc, false, c.stream)) return -EIO;
    return c.out(dst, stride, res);
}

int mi_dsp_cdef_dir(const void *img, ptrdiff_t stride, unsigned *var, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !img || !var) return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    Call c;
    const Win win = c.win(0, 8, 0, 8 * px);
    int r[2];   // {dir, var}
    uint8_t *dout = c.take(sizeof(r));
    c.in(win, img, stride);
    if (c.err) return c.err;
    mi::CdefCallArgs a;
    memset(&a, 0, sizeof(a));
    a.dst = win.dev;
    a.out = dout;
    a.stride = win.pitch();
    a.bdm8 = bpc - 8;
    if (mi::launch_cdef_call(a, bpc, true, c.stream)) return -EIO;
    if (int e = c.result(r, dout, sizeof(r))) return e;
    *var = (unsigned)r[1];
    return r[0];
}

// ---- mc table (src/mc.rs:1174-1338): put / prep, combine, blend, emu_edge ----
namespace {
// what every mc kernel takes: the source at sample (0, 0), the packed result (pixels, or the
// int16 intermediate of a prep), the block size and the bit depth
mi::McCallArgs mc_args(const uint8_t *src, int64_t src_stride, const Win &res, int w, int h, int bpc, int bdmax) {
    mi::McCallArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src;
    a.src_stride = src_stride;
    a.dst = res.dev;
    a.dst_stride = res.pitch();
    a.tmp1 = (int16_t *)res.dev;
    a.w = w;
    a.h = h;
    a.bpc = bpc;
    a.ib = bpc == 8 ? 4 : 14 - bpc;
    a.bias = bpc == 8 ? 0 : 8192;
    a.bdmax = bdmax;
    return a;
}
bool mc_dims_ok(int w, int h) { return w >= 2 && h >= 2 && w <= 128 && h <= 128; }

// put (dst) / prep (tmp)
int mc_put_prep(int filter2d, void *dst, ptrdiff_t dst_stride, int16_t *tmp, const void *src, ptrdiff_t src_stride,
                int w, int h, int mx, int my, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !(tmp ? (void *)tmp : dst) || !src || filter2d < 0 || filter2d > 9 || !mc_dims_ok(w, h) || mx < 0 ||
        mx > 15 || my < 0 || my > 15)
        return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    Call c;
    // source window: rows -3 .. h+4, columns -3 .. w+4 (8-tap reach; bilinear uses +1)
    const int lead = filter2d == 9 ? 0 : 3, tail = filter2d == 9 ? 1 : 5;
    const Win win = c.reach_in(src, src_stride, lead, h + tail, w + tail, px);
    const Win res = c.win(0, h, 0, (ptrdiff_t)w * (tmp ? 2 : px));
    if (c.err) return c.err;
    mi::McCallArgs a = mc_args(win.origin(), win.pitch(), res, w, h, bpc, bitdepth_max);
    a.prep = tmp != nullptr;
    a.mx = mx; a.my = my; a.filter2d = filter2d;
    if (mi::launch_mc_call(a, 0, c.stream)) return -EIO;
    return tmp ? c.result(tmp, res.dev, (size_t)w * h * 2) : c.out(dst, dst_stride, res);
}
}  // namespace

int mi_dsp_mc_put(int filter2d, void *dst, ptrdiff_t dst_stride, const void *src, ptrdiff_t src_stride, int w, int h,
                  int mx, int my, int bitdepth_max) {
    return mc_put_prep(filter2d, dst, dst_stride, nullptr, src, src_stride, w, h, mx, my, bitdepth_max);
}

int mi_dsp_mc_prep(int filter2d, int16_t *tmp, const void *src, ptrdiff_t src_stride, int w, int h, int mx, int my,
                   int bitdepth_max) {
    if (!tmp) return -EINVAL;
    return mc_put_prep(filter2d, nullptr, 0, tmp, src, src_stride, w, h, mx, my, bitdepth_max);
}

namespace {
// avg / w_avg / mask / w_mask / blend*: op as mc_call_comb_kernel
int mc_combine(int op, void *dst, ptrdiff_t ds, const int16_t *t1, const int16_t *t2, const void *tmp_px,
               int w, int h, const uint8_t *mask, uint8_t *mask_out, int weight, int sign, int layout, int bdmax) {
    const int bpc = bpc_of(bdmax);
    if (!bpc || !dst || !mc_dims_ok(w, h)) return -EINVAL;
    if ((op <= 3 && (!t1 || !t2)) || ((op == 2 || op == 4) && !mask) || (op == 3 && !mask_out) ||
        (op >= 4 && !tmp_px) || (op == 3 && (layout < 1 || layout > 3)))
        return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    const size_t n = (size_t)w * h;
    Call c;
    const Win pix = c.win(0, h, 0, (ptrdiff_t)w * px);
    // (the kernel reads only what its op takes: the intermediates up to w_mask, pixels in the blends)
    uint8_t *d1 = op <= 3 ? c.stage(t1, n * 2) : nullptr, *d2 = op <= 3 ? c.stage(t2, n * 2) : nullptr;
    uint8_t *dm = op == 2 || op == 4 ? c.stage(mask, n) : nullptr, *dmo = c.take(n);
    uint8_t *dt = op >= 4 ? c.stage(tmp_px, n * px) : nullptr;
    if (op >= 4) c.in(pix, dst, ds);   // blends read dst
    if (c.err) return c.err;
    mi::McCallArgs a = mc_args(dt, 0, pix, w, h, bpc, bdmax);
    a.tmp1 = (int16_t *)d1;
    a.tmp2 = (const int16_t *)d2;
    a.mask = dm;
    a.mask_out = dmo;
    a.op = op; a.weight = weight; a.sign = sign;
    a.ss_hor = layout == 1 || layout == 2;
    a.ss_ver = layout == 1;
    if (mi::launch_mc_call(a, 1, c.stream)) return -EIO;
    if (op == 3) c.copy_out(mask_out, dmo, (size_t)(w >> a.ss_hor) * (h >> a.ss_ver));
    return c.out(dst, ds, pix);
}
}  // namespace

int mi_dsp_mc_avg(void *dst, ptrdiff_t dst_stride, const int16_t *tmp1, const int16_t *tmp2, int w, int h,
                  int bitdepth_max) {
    return mc_combine(0, dst, dst_stride, tmp1, tmp2, nullptr, w, h, nullptr, nullptr, 0, 0, 0, bitdepth_max);
}
int mi_dsp_mc_w_avg(void *dst, ptrdiff_t dst_stride, const int16_t *tmp1, const int16_t *tmp2, int w, int h, int weight,
                    int bitdepth_max) {
    return mc_combine(1, dst, dst_stride, tmp1, tmp2, nullptr, w, h, nullptr, nullptr, weight, 0, 0, bitdepth_max);
}
int mi_dsp_mc_mask(void *dst, ptrdiff_t dst_stride, const int16_t *tmp1, const int16_t *tmp2, int w, int h,
                   const uint8_t *mask, int bitdepth_max) {
    return mc_combine(2, dst, dst_stride, tmp1, tmp2, nullptr, w, h, mask, nullptr, 0, 0, 0, bitdepth_max);
}
int mi_dsp_mc_w_mask(int layout, void *dst, ptrdiff_t dst_stride, const int16_t *tmp1, const int16_t *tmp2, int w,
                     int h, uint8_t *mask, int sign, int bitdepth_max) {
    return mc_combine(3, dst, dst_stride, tmp1, tmp2, nullptr, w, h, nullptr, mask, 0, sign, layout, bitdepth_max);
}
int mi_dsp_mc_blend(void *dst, ptrdiff_t dst_stride, const void *tmp, int w, int h, const uint8_t *mask,
                    int bitdepth_max) {
    return mc_combine(4, dst, dst_stride, nullptr, nullptr, tmp, w, h, mask, nullptr, 0, 0, 0, bitdepth_max);
}
int mi_dsp_mc_blend_v(void *dst, ptrdiff_t dst_stride, const void *tmp, int w, int h, int bitdepth_max) {
    return mc_combine(5, dst, dst_stride, nullptr, nullptr, tmp, w, h, nullptr, nullptr, 0, 0, 0, bitdepth_max);
}
int mi_dsp_mc_blend_h(void *dst, ptrdiff_t dst_stride, const void *tmp, int w, int h, int bitdepth_max) {
    return mc_combine(6, dst, dst_stride, nullptr, nullptr, tmp, w, h, nullptr, nullptr, 0, 0, 0, bitdepth_max);
}

int mi_dsp_mc_emu_edge(int bw, int bh, int iw, int ih, int x, int y, void *dst, ptrdiff_t dst_stride, const void *ref,
                       ptrdiff_t ref_stride, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !dst || !ref || bw < 1 || bh < 1 || bw > 256 || bh > 256 || iw < 1 || ih < 1) return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    auto clip = [](int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; };
    // the reference pixels the block can reach: the clamped rectangle
    const int ry0 = clip(y, 0, ih - 1), ry1 = clip(y + bh - 1, 0, ih - 1) + 1;
    const int rx0 = clip(x, 0, iw - 1), rx1 = clip(x + bw - 1, 0, iw - 1) + 1;
    Call c;
    const Win win = c.win(0, ry1 - ry0, 0, (ptrdiff_t)(rx1 - rx0) * px), res = c.win(0, bh, 0, (ptrdiff_t)bw * px);
    c.in(win, (const uint8_t *)ref + (ptrdiff_t)ry0 * ref_stride + (ptrdiff_t)rx0 * px, ref_stride);
    if (c.err) return c.err;
    mi::McCallArgs a = mc_args(win.dev, win.pitch(), res, bw, bh, bpc, bitdepth_max);
    a.mx = x; a.my = y; a.iw = iw; a.ih = ih;
    if (mi::launch_mc_call(a, 2, c.stream)) return -EIO;
    return c.out(dst, dst_stride, res);
}

int mi_dsp_mc_warp8x8(int prep, void *dst, ptrdiff_t dst_stride, const void *src, ptrdiff_t src_stride,
                      const int16_t *abcd, int mx, int my, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !dst || !src || !abcd) return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    Call c;
    int16_t hb[4];
    c.peek(hb, abcd, sizeof(hb));
    const Win win = c.reach_in(src, src_stride, 3, 12, 12, px);
    // warp8x8t: dst is the int16 intermediate with stride dst_stride (in elements, as the
    // reference's tmp_stride); warp8x8: pixels
    const Win res = c.win(0, 8, 0, 8 * (prep ? 2 : px));
    if (c.err) return c.err;
    mi::McCallArgs a = mc_args(win.origin(), win.pitch(), res, 8, 8, bpc, bitdepth_max);
    a.prep = prep;
    a.mx = mx; a.my = my;
    for (int i = 0; i < 4; i++) a.abcd[i] = hb[i];
    if (mi::launch_mc_call(a, 3, c.stream)) return -EIO;
    return c.out(dst, prep ? dst_stride * 2 : dst_stride, res);
}

int mi_dsp_mc_resize(void *dst, ptrdiff_t dst_stride, const void *src, ptrdiff_t src_stride, int dst_w, int h,
                     int src_w, int dx, int mx0, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !dst || !src || dst_w < 1 || h < 1 || src_w < 1 || dst_w > 8192 || src_w > 8192 || h > 64 ||
        mx0 < 0 || mx0 >= (1 << 14))
        return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    Call c;
    if (c.err) return c.err;
    if ((size_t)(src_w + dst_w) * h * px > (1u << 20)) return -EINVAL;
    const Win win = c.win(0, h, 0, (ptrdiff_t)src_w * px), res = c.win(0, h, 0, (ptrdiff_t)dst_w * px);
    c.in(win, src, src_stride);
    if (c.err) return c.err;
    mi::McCallArgs a = mc_args(win.dev, win.pitch(), res, dst_w, h, bpc, bitdepth_max);
    a.iw = src_w; a.mx = mx0; a.weight = dx;
    if (mi::launch_mc_call(a, 4, c.stream)) return -EIO;
    return c.out(dst, dst_stride, res);
}

int mi_dsp_mc_scaled(int prep, int filter2d, void *dst, ptrdiff_t dst_stride, const void *src, ptrdiff_t src_stride,
                     int w, int h, int mx, int my, int dx, int dy, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !dst || !src || filter2d < 0 || filter2d > 9 || !mc_dims_ok(w, h) || mx < 0 || mx >= 1024 || my < 0 ||
        my >= 1024 || dx < 1 || dy < 1 || dx > 2048 || dy > 2048)
        return -EINVAL;
    const int px = bpc == 8 ? 1 : 2;
    Call c;
    if (c.err) return c.err;
    // source reach: rows -3 .. ((h-1)*dy + my >> 10) + 4, columns -3 .. ((w-1)*dx + mx >> 10) + 4
    const int r1 = (((h - 1) * dy + my) >> 10) + 5, c1 = (((w - 1) * dx + mx) >> 10) + 5;
    if ((size_t)(r1 + 3) * (c1 + 3) * px > (1u << 19)) return -EINVAL;
    const Win win = c.reach_in(src, src_stride, 3, r1, c1, px);
    const Win res = c.win(0, h, 0, (ptrdiff_t)w * (prep ? 2 : px));
    if (c.err) return c.err;
    mi::McCallArgs a = mc_args(win.origin(), win.pitch(), res, w, h, bpc, bitdepth_max);
    a.prep = prep;
    a.mx = mx; a.my = my; a.dx = dx; a.dy = dy; a.filter2d = filter2d;
    if (mi::launch_mc_call(a, 5, c.stream)) return -EIO;
    return prep ? c.result(dst, res.dev, (size_t)w * h * 2) : c.out(dst, dst_stride, res);
}

// ---- lr table (src/looprestoration.rs:91-107): wiener, sgr[kind] on one unit ----
namespace {
// Stage the unit's pixels (columns 0 .. w + 3*have_right), the lpf rows 0, 1, 6, 7 (columns
// -3*have_left .. w + 3*have_right) and left[h][4] into windows of one pitch (samples -3 .. w + 3),
// filter, and write the w x h result back over p.
int lr_call(Call &c, mi::LrCallArgs &a, void *p, ptrdiff_t stride, const void *left, const void *lpf, int w, int h,
            int edges, int bpc) {
    const int px = bpc == 8 ? 1 : 2;
    const bool hl = edges & 1, hr = edges & 2, ht = edges & 4, hb = edges & 8;
    if ((hl && !left) || ((ht || hb) && !lpf)) return -EINVAL;
    const Win dp = c.win(0, h, -3 * px, (ptrdiff_t)(w + 3) * px), dlpf = c.win(0, 8, dp.b0, dp.b1);
    uint8_t *dleft = c.take((size_t)h * 4 * px);
    const Win res = c.win(0, h, 0, (ptrdiff_t)w * px);
    if (c.err) return c.err;
    auto row = [&](const Win &d, const void *src, int r, ptrdiff_t c0, ptrdiff_t c1) {
        c.copy_in(d.origin() + r * d.pitch() + c0, (const uint8_t *)src + r * stride + c0, c1 - c0);
    };
    const ptrdiff_t c1 = (ptrdiff_t)(w + (hr ? 3 : 0)) * px, lc0 = hl ? -3 * px : 0;
    for (int r = 0; r < h; r++) row(dp, p, r, 0, c1);
    if (ht) for (int r = 0; r < 2; r++) row(dlpf, lpf, r, lc0, c1);
    if (hb) for (int r = 6; r < 8; r++) row(dlpf, lpf, r, lc0, c1);
    if (hl) c.copy_in(dleft, left, (size_t)h * 4 * px);
    if (c.err) return c.err;
    a.p = dp.origin();
    a.lpf = dlpf.origin();
    a.left = dleft;
    a.out = res.dev;
    a.ps = dp.pitch() / px;
    a.w = w;
    a.h = h;
    a.edges = edges;
    a.bd = bpc;
    if (mi::launch_lr_call(a, bpc, c.stream)) return -EIO;
    return c.out(p, stride, res);
}
bool lr_dims_ok(int w, int h) { return w >= 1 && w <= 384 && h >= 1 && h <= 64; }
}  // namespace

int mi_dsp_lr_wiener(void *p, ptrdiff_t stride, const void *left, const void *lpf, int w, int h, const void *params,
                     int edges, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !p || !params || !lr_dims_ok(w, h) || edges < 0 || edges > 15) return -EINVAL;
    Call c;
    int16_t f[2][8];
    c.peek(f, params, sizeof(f));
    if (c.err) return c.err;
    mi::LrCallArgs a;
    memset(&a, 0, sizeof(a));
    a.tp.wiener = true;
    for (int k = 0; k < 7; k++) { a.tp.fh[k] = f[0][k]; a.tp.fv[k] = f[1][k]; }
    if (bpc == 8) a.tp.fh[3] += 128;   // the reference adds the 8-bit centre tap separately
    return lr_call(c, a, p, stride, left, lpf, w, h, edges, bpc);
}

int mi_dsp_lr_sgr(int kind, void *p, ptrdiff_t stride, const void *left, const void *lpf, int w, int h,
                  const void *params, int edges, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || kind < 0 || kind > 2 || !p || !params || !lr_dims_ok(w, h) || edges < 0 || edges > 15) return -EINVAL;
    Call c;
    struct { uint32_t s0, s1; int16_t w0, w1; } sp;   // LooprestorationParams_sgr
    c.peek(&sp, params, sizeof(sp));
    if (c.err) return c.err;
    mi::LrCallArgs a;
    memset(&a, 0, sizeof(a));
    a.tp.wiener = false;
    a.tp.s0 = kind != 1 ? (int)sp.s0 : 0;
    a.tp.s1 = kind != 0 ? (int)sp.s1 : 0;
    a.tp.w0 = sp.w0;
    a.tp.w1 = sp.w1;
    if ((kind != 1 && !a.tp.s0) || (kind != 0 && !a.tp.s1)) return -EINVAL;
    return lr_call(c, a, p, stride, left, lpf, w, h, edges, bpc);
}

// ---- film-grain table (src/filmgrain.rs:41-198): generate_grain_y / _uv, fgy / fguv_32x32xn ----
namespace {
constexpr int kGW = 82, kGH = 73, kGP = 88;   // template width / height, device pitch (fg.hip)
constexpr size_t kFgLutB = 3 * kGH * kGP * 2, kFgSclB = 3 * 4096;

// the entry's turn, the constant tables and the caller's parameters: what every fg entry starts with
int fg_begin(Call &c, mi::FgArgs &a, const MiFilmGrainData *data) {
    if (c.err) return c.err;
    if (int e = mi_internal::fg_tables()) return e;
    memset(&a, 0, sizeof(a));
    c.peek(&a.data, data, sizeof(a.data));
    if (c.err) return c.err;
    return mi_internal::fg_data_ok(&a.data) ? 0 : -EINVAL;
}
// caller's GrainLut<Entry> rows (82 entries: int8 at 8 bits, int16 above) <-> int16 [73][82]
int fg_lut_read(Call &c, int16_t *t, const void *buf, int bpc) {
    if (bpc == 8) {
        int8_t b[kGH * kGW];
        c.peek(b, buf, sizeof(b));
        for (int i = 0; i < kGH * kGW && !c.err; i++) t[i] = b[i];
    } else {
        c.peek(t, buf, kGH * kGW * 2);
    }
    return c.err;
}
int fg_lut_write(void *buf, const int16_t *t, int bpc) {
    if (bpc == 8) {
        int8_t b[kGH * kGW];
        for (int i = 0; i < kGH * kGW; i++) b[i] = (int8_t)t[i];
        return hipMemcpy(buf, b, sizeof(b), hipMemcpyDefault) == hipSuccess ? 0 : -EIO;
    }
    return hipMemcpy(buf, t, kGH * kGW * 2, hipMemcpyDefault) == hipSuccess ? 0 : -EIO;
}
// run the template generator and fetch plane pl's template into t [73][82]
int fg_generate(Call &c, mi::FgArgs &a, int pl, int16_t *t) {
    a.lut = (int16_t *)c.take(kFgLutB);
    a.scaling = c.take(kFgSclB);
    if (c.err) return c.err;
    if (mi::launch_fg(a, c.stream, true, false)) return -EIO;
    static int16_t dev[kGH * kGP];
    if (int e = c.result(dev, a.lut + pl * kGH * kGP, sizeof(dev))) return e;
    for (int r = 0; r < kGH; r++) memcpy(t + r * kGW, dev + r * kGP, kGW * 2);
    return 0;
}
// the caller's template -> device slot pl (pitch 88)
int fg_lut_in(Call &c, int16_t *dlut, int pl, const void *grain_lut, int bpc) {
    static int16_t t[kGH * kGW], dev[kGH * kGP];
    if (int e = fg_lut_read(c, t, grain_lut, bpc)) return e;
    memset(dev, 0, sizeof(dev));
    for (int r = 0; r < kGH; r++) memcpy(dev + r * kGP, t + r * kGW, kGW * 2);
    c.copy_in(dlut + pl * kGH * kGP, dev, sizeof(dev));
    return c.finish();   // dev is reused
}
int layout_ok(int layout) { return layout >= 1 && layout <= 3; }

// fgy (plane 0) / fguv (plane 1 + uv): one 32-row strip through the frame apply kernel
int fg_strip(int pl, int layout, void *dst_row, const void *src_row, ptrdiff_t stride, const MiFilmGrainData *data,
             size_t pw, const uint8_t *scaling, const void *grain_lut, int bh, int row_num, const void *luma_row,
             ptrdiff_t luma_stride, int is_id, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    const int sx = pl && layout != 3, sy = pl && layout == 1;
    if (!bpc || !dst_row || !src_row || !data || !scaling || !grain_lut || (pl && (!luma_row || !layout_ok(layout))) ||
        pw < 1 || pw > 8192 || bh < 1 || bh > (32 >> sy) || row_num < 0)
        return -EINVAL;
    Call c;
    mi::FgArgs a;
    if (int e = fg_begin(c, a, data)) return e;
    const int px = bpc == 8 ? 1 : 2;
    const size_t lw = pw << sx;
    const int lrows = pl ? ((bh - 1) << sy) + 1 : 0;
    const int nblocks = (int)((pw + (32 >> sx) - 1) / (32 >> sx));
    // a row can be 8192 px wide: the one entry that may need more than the scratch holds
    const ptrdiff_t P = (ptrdiff_t)((pw * px + 255) & ~(size_t)255), LP = (ptrdiff_t)((lw * px + 255) & ~(size_t)255);
    if (int e = c.reserve({kFgLutB, kFgSclB, 2 * (size_t)nblocks, (size_t)P * bh, (size_t)LP * lrows})) return e;
    a.lut = (int16_t *)c.take(kFgLutB);
    a.scaling = c.take(kFgSclB);
    a.offsets = c.take(2 * (size_t)nblocks);
    const Win pix = c.win(0, bh, 0, P), luma = c.win(0, lrows, 0, LP);
    if (c.err) return c.err;
    if (int e = fg_lut_in(c, a.lut, pl, grain_lut, bpc)) return e;
    c.copy_in(a.scaling + pl * 4096, scaling, (size_t)1 << bpc);
    if (pl) c.copy_in(a.scaling, scaling, (size_t)1 << bpc);   // the slot read under chroma_scaling_from_luma
    for (int r = 0; r < bh; r++) c.copy_in(pix.dev + r * P, (const uint8_t *)src_row + r * stride, pw * px);
    for (int y = 0; pl && y < bh; y++)
        c.copy_in(luma.dev + (size_t)(y << sy) * LP, (const uint8_t *)luma_row + (y << sy) * luma_stride, lw * px);
    if (c.err) return c.err;
    a.bpc = bpc;
    a.layout = pl ? layout : 0;
    a.ss_x = sx;
    a.ss_y = sy;
    a.w = (int)lw;
    a.h = bh << sy;
    a.is_id = is_id;
    const bool prev = a.data.overlap_flag && row_num > 0;
    a.nrows = prev ? 2 : 1;
    a.row0 = prev ? row_num - 1 : row_num;
    a.row_off = prev ? 1 : 0;
    a.nblocks = nblocks;
    a.src[0] = pl ? luma.dev : pix.dev;
    a.stride[0] = pl ? LP : P;
    a.src[pl] = pix.dev;
    a.dst[pl] = pix.dev;
    a.stride[pl] = P;
    a.pw[pl] = (int)pw;
    a.ph[pl] = bh;
    a.chunks[pl] = (int)((pw + 511) / 512);
    a.grain[pl] = 1;
    const int nb = (a.chunks[pl] * bh + 4 * mi::kFgItems - 1) / (4 * mi::kFgItems);
    for (int q = 0; q < 4; q++) a.blk_start[q] = q <= pl ? 0 : nb;
    if (mi::launch_fg_call(a, c.stream)) return -EIO;
    for (int r = 0; r < bh; r++) c.copy_out((uint8_t *)dst_row + r * stride, pix.dev + r * P, pw * px);
    return c.finish();
}
}  // namespace

int mi_dsp_fg_generate_grain_y(void *buf, const MiFilmGrainData *data, int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !buf || !data) return -EINVAL;
    Call c;
    mi::FgArgs a;
    if (int e = fg_begin(c, a, data)) return e;
    a.bpc = bpc;
    static int16_t t[kGH * kGW];
    if (int e = fg_generate(c, a, 0, t)) return e;
    return fg_lut_write(buf, t, bpc);
}

int mi_dsp_fg_generate_grain_uv(int layout, void *buf, const void *buf_y, const MiFilmGrainData *data, int uv,
                                int bitdepth_max) {
    const int bpc = bpc_of(bitdepth_max);
    if (!bpc || !layout_ok(layout) || !buf || !buf_y || !data || uv < 0 || uv > 1) return -EINVAL;
    Call c;
    mi::FgArgs a;
    if (int e = fg_begin(c, a, data)) return e;
    static int16_t ty[kGH * kGW], t[kGH * kGW], out[kGH * kGW];
    if (int e = fg_lut_read(c, ty, buf_y, bpc)) return e;
    int16_t *dly = (int16_t *)c.stage(ty, sizeof(ty));
    a.bpc = bpc;
    a.layout = layout;
    a.ss_x = layout != 3;
    a.ss_y = layout == 1;
    a.lut_y = dly;
    a.uv_only = 1 + uv;
    if (int e = fg_generate(c, a, 1 + uv, t)) return e;
    // only the chroma template's own cw x chh corner is written, as the reference does
    if (int e = fg_lut_read(c, out, buf, bpc)) return e;
    const int cw = a.ss_x ? 44 : kGW, chh = a.ss_y ? 38 : kGH;
    for (int r = 0; r < chh; r++) memcpy(out + r * kGW, t + r * kGW, cw * 2);
    return fg_lut_write(buf, out, bpc);
}

int mi_dsp_fgy_32x32xn(void *dst_row, const void *src_row, ptrdiff_t stride, const MiFilmGrainData *data, size_t pw,
                       const uint8_t *scaling, const void *grain_lut, int bh, int row_num, int bitdepth_max) {
    return fg_strip(0, 0, dst_row, src_row, stride, data, pw, scaling, grain_lut, bh, row_num, nullptr, 0, 0,
                    bitdepth_max);
}

int mi_dsp_fguv_32x32xn(int layout, void *dst_row, const void *src_row, ptrdiff_t stride,
                        const MiFilmGrainData *data, size_t pw, const uint8_t *scaling, const void *grain_lut, int bh,
                        int row_num, const void *luma_row, ptrdiff_t luma_stride, int uv_pl, int is_id,
                        int bitdepth_max) {
    if (uv_pl < 0 || uv_pl > 1) return -EINVAL;
    return fg_strip(1 + uv_pl, layout, dst_row, src_row, stride, data, pw, scaling, grain_lut, bh, row_num, luma_row,
                    luma_stride, is_id, bitdepth_max);
}

}  // extern "C"
