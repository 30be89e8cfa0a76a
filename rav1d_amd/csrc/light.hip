// light.hip — mi_picture_light_level (include/mi_av1out.h): the histogram of max(R', G', B') over
// the planar R'G'B' picture mi_display_picture would write for the same source, without writing
// that picture. The front of a lane is display_kernel's (display.h: load_run, upsample,
// convert_run over 8 luma columns of one row unit); the new work is the counting.
//
// One workgroup (64 x 4 lanes) owns a histogram of 1 << bpc bins in LDS (16 KB at 12 bits). It
// walks tiles of 512 columns x 4 row units down the picture with a stride of gridDim.y tiles, so
// the number of workgroups, and with it the global atomics of the flush, is bounded whatever the
// picture's size (kLightBlocks: no more than are resident at once, and the tiles split evenly
// between them; DESIGN.md has what the other splits cost). The flush adds the non-zero bins to
// `hist` with one atomicAdd per bin per workgroup.
//
// Counting. The case that decides it is a flat picture (bars, a black frame, a test card): every
// lane of a wave then hits one bin and LDS atomics on one address serialise. Three variants are
// kept behind a template switch so that tools/light_bench.py can measure them; the entry uses
// kLightShipped:
//   0: one LDS atomic per pixel;
//   1: equal neighbours of a lane's run (8 pixels, 16 for 4:2:0's row pair) combined first;
//   2: as 1, and when every pixel of the wave's tile row has the same value (a ballot), the
//      counts are summed across the wave and one lane adds them.
#include <cerrno>
#include <cstring>

#include "display.h"

namespace mi {
namespace {

constexpr int kLightBlocks = 1024;   // workgroups of a call at most: the four per CU that are resident at once
constexpr int kLightShipped = 2;

// The lane's values counted into the workgroup's histogram: v[0 .. n0) is the first row's run,
// v[8 .. 8 + n1) the second's. Every lane of a wave calls it (MODE 2 votes across the wave).
template <int MODE>
__device__ __forceinline__ void count_run(uint32_t *h, const int (&v)[16], int n0, int n1) {
    if constexpr (MODE == 0) {
#pragma unroll
        for (int k = 0; k < 16; k++)
            if ((k < 8 && k < n0) || (k >= 8 && k - 8 < n1)) atomicAdd(&h[v[k]], 1u);
    } else {
        if constexpr (MODE == 2) {
            // wave-uniform content: one add per wave. A lane without pixels agrees with anything.
            const int mine = n0 ? v[0] : n1 ? v[8] : -1;
            const unsigned long long have = __ballot(mine >= 0);
            if (have) {
                const int first = __shfl(mine, __ffsll((long long)have) - 1);
                bool same = true;
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if ((k < 8 && k < n0) || (k >= 8 && k - 8 < n1)) same &= v[k] == first;
                if (__all(same)) {
                    int c = n0 + n1;
#pragma unroll
                    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
                    if (threadIdx.x == 0) atomicAdd(&h[first], (uint32_t)c);
                    return;
                }
            }
        }
        int cur = -1;
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if ((k < 8 && k < n0) || (k >= 8 && k - 8 < n1)) {
                if (v[k] == cur) {
                    cnt++;
                } else {
                    if (cnt) atomicAdd(&h[cur], cnt);
                    cur = v[k];
                    cnt = 1;
                }
            }
        }
        if (cnt) atomicAdd(&h[cur], cnt);
    }
}

template <typename Px, int MODE>
__global__ __launch_bounds__(256) void light_kernel(const DisplayArgs a, uint32_t *__restrict__ hist, int nbins) {
    __shared__ uint32_t h[4096];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int i = tid; i < nbins; i += 256) h[i] = 0;
    __syncthreads();
    const int cx = blockIdx.x * 64 + threadIdx.x, x0 = cx * 8, nrows = 1 + a.ss_ver;
    // (every lane walks the same number of tiles: the wave-level steps of count_run need the
    // whole wave, and the barrier below the whole workgroup)
    for (int ub = blockIdx.y * 4; ub < a.units; ub += gridDim.y * 4) {
        const int u = ub + threadIdx.y;
        int n0 = 0, n1 = 0;
        int m[16];
#pragma unroll
        for (int k = 0; k < 16; k++) m[k] = 0;
        if (cx < a.chunks && u < a.units) {
            const int r0 = u * nrows;
            int y[2][8];
            load_run<Px, 8>(a.src[0] + r0 * a.sstride[0], x0, a.w, a.svec & 1, y[0]);
            if (a.ss_ver) {
                load_run<Px, 8>(a.src[0] + min(r0 + 1, a.h - 1) * a.sstride[0], x0, a.w, a.svec & 1, y[1]);
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++) y[1][k] = y[0][k];   // (not used)
            }
            int cu[2][8] = {}, cv[2][8] = {};
            if (!a.mono) {
                upsample<Px>(a, 1, u, x0, cu);
                upsample<Px>(a, 2, u, x0, cv);
            }
            n0 = min(8, a.w - x0);
            n1 = a.ss_ver && r0 + 1 < a.h ? n0 : 0;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                int R[8], G[8], B[8];
                convert_run(a, y[r], cu[r], cv[r], R, G, B);
                // (the matrix clips to [0, M]; the identity hands samples on: the min keeps the
                // index inside the histogram whatever the planes hold)
#pragma unroll
                for (int k = 0; k < 8; k++) m[8 * r + k] = min(max(max(R[k], G[k]), B[k]), a.maxv);
            }
        }
        count_run<MODE>(h, m, n0, n1);
    }
    __syncthreads();
    for (int i = tid; i < nbins; i += 256) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

template <typename Px>
int launch_light(const DisplayArgs &a, uint32_t *hist, int nbins, int mode, hipStream_t s) {
    const int gx = (a.chunks + 63) / 64, tiles = (a.units + 3) / 4;
    // at most kLightBlocks workgroups, each with the same number of tiles (but for the ragged end)
    const int per_col = kLightBlocks / gx > 0 ? kLightBlocks / gx : 1;
    const int passes = (tiles + per_col - 1) / per_col, gy = (tiles + passes - 1) / passes;
    const dim3 block(64, 4), grid(gx, gy);
    switch (mode) {
    case 0: light_kernel<Px, 0><<<grid, block, 0, s>>>(a, hist, nbins); break;
    case 1: light_kernel<Px, 1><<<grid, block, 0, s>>>(a, hist, nbins); break;
    default: light_kernel<Px, 2><<<grid, block, 0, s>>>(a, hist, nbins); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int light_level(MiCtx *ctx, const MiPicture *in, const MiColorInfo *color, uint32_t *hist, int mode, void *stream) {
    if (!in || !hist) return -EINVAL;
    if (int e = display_check_picture(in)) return e;
    if (int e = display_check_strides(in)) return e;
    if ((int64_t)in->w * in->h >= (int64_t)1 << 32) return -EINVAL;   // (a bin holds a picture's pixels)
    DisplayArgs a;
    memset(&a, 0, sizeof(a));
    if (int e = display_color(in, color, a)) return e;
    if (mode < 0 || mode > 2) return -EINVAL;
    if (!ctx) return -EINVAL;

    display_source(*in, color, a);
    a.chunks = (in->w + 7) >> 3;
    a.units = in->layout == 1 ? a.ch : in->h;
    const int nbins = 1 << in->bpc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)nbins * sizeof(uint32_t), s) != hipSuccess) return ctx->last_error = -EIO;
    if (in->bpc == 8 ? launch_light<uint8_t>(a, hist, nbins, mode, s) : launch_light<uint16_t>(a, hist, nbins, mode, s))
        return ctx->last_error = -EIO;
    return 0;
}

}  // namespace
}  // namespace mi

extern "C" int mi_picture_light_level(MiCtx *ctx, const MiPicture *in, const MiColorInfo *color, uint32_t *hist,
                                      void *stream) {
    return mi::light_level(ctx, in, color, hist, mi::kLightShipped, stream);
}

extern "C" int mi_picture_light_level_variant(MiCtx *ctx, const MiPicture *in, const MiColorInfo *color, uint32_t *hist,
                                              int variant, void *stream) {
    return mi::light_level(ctx, in, color, hist, variant, stream);
}
