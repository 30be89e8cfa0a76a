/*
 * oracle/loopfilter.c — CPU restatement of the deblocking filter (TEST INFRASTRUCTURE ONLY).
 *
 * Follows FreezyLemon/rav1d:
 *   src/loopfilter.rs:396-721   loop_filter (C src/loopfilter_tmpl.c:37-160)
 *   src/loopfilter.rs:745-985   loop_filter_{h,v}_sb128{y,uv} (C loopfilter_tmpl.c:162-250)
 *   src/lf_apply.rs:388-834     filter_plane_{cols,rows}_{y,uv}, rav1d_loopfilter_sbrow_{cols,rows}
 *                               (C src/lf_apply_tmpl.c:174-466)
 * The frame driver walks superblock rows in the reference's order (columns then rows per
 * sbrow, src/recon.rs:4319-4338). Tile-boundary mask fixups (lf_apply.rs:625-705) are a
 * property of the input masks here: callers pass masks with the fixups already applied.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "oracle.h"
#include "census.h"

/* The reference's comparisons, each with the number of the mutant that weakens it. In the
 * plain build MUT() is the constant 0 and these are the bare operators. */
#define LE(a, b, c) (MUT(MUT_LF_LT + (c)) ? (a) < (b) : (a) <= (b))
#define GT(a, b, m) (MUT(m) ? (a) >= (b) : (a) > (b))
#define SUM8(x) (MUT(MUT_LF_SUM8_I16) ? (int)(int16_t)(x) : (x))
#define SUM16(x) (MUT(MUT_LF_SUM16_I16) ? (int)(int16_t)(x) : (x))

static inline int imin(int a, int b) { return a < b ? a : b; }
static inline int imax(int a, int b) { return a > b ? a : b; }
static inline int iclip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

typedef struct {
    int hbd, bdmax, bdm8;
} Px;

static inline int rd(const Px *px, const uint8_t *base, ptrdiff_t off)
{
    return px->hbd ? ((const uint16_t *)base)[off] : base[off];
}
static inline void wr(const Px *px, uint8_t *base, ptrdiff_t off, int v)
{
    if (px->hbd) ((uint16_t *)base)[off] = (uint16_t)v;
    else base[off] = (uint8_t)v;
}

#ifdef ORACLE_CENSUS
uint64_t oracle_census_ctr[CEN_COUNT];
int oracle_census_mutant;
void oracle_census_reset(void) { memset(oracle_census_ctr, 0, sizeof(oracle_census_ctr)); }
int oracle_census_read(uint64_t *out, int n)
{
    if (n > CEN_COUNT) n = CEN_COUNT;
    memcpy(out, oracle_census_ctr, (size_t)n * sizeof(*out));
    return CEN_COUNT;
}
void oracle_census_set_mutant(int m) { oracle_census_mutant = m; }
/* index of the first counter of a group, so that the binding need not repeat the layout */
int oracle_census_layout(int what)
{
    static const int v[] = {
        CEN_COUNT, MUT_COUNT, LF_NCELL, LF_CELL_SIZE, LF_NBR, LF_NCMP, LF_NCLIP, LF_CELL_BRANCH,
        LF_CELL_AT, LF_CELL_AT1, LF_CELL_PIN_LO, LF_CELL_PIN_HI, LF_CELL_CLIP, LF_CELL_PAIR,
        CEN_LF, CEN_CDEF_TIES, CEN_CDEF_WIN, CEN_CDEF_WIN_SUBTIE, CEN_CDEF_VAR0, CEN_CDEF_PX_BOTH,
        CEN_CDEF_PX_CLAMPED, CEN_CDEF_PX_SENTINEL, CEN_CDEF_PX_PRISHIFT0, CEN_CDEF_PX_NEG,
        CEN_CDEF_PX_OUT0, CEN_CDEF_PX_OUTMAX, CEN_WIENER_HCLIP_LO, CEN_WIENER_HCLIP_HI,
        CEN_WIENER_VCLIP_LO, CEN_WIENER_VCLIP_HI, CEN_SGR_Z0, CEN_SGR_Z255, CEN_SGR_PS31,
        CEN_SGR_XSUM31, CEN_SGR_OUT_LO, CEN_SGR_OUT_HI, CEN_LR_SET, CEN_LR_WIENER,
        CEN_ITX_ROW_CLIP_LO, CEN_ITX_ROW_CLIP_HI, CEN_ITX_COL_CLIP_LO, CEN_ITX_COL_CLIP_HI,
        CEN_ITX_MID_CLIP_LO, CEN_ITX_MID_CLIP_HI, CEN_ITX_PX_CLIP_0, CEN_ITX_PX_CLIP_MAX,
        CEN_ITX_RES_GT_I16, CEN_ITX_WHT_MID_GT_I16, CEN_ITX_ROT_GE_2P31,
        MUT_ITX_ROT_I32, MUT_ITX_NO_CLIP, MUT_ITX_NO_MIDCLIP, MUT_ITX_MID_I16, MUT_ITX_RES_I16,
        MUT_ITX_WHT_MID_I16,
    };
    return what >= 0 && what < (int)(sizeof(v) / sizeof(v[0])) ? v[what] : -1;
}

static int lf_cell;   /* set by oracle_lf_sb: ((dir * 2 + cls) * 4 + width index) */

/* Which comparisons decide this line's branch while sitting at their limit or one past it.
 * A comparison decides when every other comparison of its conjunction holds (for the two
 * hev tests, which are or-ed: when the other one fails), so that weakening it alone changes
 * the branch. s[0..6] = p0..p6, s[7..13] = q0..q6; unmutated arithmetic throughout. */
static int lf_census_line(const int *s, int wd, int E, int I, int H, int F, int bdmax)
{
    uint64_t *cell = &oracle_census_ctr[CEN_LF + lf_cell * LF_CELL_SIZE];
    const int *p = s, *q = s + 7;
    int dist[LF_NCMP], lim[LF_NCMP], on[LF_NCMP] = { 0 };
#define SET(c, d, l) (dist[c] = (d), lim[c] = (l), on[c] = 1)
    SET(LF_CMP_I_P1P0, abs(p[1] - p[0]), I);
    SET(LF_CMP_I_Q1Q0, abs(q[1] - q[0]), I);
    SET(LF_CMP_E, abs(p[0] - q[0]) * 2 + (abs(p[1] - q[1]) >> 1), E);
    if (wd > 4) {
        SET(LF_CMP_I_P2P1, abs(p[2] - p[1]), I);
        SET(LF_CMP_I_Q2Q1, abs(q[2] - q[1]), I);
        SET(LF_CMP_FI_P2, abs(p[2] - p[0]), F);
        SET(LF_CMP_FI_P1, abs(p[1] - p[0]), F);
        SET(LF_CMP_FI_Q1, abs(q[1] - q[0]), F);
        SET(LF_CMP_FI_Q2, abs(q[2] - q[0]), F);
    }
    if (wd > 6) {
        SET(LF_CMP_I_P3P2, abs(p[3] - p[2]), I);
        SET(LF_CMP_I_Q3Q2, abs(q[3] - q[2]), I);
        SET(LF_CMP_FI_P3, abs(p[3] - p[0]), F);
        SET(LF_CMP_FI_Q3, abs(q[3] - q[0]), F);
    }
    if (wd >= 16) {
        SET(LF_CMP_FO_P6, abs(p[6] - p[0]), F);
        SET(LF_CMP_FO_P5, abs(p[5] - p[0]), F);
        SET(LF_CMP_FO_P4, abs(p[4] - p[0]), F);
        SET(LF_CMP_FO_Q4, abs(q[4] - q[0]), F);
        SET(LF_CMP_FO_Q5, abs(q[5] - q[0]), F);
        SET(LF_CMP_FO_Q6, abs(q[6] - q[0]), F);
    }
    SET(LF_CMP_H_P, abs(p[1] - p[0]), H);
    SET(LF_CMP_H_Q, abs(q[1] - q[0]), H);
#undef SET
    /* the three conjunctions: fm (I and E tests), inner flat, outer flat */
    static const uint8_t grp[LF_NCMP] = { 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 3, 3 };
    int fails[3] = { 0, 0, 0 };
    for (int c = 0; c < LF_CMP_H_P; c++)
        if (on[c] && dist[c] > lim[c]) fails[grp[c]]++;
    const int fm = !fails[0], fin = wd >= 6 && !fails[1], fout = wd >= 16 && !fails[2];
    int br;
    if (!fm) br = LF_BR_NONE;
    else if (fin && fout) br = LF_BR_13TAP;
    else if (fin) br = wd == 6 ? LF_BR_6TAP : LF_BR_8TAP;
    else br = dist[LF_CMP_H_P] > H || dist[LF_CMP_H_Q] > H ? LF_BR_NARROW_HEV : LF_BR_NARROW;
    for (int c = 0; c < LF_NCMP; c++) {
        if (!on[c]) continue;
        int decides;
        const int others = fails[grp[c] < 3 ? grp[c] : 0] - (grp[c] < 3 && dist[c] > lim[c]);
        if (grp[c] == 0) decides = !others;
        else if (grp[c] == 1) decides = fm && !others;
        else if (grp[c] == 2) decides = fm && fin && !others;
        else decides = fm && !fin && dist[c == LF_CMP_H_P ? LF_CMP_H_Q : LF_CMP_H_P] <= H;
        if (!decides) continue;
        if (dist[c] == lim[c]) cell[LF_CELL_AT + c]++;
        if (dist[c] == lim[c] + 1) cell[LF_CELL_AT1 + c]++;
    }
    if (br >= LF_BR_6TAP) {
        const int n = br == LF_BR_6TAP ? 3 : br == LF_BR_8TAP ? 4 : 7;
        int lo = 1, hi = 1;
        for (int k = 0; k < n; k++) {
            lo &= p[k] <= F && q[k] <= F;
            hi &= p[k] >= bdmax - F && q[k] >= bdmax - F;
        }
        cell[LF_CELL_PIN_LO + br] += lo;
        cell[LF_CELL_PIN_HI + br] += hi;
    }
    cell[LF_CELL_BRANCH + br]++;
    return br;
}
#define LF_CLIP(c, i) CEN_IF(c, CEN_LF + lf_cell * LF_CELL_SIZE + LF_CELL_CLIP + (i))
#else
#define LF_CLIP(c, i) ((void)0)
#endif

/* One 4-line edge segment. `dst` points at q0 of line 0; sa steps between lines, sb across
 * the edge (both in pixels). wd in {4, 6, 8, 16}. loopfilter.rs:396-721. */
static void filter4lines(const Px *px, uint8_t *dst, int E, int I, int H, ptrdiff_t sa,
                         ptrdiff_t sb, int wd)
{
    const int F = 1 << px->bdm8;
    E <<= px->bdm8;
    I <<= px->bdm8;
    H <<= px->bdm8;
    const int dlo = -128 * (1 << px->bdm8), dhi = 128 * (1 << px->bdm8) - 1;
    const int fmax = (128 << px->bdm8) - 1;

    CEN_ONLY(int prev_br = 0;)
    for (int i = 0; i < 4; i++) {
        const ptrdiff_t o = i * sa;
#define P(k) rd(px, dst, o - (k + 1) * sb)
#define Q(k) rd(px, dst, o + (k) * sb)
#define SP(k, v) wr(px, dst, o - (k + 1) * sb, v)
#define SQ(k, v) wr(px, dst, o + (k) * sb, v)
        const int p1 = P(1), p0 = P(0), q0 = Q(0), q1 = Q(1);
        int p2 = 0, p3 = 0, q2 = 0, q3 = 0, p4 = 0, p5 = 0, p6 = 0, q4 = 0, q5 = 0, q6 = 0;
        int fm = LE(abs(p1 - p0), I, LF_CMP_I_P1P0) && LE(abs(q1 - q0), I, LF_CMP_I_Q1Q0) &&
                 LE(abs(p0 - q0) * 2 + (abs(p1 - q1) >> 1), E, LF_CMP_E);
        if (wd > 4) {
            p2 = P(2); q2 = Q(2);
            fm &= LE(abs(p2 - p1), I, LF_CMP_I_P2P1) && LE(abs(q2 - q1), I, LF_CMP_I_Q2Q1);
            if (wd > 6) {
                p3 = P(3); q3 = Q(3);
                fm &= LE(abs(p3 - p2), I, LF_CMP_I_P3P2) && LE(abs(q3 - q2), I, LF_CMP_I_Q3Q2);
            }
        }
        CEN_ONLY(
            const int smp[14] = { p0, p1, p2, p3, wd >= 16 ? P(4) : 0, wd >= 16 ? P(5) : 0,
                                  wd >= 16 ? P(6) : 0, q0, q1, q2, q3, wd >= 16 ? Q(4) : 0,
                                  wd >= 16 ? Q(5) : 0, wd >= 16 ? Q(6) : 0 };
            const int br = lf_census_line(smp, wd, E, I, H, F, px->bdmax);
            if (i & 1) {
                const int a = br < prev_br ? br : prev_br, b = br < prev_br ? prev_br : br;
                CEN(CEN_LF + lf_cell * LF_CELL_SIZE + LF_CELL_PAIR + a * LF_NBR + b);
            }
            prev_br = br;
        )
        if (!fm) continue;

        int flat8out = 0, flat8in = 0;
        if (wd >= 16) {
            p6 = P(6); p5 = P(5); p4 = P(4);
            q4 = Q(4); q5 = Q(5); q6 = Q(6);
            flat8out = LE(abs(p6 - p0), F, LF_CMP_FO_P6) && LE(abs(p5 - p0), F, LF_CMP_FO_P5) &&
                       LE(abs(p4 - p0), F, LF_CMP_FO_P4) && LE(abs(q4 - q0), F, LF_CMP_FO_Q4) &&
                       LE(abs(q5 - q0), F, LF_CMP_FO_Q5) && LE(abs(q6 - q0), F, LF_CMP_FO_Q6);
        }
        if (wd >= 6)
            flat8in = LE(abs(p2 - p0), F, LF_CMP_FI_P2) && LE(abs(p1 - p0), F, LF_CMP_FI_P1) &&
                      LE(abs(q1 - q0), F, LF_CMP_FI_Q1) && LE(abs(q2 - q0), F, LF_CMP_FI_Q2);
        if (wd >= 8)
            flat8in &= LE(abs(p3 - p0), F, LF_CMP_FI_P3) && LE(abs(q3 - q0), F, LF_CMP_FI_Q3);

        if (wd >= 16 && flat8out && flat8in) {
            SP(5, (SUM16(p6 * 7 + p5 * 2 + p4 * 2 + p3 + p2 + p1 + p0 + q0 + 8) >> 4));
            SP(4, (SUM16(p6 * 5 + p5 * 2 + p4 * 2 + p3 * 2 + p2 + p1 + p0 + q0 + q1 + 8) >> 4));
            SP(3, (SUM16(p6 * 4 + p5 + p4 * 2 + p3 * 2 + p2 * 2 + p1 + p0 + q0 + q1 + q2 + 8) >> 4));
            SP(2, (SUM16(p6 * 3 + p5 + p4 + p3 * 2 + p2 * 2 + p1 * 2 + p0 + q0 + q1 + q2 + q3 + 8) >> 4));
            SP(1, (SUM16(p6 * 2 + p5 + p4 + p3 + p2 * 2 + p1 * 2 + p0 * 2 + q0 + q1 + q2 + q3 + q4 + 8) >> 4));
            SP(0, (SUM16(p6 + p5 + p4 + p3 + p2 + p1 * 2 + p0 * 2 + q0 * 2 + q1 + q2 + q3 + q4 + q5 + 8) >> 4));
            SQ(0, (SUM16(p5 + p4 + p3 + p2 + p1 + p0 * 2 + q0 * 2 + q1 * 2 + q2 + q3 + q4 + q5 + q6 + 8) >> 4));
            SQ(1, (SUM16(p4 + p3 + p2 + p1 + p0 + q0 * 2 + q1 * 2 + q2 * 2 + q3 + q4 + q5 + q6 * 2 + 8) >> 4));
            SQ(2, (SUM16(p3 + p2 + p1 + p0 + q0 + q1 * 2 + q2 * 2 + q3 * 2 + q4 + q5 + q6 * 3 + 8) >> 4));
            SQ(3, (SUM16(p2 + p1 + p0 + q0 + q1 + q2 * 2 + q3 * 2 + q4 * 2 + q5 + q6 * 4 + 8) >> 4));
            SQ(4, (SUM16(p1 + p0 + q0 + q1 + q2 + q3 * 2 + q4 * 2 + q5 * 2 + q6 * 5 + 8) >> 4));
            SQ(5, (SUM16(p0 + q0 + q1 + q2 + q3 + q4 * 2 + q5 * 2 + q6 * 7 + 8) >> 4));
        } else if (wd >= 8 && flat8in) {
            SP(2, (SUM8(p3 * 3 + p2 * 2 + p1 + p0 + q0 + 4) >> 3));
            SP(1, (SUM8(p3 * 2 + p2 + p1 * 2 + p0 + q0 + q1 + 4) >> 3));
            SP(0, (SUM8(p3 + p2 + p1 + p0 * 2 + q0 + q1 + q2 + 4) >> 3));
            SQ(0, (SUM8(p2 + p1 + p0 + q0 * 2 + q1 + q2 + q3 + 4) >> 3));
            SQ(1, (SUM8(p1 + p0 + q0 + q1 * 2 + q2 + q3 * 2 + 4) >> 3));
            SQ(2, (SUM8(p0 + q0 + q1 + q2 * 2 + q3 * 3 + 4) >> 3));
        } else if (wd == 6 && flat8in) {
            SP(1, (p2 * 3 + p1 * 2 + p0 * 2 + q0 + 4) >> 3);
            SP(0, (p2 + p1 * 2 + p0 * 2 + q0 * 2 + q1 + 4) >> 3);
            SQ(0, (p1 + p0 * 2 + q0 * 2 + q1 * 2 + q2 + 4) >> 3);
            SQ(1, (p0 + q0 * 2 + q1 * 2 + q2 * 3 + 4) >> 3);
        } else {
            const int hev = GT(abs(p1 - p0), H, MUT_LF_HEV_GE_P) || GT(abs(q1 - q0), H, MUT_LF_HEV_GE_Q);
            int f, f1, f2;
            if (hev) {
                LF_CLIP(p1 - q1 <= dlo, LF_CLIP_D_LO);
                LF_CLIP(p1 - q1 >= dhi, LF_CLIP_D_HI);
                f = iclip(p1 - q1, dlo, dhi);
                f = iclip(3 * (q0 - p0) + f, dlo, dhi);
                LF_CLIP(f == dlo, LF_CLIP_F_LO);
                LF_CLIP(f == dhi, LF_CLIP_F_HI);
                LF_CLIP(f + 4 > fmax, LF_CLIP_F4_MAX);
                LF_CLIP(f + 3 > fmax, LF_CLIP_F3_MAX);
                f1 = imin(f + 4, fmax) >> 3;
                f2 = imin(f + 3, fmax) >> 3;
                LF_CLIP(p0 + f2 < 0 || q0 - f1 < 0, LF_CLIP_OUT_LO);
                LF_CLIP(p0 + f2 > px->bdmax || q0 - f1 > px->bdmax, LF_CLIP_OUT_HI);
                SP(0, iclip(p0 + f2, 0, px->bdmax));
                SQ(0, iclip(q0 - f1, 0, px->bdmax));
            } else {
                f = iclip(3 * (q0 - p0), dlo, dhi);
                LF_CLIP(f == dlo, LF_CLIP_F_LO);
                LF_CLIP(f == dhi, LF_CLIP_F_HI);
                LF_CLIP(f + 4 > fmax, LF_CLIP_F4_MAX);
                LF_CLIP(f + 3 > fmax, LF_CLIP_F3_MAX);
                f1 = imin(f + 4, fmax) >> 3;
                f2 = imin(f + 3, fmax) >> 3;
                LF_CLIP(p0 + f2 < 0 || q0 - f1 < 0, LF_CLIP_OUT_LO);
                LF_CLIP(p0 + f2 > px->bdmax || q0 - f1 > px->bdmax, LF_CLIP_OUT_HI);
                SP(0, iclip(p0 + f2, 0, px->bdmax));
                SQ(0, iclip(q0 - f1, 0, px->bdmax));
                f = (f1 + 1) >> 1;
                LF_CLIP(p1 + f < 0 || q1 - f < 0, LF_CLIP_OUT_LO);
                LF_CLIP(p1 + f > px->bdmax || q1 - f > px->bdmax, LF_CLIP_OUT_HI);
                SP(1, iclip(p1 + f, 0, px->bdmax));
                SQ(1, iclip(q1 - f, 0, px->bdmax));
            }
        }
#undef P
#undef Q
#undef SP
#undef SQ
    }
}

/* loop_filter_sb[plane class][dir] (loopfilter.rs:745-985).
 * cls 0 luma, 1 chroma; dir 0 = column edges (filtering along rows, "h"), 1 = row edges.
 * `lvl` points at the level slot to use; level entries are 4 bytes. */
void oracle_lf_sb(int cls, int dir, void *dst_, ptrdiff_t stride, const uint32_t *vmask,
                  const uint8_t *lvl, ptrdiff_t b4_stride, const uint8_t *lut_e,
                  const uint8_t *lut_i, int wh, int bdmax)
{
    (void)wh;
    Px px = { bdmax > 255, bdmax, 0 };
    px.bdm8 = bdmax == 255 ? 0 : bdmax == 1023 ? 2 : 4;
    const int pxb = px.hbd ? 2 : 1;
    const ptrdiff_t ps = stride / pxb;
    uint8_t *dst = dst_;
    const unsigned vm = cls == 0 ? (vmask[0] | vmask[1] | vmask[2]) : (vmask[0] | vmask[1]);
    /* step to the next 4-px unit along the edge run, and to the neighbour for the fallback */
    const ptrdiff_t unit_px = dir == 0 ? 4 * ps : 4;
    const ptrdiff_t unit_lv = dir == 0 ? b4_stride * 4 : 4;
    const ptrdiff_t prev_lv = dir == 0 ? -4 : -b4_stride * 4;
    for (unsigned bit = 1, k = 0; vm & ~(bit - 1); bit <<= 1, k++) {
        if (!(vm & bit)) continue;
        const uint8_t *l = lvl + k * unit_lv;
        int L = l[0] ? l[0] : l[prev_lv];
        if (!L) continue;
        const int H = L >> 4, E = lut_e[L], I = lut_i[L];
        int wd;
        if (cls == 0) {
            const int idx = (vmask[2] & bit) ? 2 : !!(vmask[1] & bit);
            wd = 4 << idx;
        } else {
            wd = 4 + 2 * !!(vmask[1] & bit);
        }
        uint8_t *d = dst + (ptrdiff_t)k * unit_px * pxb;
        CEN_ONLY(lf_cell = (dir * 2 + cls) * 4 + (wd == 4 ? 0 : wd == 6 ? 1 : wd == 8 ? 2 : 3);)
        if (dir == 0) filter4lines(&px, d, E, I, H, ps, 1, wd);
        else filter4lines(&px, d, E, I, H, 1, ps, wd);
    }
}

/* Av1Filter (src/lf_mask.rs:40-51): only the deblock part is read here. */
typedef struct {
    uint16_t filter_y[2][32][3][2];
    uint16_t filter_uv[2][32][2][2];
    int8_t cdef_idx[4];
    uint16_t noskip_mask[16][2];
} OAv1Filter;

/* Whole-frame deblocking in the reference's sbrow order.
 * planes/strides: picture (bytes). level: [u8;4] per 4x4 unit, b4_stride units per row.
 * masks: Av1Filter per 128x128 ([sb128h][sb128w]). sb128: superblock size flag (affects only
 * the traversal order). filter_uv: frame_hdr.loopfilter.level_u || level_v. */
void oracle_deblock_frame(void *const planes[3], const ptrdiff_t strides[3], int w, int h,
                          int layout, int bpc, const uint8_t *level, ptrdiff_t b4_stride,
                          const void *masks_, int sb128w, int sb128, const uint8_t *lut_e,
                          const uint8_t *lut_i, int filter_y, int filter_uv)
{
    const OAv1Filter *masks = masks_;
    const int bdmax = (1 << bpc) - 1, pxb = bpc > 8 ? 2 : 1;
    const int w4 = (w + 3) >> 2, h4 = (h + 3) >> 2;
    const int is_sb64 = !sb128;
    const int sbsz = 32 >> is_sb64;
    const int sbh = (h4 + sbsz - 1) / sbsz;
    const int ss_ver = layout == 1, ss_hor = layout == 1 || layout == 2;
    const int has_uv = layout != 0 && filter_uv;
    /* deblocking is skipped as a whole when both luma levels are 0 (recon.rs:4047-4060) */
    if (!filter_y) return;

    for (int sby = 0; sby < sbh; sby++) {
        const int starty4 = (sby & is_sb64) << 4;
        const int endy4 = starty4 + imin(h4 - sby * sbsz, sbsz);
        const int uv_endy4 = (endy4 + ss_ver) >> ss_ver;
        const OAv1Filter *lflvl = masks + (sby >> is_sb64) * sb128w;
        const int row0 = sby * sbsz * 4; /* first luma pixel row of this sbrow */

        {
            /* ---- luma column edges (filter_plane_cols_y) ---- */
            for (int X = 0; X < sb128w; X++) {
                const int wx = imin(32, w4 - X * 32);
                const uint8_t *lv = level + ((ptrdiff_t)sby * sbsz * b4_stride + X * 32) * 4;
                uint8_t *p = (uint8_t *)planes[0] + (ptrdiff_t)row0 * strides[0] + (ptrdiff_t)X * 128 * pxb;
                for (int x = 0; x < wx; x++) {
                    if (X == 0 && x == 0) continue;
                    uint32_t hm[4];
                    const uint16_t (*m)[2] = lflvl[X].filter_y[0][x];
                    if (!starty4) {
                        for (int k = 0; k < 3; k++) {
                            hm[k] = m[k][0];
                            if (endy4 > 16) hm[k] |= (uint32_t)m[k][1] << 16;
                        }
                    } else {
                        for (int k = 0; k < 3; k++) hm[k] = m[k][1];
                    }
                    hm[3] = 0;
                    oracle_lf_sb(0, 0, p + x * 4 * pxb, strides[0], hm, lv + x * 4 + 0, b4_stride,
                                 lut_e, lut_i, endy4 - starty4, bdmax);
                }
            }
        }
        if (has_uv) {
            const int cw_sb = 32 >> ss_hor;
            const int crow0 = (sby * sbsz >> ss_ver) * 4;
            for (int X = 0; X < sb128w; X++) {
                const int wx = (imin(32, w4 - X * 32) + ss_hor) >> ss_hor;
                const uint8_t *lv = level + ((ptrdiff_t)(sby * sbsz >> ss_ver) * b4_stride + X * cw_sb) * 4;
                for (int x = 0; x < wx; x++) {
                    if (X == 0 && x == 0) continue;
                    uint32_t hm[3];
                    const uint16_t (*m)[2] = lflvl[X].filter_uv[0][x];
                    const int sty = starty4 >> ss_ver;
                    if (!sty) {
                        for (int k = 0; k < 2; k++) {
                            hm[k] = m[k][0];
                            if (uv_endy4 > (16 >> ss_ver)) hm[k] |= (uint32_t)m[k][1] << (16 >> ss_ver);
                        }
                    } else {
                        for (int k = 0; k < 2; k++) hm[k] = m[k][1];
                    }
                    hm[2] = 0;
                    for (int pl = 1; pl <= 2; pl++) {
                        uint8_t *p = (uint8_t *)planes[pl] + (ptrdiff_t)crow0 * strides[pl] +
                                     ((ptrdiff_t)X * cw_sb * 4 + x * 4) * pxb;
                        oracle_lf_sb(1, 0, p, strides[pl], hm, lv + x * 4 + 1 + pl, b4_stride,
                                     lut_e, lut_i, uv_endy4 - sty, bdmax);
                    }
                }
            }
        }
        {
            /* ---- luma row edges (filter_plane_rows_y) ---- */
            for (int X = 0; X < sb128w; X++) {
                for (int y = starty4; y < endy4; y++) {
                    if (sby == 0 && y == 0) continue;
                    const int ry = sby * sbsz + (y - starty4);  /* absolute 4x4 row */
                    const uint16_t (*m)[2] = lflvl[X].filter_y[1][y];
                    uint32_t vm[4] = { m[0][0] | ((uint32_t)m[0][1] << 16),
                                       m[1][0] | ((uint32_t)m[1][1] << 16),
                                       m[2][0] | ((uint32_t)m[2][1] << 16), 0 };
                    uint8_t *p = (uint8_t *)planes[0] + (ptrdiff_t)ry * 4 * strides[0] + (ptrdiff_t)X * 128 * pxb;
                    const uint8_t *lv = level + ((ptrdiff_t)ry * b4_stride + X * 32) * 4;
                    oracle_lf_sb(0, 1, p, strides[0], vm, lv + 1, b4_stride, lut_e, lut_i,
                                 imin(32, w4 - X * 32), bdmax);
                }
            }
        }
        if (has_uv) {
            const int cw_sb = 32 >> ss_hor;
            const int sty = starty4 >> ss_ver;
            for (int X = 0; X < sb128w; X++) {
                for (int y = sty; y < uv_endy4; y++) {
                    if (sby == 0 && y == 0) continue;
                    const int ry = (sby * sbsz >> ss_ver) + (y - sty);
                    const uint16_t (*m)[2] = lflvl[X].filter_uv[1][y];
                    uint32_t vm[3] = { m[0][0] | ((uint32_t)m[0][1] << (16 >> ss_hor)),
                                       m[1][0] | ((uint32_t)m[1][1] << (16 >> ss_hor)), 0 };
                    const uint8_t *lv = level + ((ptrdiff_t)ry * b4_stride + X * cw_sb) * 4;
                    for (int pl = 1; pl <= 2; pl++) {
                        uint8_t *p = (uint8_t *)planes[pl] + (ptrdiff_t)ry * 4 * strides[pl] +
                                     (ptrdiff_t)X * cw_sb * 4 * pxb;
                        oracle_lf_sb(1, 1, p, strides[pl], vm, lv + 1 + pl, b4_stride, lut_e,
                                     lut_i, (imin(32, w4 - X * 32) + ss_hor) >> ss_hor, bdmax);
                    }
                }
            }
        }
    }
}

/* rav1d_calc_eih (src/lf_mask.rs:608-626; C src/lf_mask.c:408-425) */
void oracle_calc_eih(uint8_t *lut_e, uint8_t *lut_i, int sharp)
{
    for (int level = 0; level < 64; level++) {
        int limit = level;
        if (sharp > 0) {
            limit >>= (sharp + 3) >> 2;
            limit = imin(limit, 9 - sharp);
        }
        limit = imax(limit, 1);
        lut_i[level] = (uint8_t)limit;
        lut_e[level] = (uint8_t)(2 * (level + 2) + limit);
    }
}
