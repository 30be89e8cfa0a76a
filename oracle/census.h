/*
 * oracle/census.h — event counters and single-decision mutants for the in-loop filter and
 * inverse-transform restatements (TEST INFRASTRUCTURE ONLY).
 *
 * loopfilter.c, cdef.c, lr.c and itx.c are compiled twice from the same sources. The plain build
 * (liboracle.so) sees every macro below expand to nothing or to the constant 0, so it holds
 * no counter, no extra branch and no global. The census build (liboracle_census.so,
 * -DORACLE_CENSUS) counts how often each decision of the filters is taken and how often it
 * sits exactly at its limit, and can flip one decision at a time (`mutant`), which is how the
 * tests show that their inputs would notice such a slip in a kernel.
 *
 * The census build keeps its state in plain globals: call it from one thread only.
 */
#ifndef MI_ORACLE_CENSUS_H
#define MI_ORACLE_CENSUS_H

#include <stdint.h>

/* ---- mutant numbers ---- */
enum {
    MUT_NONE = 0,
    /* deblock: comparison c (LF_CMP_*) taken as `<` where the reference has `<=` */
    MUT_LF_LT = 1,                     /* + LF_CMP_* for the 19 `<=` comparisons */
    MUT_LF_HEV_GE_P = 20,              /* |p1 - p0| > H taken as >= */
    MUT_LF_HEV_GE_Q = 21,              /* |q1 - q0| > H taken as >= */
    MUT_LF_SUM8_I16 = 22,              /* 8-tap sums truncated to int16 before the shift */
    MUT_LF_SUM16_I16 = 23,             /* 13-tap sums truncated to int16 before the shift */
    MUT_CDEF_TIE_GE = 24,              /* direction search keeps the last of equal costs */
    MUT_CDEF_NO_CLAMP = 25,            /* min/max clamp removed */
    MUT_CDEF_SENTINEL_SAMPLE = 26,     /* the unavailable-sample sentinel joins the minimum */
    MUT_WIENER_NO_HCLIP_LO = 27,       /* horizontal pass: lower clip bound removed */
    MUT_WIENER_NO_HCLIP_HI = 28,       /* horizontal pass: upper clip bound removed */
    MUT_SGR_PS_I32 = 29,               /* p * s taken as int32 before its shift */
    MUT_SGR_XSUM_I32 = 30,             /* x * sum * one_by_x taken as int32 before its shift */
    /* inverse transforms (itx.c) */
    MUT_ITX_ROT_I32 = 31,              /* rotations, S12 and H181 evaluated in wrapping 32-bit */
    MUT_ITX_NO_CLIP = 32,              /* the 1-D intermediate CL() removed */
    MUT_ITX_NO_MIDCLIP = 33,           /* the clip between the row and the column pass removed */
    MUT_ITX_MID_I16 = 34,              /* the row-to-column hand-off truncated to int16 */
    MUT_ITX_RES_I16 = 35,              /* the residual (c + 8) >> 4 truncated to int16 */
    MUT_ITX_WHT_MID_I16 = 36,          /* the WHT row result truncated to int16 */
    MUT_COUNT = 37
};

/* ---- deblock comparisons, in the order the reference evaluates them ---- */
enum {
    LF_CMP_I_P1P0, LF_CMP_I_Q1Q0, LF_CMP_E, LF_CMP_I_P2P1, LF_CMP_I_Q2Q1, LF_CMP_I_P3P2,
    LF_CMP_I_Q3Q2,
    LF_CMP_FO_P6, LF_CMP_FO_P5, LF_CMP_FO_P4, LF_CMP_FO_Q4, LF_CMP_FO_Q5, LF_CMP_FO_Q6,
    LF_CMP_FI_P2, LF_CMP_FI_P1, LF_CMP_FI_Q1, LF_CMP_FI_Q2, LF_CMP_FI_P3, LF_CMP_FI_Q3,
    LF_CMP_H_P, LF_CMP_H_Q,
    LF_NCMP
};
/* deblock branches */
enum { LF_BR_NONE, LF_BR_NARROW_HEV, LF_BR_NARROW, LF_BR_6TAP, LF_BR_8TAP, LF_BR_13TAP, LF_NBR };
/* narrow-filter clip events */
enum {
    LF_CLIP_D_LO, LF_CLIP_D_HI,        /* clip(p1 - q1) at its bounds (hev only) */
    LF_CLIP_F_LO, LF_CLIP_F_HI,        /* f at its bounds */
    LF_CLIP_F4_MAX, LF_CLIP_F3_MAX,    /* f + 4 and f + 3 cut at fmax */
    LF_CLIP_OUT_LO, LF_CLIP_OUT_HI,    /* an output cut at 0 / bdmax */
    LF_NCLIP
};

/* per (dir, cls, width) cell of the deblock census */
#define LF_CELL_BRANCH 0                                 /* [LF_NBR] lines per branch */
#define LF_CELL_AT (LF_CELL_BRANCH + LF_NBR)             /* [LF_NCMP] deciding, distance == limit */
#define LF_CELL_AT1 (LF_CELL_AT + LF_NCMP)               /* [LF_NCMP] deciding, distance == limit + 1 */
#define LF_CELL_PIN_LO (LF_CELL_AT1 + LF_NCMP)           /* [LF_NBR] smoother lines all within F of 0 */
#define LF_CELL_PIN_HI (LF_CELL_PIN_LO + LF_NBR)         /* [LF_NBR] ... of bdmax */
#define LF_CELL_CLIP (LF_CELL_PIN_HI + LF_NBR)           /* [LF_NCLIP] */
#define LF_CELL_PAIR (LF_CELL_CLIP + LF_NCLIP)           /* [LF_NBR][LF_NBR], a <= b */
#define LF_CELL_SIZE (LF_CELL_PAIR + LF_NBR * LF_NBR)
#define LF_NCELL (2 * 2 * 4)

enum {
    CEN_LF = 0,
    CEN_CDEF_TIES = CEN_LF + LF_NCELL * LF_CELL_SIZE, /* [9]: searches with k directions at the best cost */
    CEN_CDEF_WIN = CEN_CDEF_TIES + 9,               /* [8] winner of every search */
    CEN_CDEF_WIN_SUBTIE = CEN_CDEF_WIN + 8,         /* [8] winner where 2..7 directions tie */
    CEN_CDEF_VAR0 = CEN_CDEF_WIN_SUBTIE + 8,
    CEN_CDEF_PX_BOTH,                               /* pixels filtered with both strengths on */
    CEN_CDEF_PX_CLAMPED,                            /* ... whose value the clamp changed */
    CEN_CDEF_PX_SENTINEL,                           /* pixels with a tap on the sentinel */
    CEN_CDEF_PX_PRISHIFT0,                          /* pixels whose pri_shift was clamped to 0 */
    CEN_CDEF_PX_NEG,                                /* sum < 0 rounding */
    CEN_CDEF_PX_OUT0, CEN_CDEF_PX_OUTMAX,
    CEN_WIENER_HCLIP_LO, CEN_WIENER_HCLIP_HI, CEN_WIENER_VCLIP_LO, CEN_WIENER_VCLIP_HI,
    CEN_SGR_Z0,                                     /* [2]: radius 2 (5x5), radius 1 (3x3) */
    CEN_SGR_Z255 = CEN_SGR_Z0 + 2,
    CEN_SGR_PS31 = CEN_SGR_Z255 + 2,
    CEN_SGR_XSUM31 = CEN_SGR_PS31 + 2,
    CEN_SGR_OUT_LO = CEN_SGR_XSUM31 + 2, CEN_SGR_OUT_HI,
    CEN_LR_SET,                                     /* [3 planes][16 sets] unit-stripes restored */
    CEN_LR_WIENER = CEN_LR_SET + 48,                /* [3 planes] */
    /* inverse transforms: every group is [3], indexed by bit depth (8, 10, 12) */
    CEN_ITX_ROW_CLIP_LO = CEN_LR_WIENER + 3,        /* 1-D intermediate clip, row pass */
    CEN_ITX_ROW_CLIP_HI = CEN_ITX_ROW_CLIP_LO + 3,
    CEN_ITX_COL_CLIP_LO = CEN_ITX_ROW_CLIP_HI + 3,  /* ... column pass */
    CEN_ITX_COL_CLIP_HI = CEN_ITX_COL_CLIP_LO + 3,
    CEN_ITX_MID_CLIP_LO = CEN_ITX_COL_CLIP_HI + 3,  /* hand-off clip between the passes */
    CEN_ITX_MID_CLIP_HI = CEN_ITX_MID_CLIP_LO + 3,
    CEN_ITX_PX_CLIP_0 = CEN_ITX_MID_CLIP_HI + 3,    /* pixel clip at 0 / bdmax */
    CEN_ITX_PX_CLIP_MAX = CEN_ITX_PX_CLIP_0 + 3,
    CEN_ITX_RES_GT_I16 = CEN_ITX_PX_CLIP_MAX + 3,   /* residual (c + 8) >> 4 beyond int16 */
    CEN_ITX_WHT_MID_GT_I16 = CEN_ITX_RES_GT_I16 + 3, /* WHT row result beyond int16 */
    CEN_ITX_ROT_GE_2P31 = CEN_ITX_WHT_MID_GT_I16 + 3, /* exact rotation sum (its +2048 included, ADST4's
                                                     * four-term sums too) at or beyond 2^31 in magnitude */
    CEN_COUNT = CEN_ITX_ROT_GE_2P31 + 3
};

#ifdef ORACLE_CENSUS
extern uint64_t oracle_census_ctr[CEN_COUNT];
extern int oracle_census_mutant;
#define CEN(i) (oracle_census_ctr[(i)]++)
#define CEN_IF(c, i) do { if (c) oracle_census_ctr[(i)]++; } while (0)
#define CEN_ONLY(...) __VA_ARGS__
#define MUT(n) (oracle_census_mutant == (n))
#else
#define CEN(i) ((void)0)
#define CEN_IF(c, i) ((void)0)
#define CEN_ONLY(...)
#define MUT(n) 0
#endif

#endif
