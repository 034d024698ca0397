/*
 * leaf_funcs.h -- TEST INFRASTRUCTURE: every leaf function of rmcv_amd/csrc/pinned_math.h and enhance_math.h, and the IEEE primitives those
 * headers take for granted, behind one numbered entry point.  The same text is compiled three times -- by gcc as C (leaf_host_main.c: the
 * build the CPU oracle and the tests' references use), by hipcc's clang host pass and by hipcc for gfx950 (leaf_main.hip) -- and the three
 * must give the same bits (tests/test_leaf_cpu.py, tests/test_gpu_leaf.py).
 *
 * Every argument and every result travels as a 64-bit slot: a double as its bits, a float as its 32 bits (upper half zero), an integer as
 * itself.  tests/leaf_cases.py holds the same table of ids (FUNCS) and says what each slot means.
 */
#ifndef RMCV_LEAF_FUNCS_H
#define RMCV_LEAF_FUNCS_H

#include "../../rmcv_amd/csrc/enhance_math.h"

#define LEAF_MAGIC 0x4641454Cu /* "LEAF" */
#define LEAF_MAX_ARGS 6

enum {
    LEAF_SIN = 0, LEAF_COS, LEAF_TAN, LEAF_ATAN, LEAF_ATAN2, LEAF_ACOS, LEAF_SINF, LEAF_COSF, LEAF_ATAN2F, LEAF_FMOD180, LEAF_LOG, LEAF_EXP,
    LEAF_POW, LEAF_HYPOT, LEAF_ENH_GAMMA, LEAF_LUT_ENTRY,
    LEAF_SQRT64, LEAF_SQRT32, LEAF_DIV64, LEAF_DIV32, LEAF_FMA64, LEAF_ADD32, LEAF_MUL32, LEAF_ADD64, LEAF_MUL64, LEAF_NARROW, LEAF_I64_TO_F64,
    LEAF_U64_TO_F64, LEAF_RINT, LEAF_RINTF, LEAF_FLOORF, LEAF_F64_TO_INT, LEAF_F32_TO_INT,
    LEAF_N_FUNCS
};

/* the number of argument slots of every id, in the enum's order */
#define LEAF_NARGS_TABLE {1, 1, 1, 1, 2, 1, 1, 1, 2, 1, 1, 1, 2, 2, 6, 2, 1, 1, 2, 2, 3, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1}

PM_FN double leaf_d(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
PM_FN float leaf_f(uint64_t u) { uint32_t w = (uint32_t)u; float f; __builtin_memcpy(&f, &w, 4); return f; }
PM_FN uint64_t leaf_ud(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
PM_FN uint64_t leaf_uf(float f) { uint32_t w; __builtin_memcpy(&w, &f, 4); return (uint64_t)w; }

/* element i of record `fid`; a[k] is the k-th argument array */
PM_FN uint64_t leaf_eval(int fid, const uint64_t* const* a, uint64_t i)
{
    switch (fid) {
        case LEAF_SIN: return leaf_ud(pm_sin(leaf_d(a[0][i])));
        case LEAF_COS: return leaf_ud(pm_cos(leaf_d(a[0][i])));
        case LEAF_TAN: return leaf_ud(pm_tan(leaf_d(a[0][i])));
        case LEAF_ATAN: return leaf_ud(pm_atan(leaf_d(a[0][i])));
        case LEAF_ATAN2: return leaf_ud(pm_atan2(leaf_d(a[0][i]), leaf_d(a[1][i])));
        case LEAF_ACOS: return leaf_ud(pm_acos(leaf_d(a[0][i])));
        case LEAF_SINF: return leaf_uf(pm_sinf(leaf_f(a[0][i])));
        case LEAF_COSF: return leaf_uf(pm_cosf(leaf_f(a[0][i])));
        case LEAF_ATAN2F: return leaf_uf(pm_atan2f(leaf_f(a[0][i]), leaf_f(a[1][i])));
        case LEAF_FMOD180: {
            /* pm_fmod180's loop does not end for +infinity: nothing outside its contract (0 <= x < 720, or NaN) reaches it, whatever the file says */
            const double x = leaf_d(a[0][i]);
            if (x == x && !(x >= 0.0 && x < 720.0)) return 0xBADBADBADBADBADBull;
            return leaf_ud(pm_fmod180(x));
        }
        case LEAF_LOG: return leaf_ud(pm_log(leaf_d(a[0][i])));
        case LEAF_EXP: return leaf_ud(pm_exp(leaf_d(a[0][i])));
        case LEAF_POW: return leaf_ud(pm_pow(leaf_d(a[0][i]), leaf_d(a[1][i])));
        case LEAF_HYPOT: return leaf_ud(pm_hypot(leaf_d(a[0][i]), leaf_d(a[1][i])));
        case LEAF_ENH_GAMMA: {
            const uint64_t sums[3] = {a[0][i], a[1][i], a[2][i]};
            return leaf_uf(enh_gamma(sums, (int64_t)a[3][i], leaf_f(a[4][i]), leaf_f(a[5][i])));
        }
        case LEAF_LUT_ENTRY: return (uint64_t)enh_lut_entry((int)a[0][i], leaf_f(a[1][i]));
        case LEAF_SQRT64: return leaf_ud(__builtin_sqrt(leaf_d(a[0][i])));
        case LEAF_SQRT32: return leaf_uf(__builtin_sqrtf(leaf_f(a[0][i])));
        case LEAF_DIV64: return leaf_ud(leaf_d(a[0][i]) / leaf_d(a[1][i]));
        case LEAF_DIV32: return leaf_uf(leaf_f(a[0][i]) / leaf_f(a[1][i]));
        case LEAF_FMA64: return leaf_ud(__builtin_fma(leaf_d(a[0][i]), leaf_d(a[1][i]), leaf_d(a[2][i])));
        case LEAF_ADD32: return leaf_uf(leaf_f(a[0][i]) + leaf_f(a[1][i]));
        case LEAF_MUL32: return leaf_uf(leaf_f(a[0][i]) * leaf_f(a[1][i]));
        case LEAF_ADD64: return leaf_ud(leaf_d(a[0][i]) + leaf_d(a[1][i]));
        case LEAF_MUL64: return leaf_ud(leaf_d(a[0][i]) * leaf_d(a[1][i]));
        case LEAF_NARROW: return leaf_uf((float)leaf_d(a[0][i]));
        case LEAF_I64_TO_F64: return leaf_ud((double)(int64_t)a[0][i]);
        case LEAF_U64_TO_F64: return leaf_ud((double)a[0][i]);
        case LEAF_RINT: return leaf_ud(__builtin_rint(leaf_d(a[0][i])));
        case LEAF_RINTF: return leaf_uf(__builtin_rintf(leaf_f(a[0][i])));
        case LEAF_FLOORF: return leaf_uf(__builtin_floorf(leaf_f(a[0][i])));
        case LEAF_F64_TO_INT: return (uint64_t)(uint32_t)(int)leaf_d(a[0][i]); /* in-range arguments only (the case list's rule) */
        case LEAF_F32_TO_INT: return (uint64_t)(uint32_t)(int)leaf_f(a[0][i]);
        default: return 0;
    }
}

#endif /* RMCV_LEAF_FUNCS_H */
