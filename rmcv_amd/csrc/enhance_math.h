/*
 * enhance_math.h -- rm::AutoEnhance / rm::CalcGamma (src/imgproc.cpp:37-48, 77-98) as arithmetic: the gamma of a frame from its
 * channel sums, the 256-entry table of a gamma, and the threshold table the pixel kernel reads.  HIP-free and PM_FN like
 * pinned_math.h: the SAME source builds the table on the host (rmcv_gamma_lut, rmcv_enhance_gamma, the CPU tests) and on the device
 * (k_enhance_table).  Compile with -ffp-contract=off, no fast-math.
 */
#ifndef RMCV_ENHANCE_MATH_H
#define RMCV_ENHANCE_MATH_H

#include "pinned_math.h"

/* imgproc.cpp:79-95.  sums: exact integer sums of the B, G, R bytes of a frame of n pixels.  cv::mean multiplies each sum by the
 * reciprocal of the pixel count (as recalled; not pinned against OpenCV); the three means are added in double, left to right,
 * narrowed once and divided by 3 in float; everything after that is float arithmetic in the reference's order. */
PM_FN float enh_gamma(const uint64_t sums[3], int64_t n, float max_gain, float min_gain)
{
    const double rn = 1.0 / (double)n;
    const double m0 = (double)sums[0] * rn, m1 = (double)sums[1] * rn, m2 = (double)sums[2] * rn;
    const float mean_c3 = (float)((m0 + m1) + m2) / 3.0f;
    const float k = 2.0f / (max_gain - min_gain);
    const float b = 3.0f - max_gain * k;
    float g = k * mean_c3 + b;
    if (g <= 1.0f && g >= -3.0f) g = 1.0f + (g - 1.0f) / 4.0f; /* map [1, -3] to [1, 0] */
    else if (g < -3.0f) g = 0.0f;                                /* frame too dark */
    return g;
}

/* imgproc.cpp:43: cv::saturate_cast<uchar>(pow(i / 255.0, gamma) * 255.0) -- cvRound (half to even), clamped to 0..255.
 * gamma >= 0 and finite (the callers check); pow(0, 0) = 1 as in C. */
PM_FN uint8_t enh_lut_entry(int i, float gamma)
{
    const double v = pm_pow((double)i / 255.0, (double)gamma) * 255.0;
    const double r = (v + 4503599627370496.0) - 4503599627370496.0; /* round half to even, 0 <= v < 2^51 */
    return (uint8_t)(r < 0.0 ? 0 : (r > 255.0 ? 255 : (int)r));
}

/* With a non-decreasing table,  lut[a] - lut[b] >= lb  <=>  a >= M[b],  M[b] = min{a : lut[a] >= lut[b] + lb}  (256: no such a).
 * lb in 1 .. 256.  The pixel kernel keeps M, not the table: one lookup per pixel, and the bound is folded in. */
PM_FN uint16_t enh_m_entry(const uint8_t* lut, int b, int lb)
{
    const int need = (int)lut[b] + lb;
    int lo = 0, hi = 256; /* first a in [0, 256] with lut[a] >= need */
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)lut[mid] >= need) hi = mid;
        else lo = mid + 1;
    }
    return (uint16_t)lo;
}

#endif /* RMCV_ENHANCE_MATH_H */
