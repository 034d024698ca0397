"""rm::AutoEnhance / rm::CalcGamma (the reference's src/imgproc.cpp:37-48, 77-98) restated in plain numpy + math.pow: what the
library's enhancement must equal, byte for byte.  No product code is used here.

    S_c    = exact integer sum of channel c                    m_c = float64(S_c) * (1.0 / float64(w * h))      (cv::mean, as recalled)
    meanC3 = float32(m_B + m_G + m_R) / float32(3)             k = 2 / (max - min), b = 3 - max * k, g = k * meanC3 + b   (float32)
    g      = 1 + (g - 1) / 4 if -3 <= g <= 1;  0 if g < -3;  unchanged otherwise
    LUT[i] = saturate_cast<uchar>(pow(i / 255.0, float64(g)) * 255.0)     round half to even, clamp; pow(0, 0) = 1
"""
import math

import numpy as np

F = np.float32


def gamma_from_mean(mean_c3, max_gain=100.0, min_gain=50.0):
    """imgproc.cpp:82-95 on a float32 mean"""
    mean_c3, max_gain, min_gain = F(mean_c3), F(max_gain), F(min_gain)
    k = F(F(2.0) / F(max_gain - min_gain))
    b = F(F(3.0) - F(max_gain * k))
    g = F(F(k * mean_c3) + b)
    if g <= F(1.0) and g >= F(-3.0):
        g = F(F(1.0) + F(F(g - F(1.0)) / F(4.0)))
    elif g < F(-3.0):
        g = F(0.0)
    return g


def gamma_from_sums(sums, n_pixels, max_gain=100.0, min_gain=50.0):
    """imgproc.cpp:79-95: the channel means from exact integer sums (times the reciprocal of the count), then the gamma"""
    rn = 1.0 / float(n_pixels)
    m = [float(int(s)) * rn for s in sums]
    mean_c3 = F(F((m[0] + m[1]) + m[2]) / F(3.0))
    return gamma_from_mean(mean_c3, max_gain, min_gain)


def sums(frame):
    """exact channel sums of an (h, w, 3) uint8 frame"""
    return [int(frame[..., c].sum(dtype=np.uint64)) for c in range(3)]


def gamma_of(frame, max_gain=100.0, min_gain=50.0):
    return gamma_from_sums(sums(frame), frame.shape[0] * frame.shape[1], max_gain, min_gain)


def lut(gamma):
    """imgproc.cpp:39-44 with the host's libm"""
    g = float(F(gamma))
    out = np.empty(256, np.uint8)
    for i in range(256):
        v = math.pow(i / 255.0, g) * 255.0
        r = round(v)  # Python rounds half to even, as cvRound does
        out[i] = min(255, max(0, r))
    return out


def calc_gamma(img, gamma):
    """rm::CalcGamma: the table applied to every byte"""
    return lut(gamma)[img]


def E(frame, max_gain=100.0, min_gain=50.0):
    """rm::AutoEnhance of a BGR frame -> (enhanced frame, gamma)"""
    g = gamma_of(frame, max_gain, min_gain)
    return lut(g)[frame], g


def m_table(table, lb):
    """brute force: M[b] = min{a : table[a] - table[b] >= lb}, 256 when there is none"""
    t = table.astype(np.int64)
    ok = (t[:, None] - t[None, :]) >= lb  # [a, b]
    return np.where(ok.any(axis=0), ok.argmax(axis=0), 256).astype(np.uint16)


def dim(frames, num):
    """an under-exposed camera: (v * num) >> 8"""
    return ((frames.astype(np.uint16) * num) >> 8).astype(np.uint8)
