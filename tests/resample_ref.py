"""float64 restatement of the resampler (multimodal-s2ut_amd/prepare.py, csrc/resample.hip) as direct
loops over the formulas, sharing no code with the product: the reference for tests/test_prepare.py and
tests/test_gpu_resample.py.

    g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) rolloff,
    width = ceil(lpw o / base), K = 2 width + o
    t = clamp((-i / n + (c - width) / o) base, -lpw, lpw)
    h[i][c] = sinc(pi t) w(t) base / o,  w = I0(beta sqrt(1 - (t / lpw)^2)) / I0(beta)  or  cos^2(pi t / (2 lpw))
    y[j n + i] = sum_c h[i][c] xp[j o + c],  xp[t] = x[t - width] inside the clip, 0 outside;  ceil(n L / o) outputs
"""
import math

import numpy as np

LPW, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492


def i0(x):
    """Modified Bessel function of the first kind, order 0: its power series sum_k ((x/2)^k / k!)^2, summed
    until a term no longer changes the float64 sum."""
    s, term, k = 1.0, 1.0, 0
    while True:
        k += 1
        term *= (x / 2.0 / k) ** 2
        if s + term == s:
            return s
        s += term


def taps(orig, new, lpw=LPW, rolloff=ROLLOFF, window="kaiser", beta=BETA):
    """-> (h float64 [n, K], width, o, n)"""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    K = 2 * width + o
    h = np.empty((n, K), dtype=np.float64)
    i0b = i0(beta)
    for i in range(n):
        for c in range(K):
            t = (-i / n + (c - width) / o) * base
            t = min(max(t, -float(lpw)), float(lpw))
            if window == "hann":
                w = math.cos(t * math.pi / lpw / 2) ** 2
            else:
                w = i0(beta * math.sqrt(max(0.0, 1.0 - (t / lpw) ** 2))) / i0b
            a = math.pi * t
            h[i, c] = (1.0 if a == 0.0 else math.sin(a) / a) * w * base / o
    return h, width, o, n


def resample(x, h, width, o, n):
    """float64 output of clip x through the table h (float64, or the product's fp32 table widened)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    L, K = len(x), h.shape[1]
    n_out = -(-n * L // o)
    frames = -(-n_out // n)
    xp = np.zeros((frames - 1) * o + K + width, dtype=np.float64)
    m = min(L, len(xp) - width)
    xp[width:width + m] = x[:m]
    y = np.empty(frames * n, dtype=np.float64)
    for j in range(frames):
        seg = xp[j * o:j * o + K]
        for i in range(n):
            y[j * n + i] = float(np.dot(h[i], seg))
    return y[:n_out]


def bound(h, K, xmax):
    """The fp32 dot-product bound (K + 2) 2^-24 max_i sum_c |h[i][c]| max|x|: K FMAs and the one rounding of
    each tap, from the taps alone."""
    return (K + 2) * 2.0 ** -24 * float(np.abs(np.asarray(h, dtype=np.float64)).sum(1).max()) * float(xmax)
