"""Float64 numpy reference of MS-SSIM (Wang, Simoncelli, Bovik 2003) as the
library defines it -- TEST INFRASTRUCTURE ONLY; the product
path is csrc/jxg_metrics.hip behind jxg_msssim_rgb8.

* Five scales; scale 0 is the two RGB8 images, each channel on its own, and
  scale j + 1 is ``((p[2y][2x] + p[2y][2x+1]) + (p[2y+1][2x] + p[2y+1][2x+1]))
  * 0.25`` of scale j with an odd last row or column dropped, so scale j has
  ``(w >> j) x (h >> j)`` samples.  Every sample is a multiple of 1/256 below
  256: exact in f32 (``pyramid`` returns f64; ``test_msssim_ref`` checks the
  round trip).
* Per window: ``oracle/metrics.py ssim_map`` restated expression for
  expression (window, taps ascending, horizontal then vertical, C1, C2), plus
  ``cs = (2.0 * cab + C2) / (vaa + vbb + C2)``.
* ``cs[j]`` / ``ssim[j]``: the sum over all windows of the three channels,
  pooled as ``metrics.ssim`` does, over ``3.0 * (w_j - 10) * (h_j - 10)``.
* ``ms_ssim = prod_{j<4} max(cs[j], 0)**W[j] * max(ssim[4], 0)**W[4]``,
  multiplied in ascending j from 1.0; NaN in every field when
  ``min(w, h) < 176`` (scale 4 under 11 x 11).
"""
import math

import numpy as np

import metrics

W = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SCALES = 5
MIN_EDGE = 176


def maps(a: np.ndarray, b: np.ndarray):
    """(ssim, cs) per window of one channel; the ssim map is metrics.ssim_map's."""
    g = metrics.gaussian_window()
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    h, w = a.shape
    oh, ow = h - 10, w - 10
    m = []
    for q in (a, b, a * a, b * b, a * b):
        acc = np.zeros((h, ow))
        for k in range(11):
            acc = acc + g[k] * q[:, k:k + ow]
        acc2 = np.zeros((oh, ow))
        for k in range(11):
            acc2 = acc2 + g[k] * acc[k:k + oh, :]
        m.append(acc2)
    c1 = (0.01 * 255.0) * (0.01 * 255.0)
    c2 = (0.03 * 255.0) * (0.03 * 255.0)
    mab = m[0] * m[1]
    maa = m[0] * m[0]
    mbb = m[1] * m[1]
    vaa = m[2] - maa
    vbb = m[3] - mbb
    cab = m[4] - mab
    num = (2.0 * mab + c1) * (2.0 * cab + c2)
    den = (maa + mbb + c1) * (vaa + vbb + c2)
    return num / den, (2.0 * cab + c2) / (vaa + vbb + c2)


def down(p: np.ndarray) -> np.ndarray:
    h, w = p.shape
    p = p[:2 * (h // 2), :2 * (w // 2)]
    return ((p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2])) * 0.25


def pyramid(img: np.ndarray):
    """[scale][channel] f64 planes of an (H, W, 3) uint8 image"""
    lv = [[np.asarray(img)[:, :, k].astype(np.float64) for k in range(3)]]
    for _ in range(SCALES - 1):
        lv.append([down(p) for p in lv[-1]])
    return lv


def combine(cs, ssim) -> float:
    v = 1.0
    for j in range(SCALES - 1):
        v *= max(cs[j], 0.0) ** W[j]
    v *= max(ssim[SCALES - 1], 0.0) ** W[SCALES - 1]
    return v


def msssim(orig: np.ndarray, comp: np.ndarray, maps_fn=maps) -> dict:
    """{"ms_ssim", "cs"[5], "ssim"[5]} of two (H, W, 3) uint8 images"""
    h, w = np.asarray(orig).shape[:2]
    if min(h, w) < MIN_EDGE:
        return {"ms_ssim": math.nan, "cs": [math.nan] * SCALES, "ssim": [math.nan] * SCALES}
    pa, pb = pyramid(orig), pyramid(comp)
    cs, ss = [], []
    for j in range(SCALES):
        hj, wj = pa[j][0].shape
        assert (hj, wj) == (h >> j, w >> j)
        n = 3.0 * (wj - 10) * (hj - 10)
        ts = tc = 0.0
        for k in range(3):
            s, c = maps_fn(pa[j][k], pb[j][k])
            ts += float(np.sum(s))
            tc += float(np.sum(c))
        ss.append(ts / n)
        cs.append(tc / n)
    return {"ms_ssim": combine(cs, ss), "cs": cs, "ssim": ss}
