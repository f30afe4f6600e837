"""The MS-SSIM reference (tests/msssim_ref.py) against its own definition: the
degenerate cases, the exactness of the pyramid in f32, scale 0 against
oracle/metrics.py, and an independent textbook evaluation."""
import math

import numpy as np
import pytest

import metrics
import msssim_ref


def _pair(h, w, seed, noise=12):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int32) + rng.integers(-noise, noise + 1, a.shape), 0, 255)
    return a, b.astype(np.uint8)


def test_identical_images_give_one_everywhere():
    a, _ = _pair(180, 200, 1)
    r = msssim_ref.msssim(a, a)
    assert r["ms_ssim"] == 1.0
    assert r["cs"] == [1.0] * 5 and r["ssim"] == [1.0] * 5


@pytest.mark.parametrize("h,w", [(176, 176), (177, 191)])
def test_scale0_is_the_oracle_ssim(h, w):
    a, b = _pair(h, w, h * 1000 + w)
    r = msssim_ref.msssim(a, b)
    assert r["ssim"][0] == metrics.ssim(a, b)
    assert 0.0 < r["ms_ssim"] < 1.0


@pytest.mark.parametrize("h,w", [(176, 176), (177, 191), (530, 700)])
def test_pyramid_is_exact_in_f32(h, w):
    a, _ = _pair(h, w, h * 1000 + w)
    lv = msssim_ref.pyramid(a)
    assert len(lv) == 5
    for j, planes in enumerate(lv):
        for p in planes:
            assert p.shape == (h >> j, w >> j)
            assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
            assert np.array_equal(p * 256.0, np.floor(p * 256.0)) and float(p.max()) < 256.0


@pytest.mark.parametrize("h,w", [(175, 400), (400, 175)])
def test_under_176_is_nan(h, w):
    a, b = _pair(h, w, 2)
    r = msssim_ref.msssim(a, b)
    assert math.isnan(r["ms_ssim"])
    assert all(math.isnan(v) for v in r["cs"] + r["ssim"])


def test_inverted_noise_is_exactly_zero():
    a, _ = _pair(200, 240, 3)
    r = msssim_ref.msssim(a, 255 - a)
    assert r["ms_ssim"] == 0.0 and math.copysign(1.0, r["ms_ssim"]) == 1.0
    assert all(v < 0.0 for v in r["cs"][:4])
    assert r["cs"][:4] == pytest.approx([-0.99, -0.95, -0.82, -0.42], abs=0.01)


def _maps_direct(a, b):
    """Textbook evaluation: direct 2-D 11 x 11 window sums with the outer-product
    kernel (another summation order than the separable reference)."""
    g1 = metrics.gaussian_window()
    g = np.outer(g1, g1)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    wa = np.lib.stride_tricks.sliding_window_view(np.asarray(a, np.float64), (11, 11))
    wb = np.lib.stride_tricks.sliding_window_view(np.asarray(b, np.float64), (11, 11))

    def mean(x):
        return np.einsum("yxij,ij->yx", x, g)

    ma, mb = mean(wa), mean(wb)
    va = mean(wa * wa) - ma * ma
    vb = mean(wb * wb) - mb * mb
    cab = mean(wa * wb) - ma * mb
    cs = (2 * cab + c2) / (va + vb + c2)
    return (2 * ma * mb + c1) / (ma * ma + mb * mb + c1) * cs, cs


def test_textbook_evaluation_agrees():
    a, b = _pair(176, 180, 176180)
    r = msssim_ref.msssim(a, b)
    d = msssim_ref.msssim(a, b, maps_fn=_maps_direct)
    assert d["ms_ssim"] == pytest.approx(r["ms_ssim"], rel=1e-9)
    assert d["cs"] == pytest.approx(r["cs"], rel=1e-9)
    assert d["ssim"] == pytest.approx(r["ssim"], rel=1e-9)
    # and the pooling / product written out once more, from the means
    v = math.prod(max(c, 0.0) ** w for c, w in zip(d["cs"][:4], msssim_ref.W)) * \
        max(d["ssim"][4], 0.0) ** msssim_ref.W[4]
    assert v == pytest.approx(r["ms_ssim"], rel=1e-9)
