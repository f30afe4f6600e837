"""The quantizers' wave-uniform zero path (jxg_merge_kernel.h quant_pass, jxg_front.hip
quant_xb): where every active lane of a wave quantizes its coefficients to 0, the
rounding and rate arithmetic is skipped.  The frames here put the votes in every
state -- all zero in every channel (flat), one lane non-zero in one wave (a
single bright pixel, moved through the places the lane map distinguishes), values
on both sides of the 0.58 threshold (stepped ramps), no vote zero (noise),
waves with invalid varblocks and partial tiles (odd sizes), a NaN estimate --
and every case compares the GPU encode with the oracle: codestream bytes, the
strategy / quant-field / DC maps and the quantized coefficients."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (cjxl preset, effort, proposals)
SETTINGS = [(cjxl, e, p) for cjxl in (False, True) for e in (5, 7) for p in (0, 3)]


def flat(w, h, v=128):
    return np.full((h, w, 3), v, dtype=np.uint8)


def pixel(w, h, y, x, v):
    img = flat(w, h)
    img[y, x] = v
    return img


def ramp(w, h, vertical):
    """a ramp per 8-pixel stripe whose slope grows from stripe to stripe (0,
    0.15, 0.3, ... grey levels per pixel): the first AC coefficient of the
    stripes' blocks passes through the quantizer's threshold on the way"""
    n, m = (w, h) if vertical else (h, w)
    slope = (np.arange(n) // 8) * 0.15
    t = np.arange(m) - m / 2.0
    g = 128.0 + slope[:, None] * t[None, :]  # [stripe position][along the ramp]
    if vertical:
        g = g.T
    return np.repeat(np.clip(np.rint(g), 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)


def smooth(w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 90 * np.sin(x / (9.0 + 4 * c) + y / (17.0 - 3 * c) + c) for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frames():
    import oracle_ffi

    oracle_ffi.build()
    out = {
        # every vote zero, in every channel
        "flat": flat(192, 136),
        # one bright (or faint) pixel: first / last varblock of a band of 64
        # columns, rows 0-7 / 8-15 of a 16-row chunk, the last 16-row chunk of
        # a 64-tall shape, a tile that is not the first
        "px_first_vb": pixel(192, 136, 3, 2, 255),
        "px_last_vb": pixel(192, 136, 5, 61, 255),
        "px_rows_0_7": pixel(192, 136, 18, 34, 255),
        "px_rows_8_15": pixel(192, 136, 28, 34, 140),
        "px_last_chunk": pixel(192, 136, 60, 20, 255),
        "px_tile_1_1": pixel(192, 136, 77, 130, 0),
        "ramp_h": ramp(192, 136, False),
        "ramp_v": ramp(192, 136, True),
        # synth's noise tiles beside its smooth ones; white noise: no vote zero
        "noise": oracle_ffi.synth_rgb8(192, 136, 21),
        "white": np.random.default_rng(7).integers(0, 256, (136, 192, 3), dtype=np.uint8),
        # partial tiles, invalid varblocks inside a wave
        "noise_72x40": oracle_ffi.synth_rgb8(72, 40, 22),
        "smooth_136x72": smooth(136, 72),
        "px_72x40": pixel(72, 40, 33, 66, 255),
    }
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_ref(name, cjxl, effort, proposals):
    import oracle_ffi

    return oracle_ffi.encode(frames()[name], 1.0, effort, proposals, 1 if cjxl else 0,
                             7 if cjxl else 0)


def flags_of(jxg_mod, cjxl):
    return jxg_mod.FLAG_KEEP_MAPS | (jxg_mod.FLAGS_CJXL_DEFAULTS if cjxl else 0)


def assert_matches(got, st, ref, what):
    assert np.array_equal(st["acs"], ref.acs), what
    assert np.array_equal(st["qf"], ref.qf), what
    assert np.array_equal(st["dc"], ref.dc), what
    assert np.array_equal(st["ac"], ref.ac), what
    assert got == ref.bytes, what


def test_frames_are_what_the_cases_need():
    """(oracle only) the flat frame has no non-zero coefficient, the pixel
    frames few, white noise mostly non-zeros in every channel; the ramps have blocks
    that quantize to all zero and blocks that do not, at slopes other than 0"""
    ref = oracle_ref("flat", True, 7, 0)
    assert not ref.ac.any()
    for name in ("px_first_vb", "px_last_vb", "px_rows_0_7", "px_rows_8_15", "px_last_chunk",
                 "px_tile_1_1", "px_72x40"):
        nzb = (oracle_ref(name, True, 7, 0).ac != 0).any(axis=(2, 3))
        assert 0 < nzb.sum() <= 8, (name, int(nzb.sum()))
    for name in ("noise", "noise_72x40"):
        assert (oracle_ref(name, True, 7, 0).ac != 0).mean() > 0.02, name
    assert (oracle_ref("white", True, 7, 0).ac != 0).mean(axis=(0, 1, 3)).min() > 0.5
    for name, axis in (("ramp_h", 0), ("ramp_v", 1)):
        for cjxl in (False, True):
            nzb = (oracle_ref(name, cjxl, 7, 0).ac != 0).any(axis=(2, 3))
            stripes = np.moveaxis(nzb, axis, 0)[1:]  # stripe 0 has slope 0
            assert stripes.any() and not stripes.all(), (name, cjxl)


@pytest.mark.parametrize("cjxl,effort,proposals", SETTINGS)
def test_every_frame_matches_oracle(jxg_mod, cjxl, effort, proposals):
    with jxg_mod.Encoder(distance=1.0, effort=effort, proposals=proposals,
                         flags=flags_of(jxg_mod, cjxl)) as enc:
        for name, img in frames().items():
            got = enc.encode(img)
            assert_matches(got, enc.stats(), oracle_ref(name, cjxl, effort, proposals), name)


@pytest.mark.parametrize("cjxl,proposals", [(True, 0), (False, 3)])
def test_batched_flat_and_noise(jxg_mod, cjxl, proposals):
    """two queued frames share the launches (blockIdx.z): one whose votes are
    all zero beside one whose votes never are"""
    names = ["flat", "noise"]
    refs = [oracle_ref(n, cjxl, 7, proposals).bytes for n in names]
    with jxg_mod.Encoder(distance=1.0, effort=7, proposals=proposals,
                         flags=flags_of(jxg_mod, cjxl) & ~jxg_mod.FLAG_KEEP_MAPS) as enc:
        for n in names:
            enc.submit(frames()[n])
        queued = []
        while enc.pending():
            queued.append(enc.receive())
    assert queued == refs


@pytest.mark.parametrize("cjxl,proposals", [(False, 2), (False, 3), (True, 3)])
def test_nan_estimates_take_the_full_path(jxg_mod, oracle, cjxl, proposals):
    """all-black tiles: hook F makes every estimate NaN (and the merge accepts
    NaN); the vote's negated compare leaves NaN to the full path"""
    img = np.zeros((136, 200, 3), dtype=np.uint8)
    img[:, 128:] = smooth(72, 136)
    ref = oracle.encode(img, 1.0, 7, proposals, 1 if cjxl else 0, 7 if cjxl else 0)
    if not cjxl and proposals == 2:
        assert ((ref.acs[:8, :8] & 0x7F) == 20).all()
    with jxg_mod.Encoder(distance=1.0, effort=7, proposals=proposals,
                         flags=flags_of(jxg_mod, cjxl)) as enc:
        got = enc.encode(img)
        assert_matches(got, enc.stats(), ref, "nan")
