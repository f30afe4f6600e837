"""Cases of the decode-side reconstruction parity test (tests/test_gpu_recon.py)
and the check that they cover every AC strategy the encoder can emit: the
reconstruction kernels (csrc/jxg_recon.hip) have one path per strategy, so a
strategy no case chooses would be a path no test runs."""
import numpy as np

# raw strategy ids the encoder emits: the 8x8 class (DCT8, IDENTITY, DCT2X2,
# DCT4X4, DCT4X8, DCT8X4), the merged shapes up to 64x64, and 128 / 256 px
EMITTED = set(range(0, 8)) | {10, 11, 12, 13} | set(range(18, 27))


def gradient_rgb8(w, h, seed):
    """smooth frame on which effort 8 chooses the 128 / 256 px shapes (the
    generator of tests/test_gpu_bigvb.py)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 60 * np.sin(x / rng.uniform(150, 400) + y / rng.uniform(150, 400) + c)
                    for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def _natural(w, h, seed):
    from jxg.synth import natural_rgb8

    return natural_rgb8(w, h, seed)


def _synth(w, h, seed):
    from jxg.synth import synth_rgb8

    return synth_rgb8(w, h, seed)


def _gradient_t(w, h, seed):
    """the transpose of gradient_rgb8(h, w): tall shapes where that has wide ones"""
    return np.ascontiguousarray(gradient_rgb8(h, w, seed).transpose(1, 0, 2))


# name, generator, width, height, seed, distance, effort, proposals, coder
# (0 prefix codes, 1 ANS), filter mask (Gaborish 1 | EPF 2 | masking AQ 4, as
# oracle_ffi.encode takes it).  The first five are the coverage set.
CASES = [
    ("natural_d1.5_epf", _natural, 200, 136, 5, 1.5, 7, 0, 1, 2),
    ("natural_d12_all", _natural, 333, 222, 8, 12.0, 7, 0, 1, 7),
    ("gradient_e8", gradient_rgb8, 768, 520, 768 * 7 + 520, 2.0, 8, 0, 1, 0),
    ("gradient_e8_tall", _gradient_t, 520, 768, 768 * 7 + 520, 2.0, 8, 0, 1, 0),
    ("gradient_e8_all", gradient_rgb8, 512, 512, 512 * 7 + 512, 1.0, 8, 0, 1, 7),
    ("1x1", _synth, 1, 1, 0x4A584C00, 1.0, 7, 0, 1, 7),
    ("9x7", _synth, 9, 7, 0x4A584C01, 3.0, 7, 0, 1, 7),
    ("natural_d1_plain", _natural, 200, 136, 5, 1.0, 7, 0, 1, 0),
    ("natural_d1_gab", _natural, 200, 136, 5, 1.0, 7, 0, 1, 1),
    ("natural_d1_all", _natural, 200, 136, 5, 1.0, 7, 0, 1, 7),
    ("natural_d4_epf3", _natural, 200, 136, 5, 4.0, 7, 0, 1, 7),
    ("natural_d6_e5", _natural, 300, 200, 3, 6.0, 5, 0, 1, 2),
    ("natural_hooks", _natural, 200, 136, 6, 1.0, 7, 3, 1, 7),
    ("natural_prefix", _natural, 200, 136, 7, 2.0, 7, 0, 0, 7),
]
COVERAGE = CASES[:5]


def case_image(case):
    _, gen, w, h, seed = case[:5]
    img = gen(w, h, seed)
    assert img.shape == (h, w, 3) and img.dtype == np.uint8
    return img


def case_flags(jxg_mod, case):
    coder, mask = case[8], case[9]
    return ((jxg_mod.FLAG_ANS if coder else 0) | (jxg_mod.FLAG_GABORISH if mask & 1 else 0) |
            (jxg_mod.FLAG_EPF if mask & 2 else 0) | (jxg_mod.FLAG_AQ_MASKING if mask & 4 else 0))


def test_case_names_are_unique():
    assert len({c[0] for c in CASES}) == len(CASES)


def test_cases_cover_every_emitted_strategy(oracle):
    """the oracle encodes the coverage set; the union of the first blocks'
    strategy ids holds every id the encoder emits"""
    seen = set()
    for case in COVERAGE:
        d, e, p, coder, mask = case[5:]
        r = oracle.encode(case_image(case), d, e, p, coder, mask)
        seen |= set(int(t) for t in np.unique(r.acs[(r.acs & 0x80) == 0]))
    assert EMITTED <= seen, sorted(EMITTED - seen)
