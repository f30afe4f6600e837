"""The decoder on the GPU against crafted codestreams (tests/crafted.py): every
varblock placement the decoder accepts -- any block offset inside a 64x64 tile
for the shapes up to 64 px, any inside a pass group for the 128 / 256 px ones,
merged shapes flush with the edges of frames of 9, 12, 25 and 28 blocks -- and the ends
of every value range.  No encoder writes such streams from an image, so the
token walk (csrc/jxg_decode_core.h), the head / type scatter and LLF rebuild of
recon_tile_kernel and the origin arithmetic of recon_big_kernel
(csrc/jxg_recon.hip) run at such offsets only here.  The streams passed the
host path first (tests/test_crafted_streams.py).

Maps are compared exactly.  Pixels (S1 - S3) against the float64 oracle
decoder: no sample differs by more than 1, and at most 0.5 % of the samples
differ IN EVERY 64x64 TILE SEPARATELY (an edge tile: of the samples it has) --
the project's bound of tests/test_gpu_recon.py, which there binds over the
frame only, so that a path wrong on a few hundred pixels of one tile passes.

What the reference alone does on these frames, float64 against the same
reconstruction with its planes rounded to f32 between the stages
(crafted.reconstruct_f32), measured over all 38 pixel cases: the largest
difference is 1, the largest differing share of a frame 3.1e-5, the largest of
one tile 1.6e-4 (2 samples of 12288) -- a thirtieth of the per-tile cap; the
magnitudes were to keep it below a fifth, which
tests/test_crafted_streams.py asserts on four of the frames.

Measured on an MI355X: the largest difference 1 in every case, the largest
differing share of a frame 6.9e-5, of one tile 6.5e-4 (one sample of the 8 px
wide edge tile of s3_72x200_3); every test under 0.5 s (the whole module
6.2 s, the batch of 44 streams 0.14 s).
"""
import time

import numpy as np
import pytest

import crafted
from test_gpu_decode import DEC_PARAMS

pytestmark = pytest.mark.gpu

MAX_SHARE = 0.005
OK, INVALID_ARG = 0, -1

ALL = crafted.all_cases
PIXEL = crafted.pixel_cases


@pytest.fixture(scope="module")
def dec(jxg_mod):
    with jxg_mod.Encoder(**DEC_PARAMS) as d:
        yield d


_single = {}


def _decoded(dec, case):
    """dec.decode of the case's stream, once"""
    if case.name not in _single:
        t0 = time.perf_counter()
        _single[case.name] = dec.decode(crafted.stream(case))
        print("%s: decode %.3f s" % (case.name, time.perf_counter() - t0))
    return _single[case.name]


@pytest.mark.parametrize("case", ALL(), ids=[c.name for c in ALL()])
def test_maps_come_back_exactly(jxg_mod, dec, case):
    t0 = time.perf_counter()
    got = jxg_mod.decode_maps(crafted.stream(case), dec)
    print("%s: decode_maps %.3f s" % (case.name, time.perf_counter() - t0))
    for k in crafted.MAPS:
        want = getattr(case, k)
        assert got[k].shape == want.shape and np.array_equal(got[k], want), k


@pytest.mark.parametrize("case", PIXEL(), ids=[c.name for c in PIXEL()])
def test_pixels_match_the_oracle_in_every_tile(dec, case):
    got = _decoded(dec, case)
    ref, seconds = crafted.reference(case)
    assert got.shape == ref.rgb.shape and got.dtype == np.uint8
    worst, share, tile = crafted.tile_shares(got, ref.rgb)
    print("%s: max |diff| %d, differing share %.3g, worst tile %.3g (reference %.1f s)" % (
        case.name, worst, share, tile, seconds))
    assert worst <= 1, "a sample differs by %d" % worst
    assert tile <= MAX_SHARE, "%.4f %% of a tile's samples differ" % (100 * tile)


def test_batch_equals_the_single_decodes(dec):
    cases = ALL()
    t0 = time.perf_counter()
    outs = dec.decode_batch([crafted.stream(c) for c in cases])
    print("decode_batch of %d streams: %.3f s" % (len(cases), time.perf_counter() - t0))
    for c, o in zip(cases, outs):
        assert np.array_equal(o, _decoded(dec, c)), c.name


@pytest.fixture(scope="module")
def good():
    return crafted.families()["S3"][0]


def test_a_coefficient_outside_int16_comes_back_invalid(jxg_mod, dec, good):
    """the first status the pass-group kernel itself returns: the headers and LF
    groups parse, the value is inside a pass group's entropy-coded section"""
    s5 = crafted.stream(crafted.s5_case())
    assert jxg_mod.load().jxg_decode_maps(None, s5, len(s5), None, None, None, None, None) \
        == INVALID_ARG
    out = np.full((64, 64, 3), 0xA5, np.uint8)
    assert jxg_mod.load().jxg_decode_rgb8(dec._ctx, s5, len(s5), out.ctypes.data, 64 * 3) \
        == INVALID_ARG
    # the context decodes the next stream as before
    after = dec.decode(crafted.stream(good))
    worst, _, tile = crafted.tile_shares(after, crafted.reference(good)[0].rgb)
    assert worst <= 1 and tile <= MAX_SHARE
    assert np.array_equal(after, _decoded(dec, good))


def test_an_invalid_frame_inside_a_batch(jxg_mod, dec, good):
    s5 = crafted.stream(crafted.s5_case())
    ok = crafted.stream(good)
    other = crafted.families()["S3"][4]
    want = [_decoded(dec, good), None, _decoded(dec, other)]
    datas = [ok, s5, crafted.stream(other)]
    outs, st = dec.decode_batch(datas, strict=False)
    assert st == [OK, INVALID_ARG, OK]
    assert outs[1] is None
    assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[2], want[2])
    # the refused frame's buffer is untouched
    bufs = [np.full((c.h, c.w, 3), 0xA5, np.uint8) for c in (good, crafted.s5_case(), other)]
    ret, st = dec._decode_batch_call(jxg_mod.load().jxg_decode_batch_rgb8, datas,
                                     [b.ctypes.data for b in bufs], [b.shape[1] * 3 for b in bufs])
    assert st == [OK, INVALID_ARG, OK] and ret != OK
    assert np.all(bufs[1] == 0xA5)
    assert np.array_equal(bufs[0], want[0]) and np.array_equal(bufs[2], want[2])
