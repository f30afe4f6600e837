"""ac_hist's band record layout (csrc/jxg_acrec.h rec_index, the shipped
function run by tests/native/ac_model.cpp): a pass group's token stream is its
four bands' streams in order, band j's records at [j * kBandTokStride, ...);
the coders map stream position k to its record slot.  Every band-count
pattern, empty bands included (partial groups: a 64-px-tall frame has one
non-empty band), must give the concatenation."""
import itertools

import pytest

import ac_model_native

K_BAND_TOK_STRIDE = 256 * 3 * 64  # jxg_acrec.h kBandTokStride
PATTERNS = list(itertools.product((0, 1, 7, 64), repeat=4))


@pytest.fixture(scope="module")
def rec_index(tmp_path_factory):
    """band counts -> rec_index(bt, k) for every stream position k, one run for all patterns"""
    exe = ac_model_native.build(tmp_path_factory)
    out = {}
    for ln in ac_model_native.run(exe, "rec_index", "".join("%d %d %d %d\n" % bt for bt in PATTERNS)):
        bt, idx = ln.split(":")
        out[tuple(int(v) for v in bt.split())] = [int(v) for v in idx.split()]
    assert sorted(out) == sorted(PATTERNS)
    return out


@pytest.mark.parametrize("bt", PATTERNS)
def test_rec_index_concatenates_bands(rec_index, bt):
    want = [j * K_BAND_TOK_STRIDE + i for j in range(4) for i in range(bt[j])]
    assert rec_index[bt] == want
