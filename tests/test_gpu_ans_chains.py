"""The rANS chain kernels (csrc/jxg_ans.hip: ans_chain, one lane per chain, codes
the streamed frames -- submit / receive; ans_chain_diag, one wave per chain,
codes a frame encoded by itself -- encode) at the group counts where the
lane-per-chain mapping changes: exactly one full wave of chains (64 pass
groups), a second wave that holds a single chain (65), and a wave whose lanes
have very unequal lengths (66 groups, a flat left part).  Codestream bytes
against the oracle's ANS coder, as test_ans_matches_oracle does, through both
entry points; all three frames have ragged right and bottom groups.  Also the
streaming pipeline with 5 frames in flight, twice on one context (stale
per-wave state would show in the second pass), and the smallest frames (one
group, one lane in use)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _noise(w, h):
    from jxg.synth import synth_rgb8

    return synth_rgb8(w, h, w * 5 + h)


def _unequal(w, h):
    """left 1280 columns (5 whole group columns) flat, the rest noise"""
    img = _noise(w, h)
    img[:, :1280] = (90, 140, 60)
    return img


# name, width, height, distance, effort, proposals, pass groups, image
CASES = [("full_wave", 4000, 1000, 1.0, 5, 3, 64, _noise),
         ("second_wave_one_chain", 3100, 1100, 1.0, 7, 0, 65, _noise),
         ("unequal_lengths", 2570, 1290, 0.5, 7, 2, 66, _unequal)]

_ref_cache = {}


def _case(oracle, name):
    """(image, oracle result) of a case, computed once per session"""
    if name not in _ref_cache:
        _, w, h, d, e, p, ng, make = next(c for c in CASES if c[0] == name)
        assert ((w + 255) // 256) * ((h + 255) // 256) == ng
        img = make(w, h)
        _ref_cache[name] = (img, oracle.encode(img, d, e, p, 1))
    return _ref_cache[name]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_chain_waves_match_oracle(jxg_mod, oracle, name):
    _, w, h, d, e, p, ng, _ = next(c for c in CASES if c[0] == name)
    img, ref = _case(oracle, name)
    flags = jxg_mod.FLAG_ANS | jxg_mod.FLAG_KEEP_MAPS
    with jxg_mod.Encoder(distance=d, effort=e, proposals=p, flags=flags) as enc:
        got = enc.encode(img)
        tok = np.asarray(enc.stats()["ac_tokens"], dtype=np.int64).reshape(ng, -1).sum(axis=1)
        enc.submit(img)  # the lane-per-chain kernel
        streamed = enc.receive()
    assert np.array_equal(tok, np.asarray(ref.ac_tokens, dtype=np.int64).reshape(ng, -1).sum(axis=1))
    if name == "unequal_lengths":
        print("tokens per group: min %d max %d" % (tok.min(), tok.max()))
        assert tok.max() >= 10 * tok.min(), "case does not make the chain lengths unequal"
    assert got == ref.bytes
    assert streamed == ref.bytes


def test_chain_stream_two_passes(jxg_mod, oracle):
    """65 groups through submit / receive, 5 frames in flight, twice on one
    context: every frame's bytes equal the oracle's"""
    _, w, h, d, e, p, _, _ = CASES[1]
    img, ref = _case(oracle, CASES[1][0])
    with jxg_mod.Encoder(distance=d, effort=e, proposals=p, flags=jxg_mod.FLAG_ANS) as enc:
        for rnd in range(2):
            for _ in range(5):
                enc.submit(img)
            assert enc.pending() == 5
            for i in range(5):
                assert enc.receive() == ref.bytes, "pass %d frame %d" % (rnd, i)


@pytest.mark.parametrize("w,h", [(9, 7), (64, 64)])
def test_chain_one_group(jxg_mod, oracle, w, h):
    img = _noise(w, h)
    with jxg_mod.Encoder(distance=1.0, effort=7, proposals=0, flags=jxg_mod.FLAG_ANS) as enc:
        got = enc.encode(img)
        enc.submit(img)
        streamed = enc.receive()
    ref = oracle.encode(img, 1.0, 7, 0, 1).bytes
    assert got == ref
    assert streamed == ref
