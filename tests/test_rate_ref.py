"""The rate report's cost model against real streams, on the CPU: the host-only
jxg_rate_symbol_cost, and tests/rate_ref.py on codestreams the oracle encoder
writes.  Prefix codes: the summed cost of a pass group IS the bits its AC
stream occupies, exactly.  ANS: the summed -log2 costs and the emitted bits
differ by the coder's state overhead; the range measured on these streams is
pinned (widened by two about its midpoint), so a cost model that drifted from
the stream -- a wrong histogram, a wrong token -- fails here, before any kernel
is compared with it."""
import ctypes

import pytest

import rate_ref
from test_recon_cases import CASES, case_image

# emitted bits - cost / 256 per pass group over the ANS streams of CASES, as
# measured with this file: the 32-bit state minus what the
# final state gives back, plus rANS's rounding.  Least: gradient_e8_all (a
# group of 2.45), most: gradient_e8 (55.70).
ANS_DIFF_OBSERVED = (2.453125, 55.6953125)
_MID = (ANS_DIFF_OBSERVED[0] + ANS_DIFF_OBSERVED[1]) / 2
_HALF = ANS_DIFF_OBSERVED[1] - ANS_DIFF_OBSERVED[0]  # twice the observed half-width
ANS_DIFF_BOUND = (_MID - _HALF, _MID + _HALF)


def test_symbol_cost_equals_the_formula(jxg_mod):
    lib = jxg_mod.load()
    assert lib.jxg_rate_symbol_cost.restype is ctypes.c_uint32
    got = [lib.jxg_rate_symbol_cost(f) for f in range(4098)]
    assert got == [rate_ref.symbol_cost(f) for f in range(4098)]
    assert got[0] == 0 and got[4097] == 0 and got[4096] == 0 and got[1] == 3072 == max(got)
    assert got[2048] == 256 and jxg_mod.rate_symbol_cost(1024) == 512
    assert jxg_mod.RATE_UNIT == 256


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_prefix_cost_is_the_stream(oracle, case):
    """every image of CASES with prefix codes: cost == 256 x bits read, per group"""
    d, e, p, _, mask = case[5:]
    r = oracle.encode(case_image(case), d, e, p, 0, mask)
    ref = rate_ref.reference(r.bytes)
    assert ref["ans"] == 0
    for g in range(ref["groups"]):
        assert ref["group_cost"][g] == 256 * ref["group_bits"][g], g
        assert 0 <= 8 * ref["group_bytes"][g] - ref["group_bits"][g]
    assert int(ref["block_cost"].astype("uint64").sum()) == int(ref["cost"].sum()) == sum(
        ref["group_cost"])
    assert [int(v) for v in ref["tokens"].sum(axis=0)] == [int(v) for v in r.ac_tokens.sum(axis=0)]


def test_ans_cost_against_the_stream(oracle):
    """the ANS streams of CASES: emitted bits - cost / 256 per pass group"""
    lo, hi = float("inf"), float("-inf")
    for case in CASES:
        d, e, p, coder, mask = case[5:]
        if not coder:
            continue
        r = oracle.encode(case_image(case), d, e, p, 1, mask)
        ref = rate_ref.reference(r.bytes)
        assert ref["ans"] == 1
        for g in range(ref["groups"]):
            diff = ref["group_bits"][g] - ref["group_cost"][g] / 256.0
            print(case[0], g, ref["group_bits"][g], ref["group_cost"][g], diff)
            lo, hi = min(lo, diff), max(hi, diff)
            assert ANS_DIFF_BOUND[0] <= diff <= ANS_DIFF_BOUND[1], (case[0], g, diff)
    print("observed", lo, hi)
