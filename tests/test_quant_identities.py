"""The float identities the round-5 quantization code relies on
(csrc/jxg_front.hip quant_lane / quant_xb, csrc/jxg_merge_kernel.h quant_pass),
checked in IEEE single precision on the CPU (numpy float32 arithmetic rounds
to nearest like the GPU's VALU; no contraction is involved):

* non-zero counts from exponent sums: a quantized magnitude qf is an
  integer-valued float in [0, 32767]; a zero has biased exponent E = 0, a
  non-zero E = 127 + floor(log2 qf) in [127, 141], so for <= 8 values
  sum(E) / 127 (integer division) is their non-zero count and
  2 sum(E) - 250 nz is the rate sum over non-zeros of 2 + 2 bitlen(qf)
  (oracle/front.c jxo_quantize_block).  Sixteen values can break the division
  -- the merge stage splits a 16-row item into two sums of eight;
* the signed error: with sq = copysign(qf, vq), (vq - sq) * sd is +-((|vq| -
  qf) * sd) exactly, so its square -- the only use -- is the oracle's;
* the tabulated AdjustQuantBias: adj(q) for q < 256 is the same float
  expression the kernels evaluated per coefficient before;
* the signed value: (int)copysign(qf, vq) == (vq < 0 ? -(int)qf : (int)qf),
  and v_cvt_pk_i16_i32's pair packing equals the mask / shift form at
  |q| <= 32767;
* the clamp: the oracle's quant1 (oracle/front.c: a < 32767 ? (int)(a + 0.5f)
  : 32767) and the kernels' floorf(fminf(a, 32767) + 0.5f) agree on every f32
  around 32767, on inf and on NaN (fminf returns its other argument), and the
  identities above hold with all eight values at the clamp or in the top token
  class (distances below 0.1 put them there: tests/highrate_cases.py).
"""
import numpy as np
import pytest

f32 = np.float32


def quantize(vq):
    """qf of the kernels: |vq| < 0.58 -> 0 else floor(min(|vq|, 32767) + 0.5), in f32"""
    a = np.abs(vq).astype(f32)
    q = np.floor(np.fmin(a, f32(32767.0)) + f32(0.5)).astype(f32)  # fmin: C's fminf on NaN
    return np.where(a < f32(0.58), f32(0.0), q).astype(f32)


def biased_exp(qf):
    return (qf.astype(f32).view(np.uint32) >> 23).astype(np.int64)


def bitlen(v):
    v = np.asarray(v, dtype=np.int64)
    out = np.zeros_like(v)
    for b in range(16):
        out = np.where(v >> b != 0, b + 1, out)
    return out


@pytest.mark.parametrize("n", [1, 2, 7, 8])
def test_nonzero_count_from_exponent_sum(n):
    rng = np.random.default_rng(100 + n)
    # magnitudes across the whole range, many zeros, the extremes included
    vals = rng.integers(0, 32768, size=(20000, n))
    vals[rng.random(vals.shape) < 0.4] = 0
    vals[0, :] = 32767
    vals[1, :] = 1
    qf = vals.astype(f32)
    E = biased_exp(qf)
    nz = (vals != 0).sum(axis=1)
    assert np.array_equal(E.sum(axis=1) // 127, nz)
    rate = np.where(vals != 0, 2 + 2 * bitlen(vals), 0).sum(axis=1)
    assert np.array_equal(2 * E.sum(axis=1) - 250 * nz, rate)


def test_sixteen_values_need_two_sums():
    vals = np.array([32767] * 10 + [0] * 6)
    E = biased_exp(vals.astype(f32))
    assert E.sum() // 127 != 10  # one sum over 16 miscounts
    assert E[:8].sum() // 127 + E[8:].sum() // 127 == 10  # the merge stage's split


def test_signed_error_is_plus_minus_the_oracle_error():
    rng = np.random.default_rng(7)
    vq = (rng.standard_normal(200000) * rng.choice([0.3, 3.0, 300.0, 3e4], 200000)).astype(f32)
    vq[:4] = [f32(0.0), f32(-0.0), f32(0.58), f32(-0.57999)]
    sd = rng.uniform(0.01, 4.0, vq.size).astype(f32)
    qf = quantize(vq)
    sq = np.copysign(qf, vq).astype(f32)
    e_oracle = ((np.abs(vq) - qf).astype(f32) * sd).astype(f32)
    e_signed = ((vq - sq).astype(f32) * sd).astype(f32)
    assert np.array_equal(np.abs(e_signed), np.abs(e_oracle))
    assert np.array_equal((e_signed * e_signed).astype(f32), (e_oracle * e_oracle).astype(f32))
    # the signed quantized value and its int16 pair packing
    q_old = np.where(vq < 0, -qf.astype(np.int64), qf.astype(np.int64))
    q_new = sq.astype(np.int64)  # C's (int) truncation; sq is integer-valued
    assert np.array_equal(q_old, q_new)
    lo, hi = q_new[0::2], q_new[1::2]
    mask_form = (lo & 0xFFFF) | ((hi & 0xFFFF) << 16)
    sat = lambda v: np.clip(v, -32768, 32767) & 0xFFFF  # v_cvt_pk_i16_i32
    assert np.array_equal(mask_form, sat(lo) | (sat(hi) << 16))


def test_bias_table_is_the_per_coefficient_expression():
    kbias1 = f32(1.0) - f32(0.07005449891748593)
    for q in range(256):
        qf = f32(q)
        per_coef = f32(0.0) if q == 0 else (kbias1 if q == 1 else f32(qf - f32(0.145) / qf))
        table = f32(0.0) if q == 0 else (kbias1 if q == 1 else f32(f32(q) - f32(0.145) / f32(q)))
        assert per_coef.view(np.uint32) == table.view(np.uint32)


def oracle_quant1(v):
    """oracle/front.c quant1, expression by expression (the int conversion only
    where C defines it)"""
    v = np.asarray(v, dtype=f32)
    a = np.abs(v)
    below = a < f32(32767.0)  # false for NaN
    with np.errstate(invalid="ignore"):
        q = np.where(below, np.trunc(np.where(below, a, f32(0.0)) + f32(0.5)), 32767.0).astype(np.int64)
    q = np.minimum(q, 32767)
    q = np.where(a < f32(0.58), 0, q)
    return np.where(v < 0, -q, q)


def test_clamp_matches_the_oracle_on_every_float_around_it():
    lo, hi = f32(32766.0).view(np.uint32), f32(32768.5).view(np.uint32)
    v = np.arange(int(lo), int(hi) + 1, dtype=np.uint32).view(f32)
    assert v[0] == 32766.0 and v[-1] == 32768.5 and v.size == 1024 + 128 + 1
    v = np.concatenate([v, -v, np.array([np.inf, -np.inf, np.nan, 3.0e38, 65536.0, 1e9], dtype=f32)])
    with np.errstate(invalid="ignore"):
        qf = quantize(v)
    assert qf.max() == 32767 and not np.isnan(qf).any()
    q = oracle_quant1(v)
    assert np.array_equal(np.abs(q), qf.astype(np.int64))
    ok = ~np.isnan(v)  # (NaN has no sign the two sides must agree on)
    assert np.array_equal(q[ok], np.copysign(qf, v)[ok].astype(np.int64))
    # round half up just below the clamp, the clamp from 32766.5 on
    assert quantize(np.array([32766.498], dtype=f32))[0] == 32766
    assert quantize(np.array([32766.5], dtype=f32))[0] == 32767
    # the packed pair at the clamp: saturation is the identity there
    pair = np.array([32767, -32767], dtype=np.int64)
    assert np.array_equal(np.clip(pair, -32768, 32767), pair)
    assert (pair & 0xFFFF).tolist() == [0x7FFF, 0x8001]


def test_rate_and_count_at_the_top_token_class():
    for mag, rate in ((16384, 32), (32767, 32), (16383, 30), (255, 18), (256, 20)):
        E = biased_exp(np.array([mag], dtype=f32))[0]
        assert 2 * E - 250 == rate == 2 + 2 * bitlen(mag)
    # eight values, each in the top class or at the clamp, with and without zeros
    rng = np.random.default_rng(11)
    vals = rng.integers(16384, 32768, size=(4096, 8))
    vals[0, :] = 32767
    vals[1, :] = 16384
    vals[2:2048][rng.random((2046, 8)) < 0.3] = 0
    E = biased_exp(vals.astype(f32))
    nz = (vals != 0).sum(axis=1)
    assert E.sum(axis=1).max() == 8 * 141
    assert np.array_equal(E.sum(axis=1) // 127, nz)
    assert np.array_equal(2 * E.sum(axis=1) - 250 * nz, 32 * nz)
