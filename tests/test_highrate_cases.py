"""Distances below 0.1 on the CPU: the oracle, the Python decoder and the bottom
of the distance range (tests/highrate_cases.py holds the frames and the table).

* the effective distance is max(distance, 1e-6): any smaller request gives the
  bytes of 1e-6, and the quality of a white-noise frame never collapses (before
  the floor a distance below ~3.3e-10 overflowed the quant field's float -> int
  conversion and came out with raw = 1, the coarsest field: MSE 5554 at 1e-17);
* every case reaches the edge it is in the table for (REACH, asserted exactly
  from the oracle's maps): coefficients at +-32767 in 8x8-class and in merged
  varblocks, the top token class with and without the clamp, stored qf 255, the
  global scale on either side of its clamp of 73727, a 128 px varblock;
* the token record's edge: tok 63 with nbits 13 occurs, with every value of
  the two mantissa bits of the top class, and so does the non-zero count of a
  fully dense 8x8 block (63);
* the oracle's codestream is read back exactly by the Python decoder, with
  either coder;
* the reference of the pixel comparisons of test_gpu_highrate.py is stable:
  the float64 reconstruction against itself rounded to f32 between its stages
  (crafted.reconstruct_f32) differs on a share of at most one tenth of the
  GPU bound.  Measured: 0 samples differ in every one of the 12 cases (largest
  difference 0, frame share 0.0, worst tile share 0.0)."""
import numpy as np
import pytest

import crafted
import highrate_cases as H
from highrate_cases import CJXL7, CJXL8, PLAIN5, PLAIN7

BELOW_FLOOR = (1e-7, 1e-10, 1e-17, 1e-38, float(np.nextafter(np.float32(0), np.float32(1))))


def _r(qf, G, c8, merged, qdc=44):
    keys = ("max", "sat", "big")
    return {"qf": qf, "G": G, "qdc": qdc, "c8": dict(zip(keys, c8)), "merged": dict(zip(keys, merged))}


# What the oracle reaches, per case: stored qf range, global scale, and per class
# (8x8 / merged) the largest |q| of X, Y, B, the coefficients at +-32767 and
# those >= 16384 (highrate_cases.reach)
REACH = {
    ("half264", 0.001, CJXL7): _r((255, 255), 73727, ([0, 32767, 6365], 1, 3), ([0, 32767, 350], 24, 96)),
    ("half264", 0.001, PLAIN5): _r((255, 255), 73727, ([0, 32767, 3172], 1, 3), ([0, 32767, 10780], 36, 60)),
    ("half264", 0.004, PLAIN5): _r((141, 255), 73727, ([0, 21208, 0], 0, 1), ([0, 32767, 10780], 36, 60)),
    ("half264", 0.0111, CJXL8): _r((67, 75), 72879, ([0, 11484, 0], 0, 0), ([0, 29785, 0], 0, 6), qdc=45),
    ("half264", 0.0108, PLAIN5): _r((52, 97), 73727, ([0, 7916, 0], 0, 0), ([0, 26595, 0], 0, 24)),
    ("edge72", 0.004, CJXL7): _r((185, 207), 73727, ([0, 31778, 0], 0, 3), ([0, 27834, 0], 0, 12)),
    ("white72", 0.001, CJXL7): _r((219, 235), 73727, ([9031, 30609, 6384], 0, 76), ([0, 0, 0], 0, 0)),
    ("white72", 0.001, PLAIN7): _r((255, 255), 73727, ([5243, 18250, 6601], 0, 2), ([0, 0, 0], 0, 0)),
    ("tri64", 0.001, PLAIN7): _r((255, 255), 73727, ([0, 14989, 0], 0, 0), ([0, 19159, 0], 0, 32)),
    ("tri64", 0.001, CJXL8): _r((255, 255), 73727, ([0, 11847, 0], 0, 0), ([0, 18080, 0], 0, 1)),
    ("colour264", 0.001, CJXL7): _r((255, 255), 73727, ([87, 10869, 2535], 0, 0), ([165, 24817, 3300], 0, 12)),
    ("corners72", 0.001, CJXL7): _r((255, 255), 73727, ([17735, 32767, 21487], 3, 282),
                                    ([9359, 29592, 5850], 0, 15)),
    ("corners72", 0.001, PLAIN5): _r((255, 255), 73727, ([9897, 32767, 21001], 1, 123), ([0, 0, 0], 0, 0)),
}


def test_the_table_is_covered():
    assert set(REACH) == set(H.CASES)


@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_case_reaches_its_edge(case):
    got = H.reach(H.oracle_ref(*case))
    print(H.case_id(case), got)
    assert got == REACH[case]


def test_edges_by_name():
    """the same facts by what they are for (were REACH regenerated from a
    changed image, these would still say what the table needs)"""
    reach = {c: H.reach(H.oracle_ref(*c)) for c in H.CASES}
    # the clamp in both classes, under either coder / preset
    for c in (("half264", 0.001, CJXL7), ("half264", 0.001, PLAIN5)):
        assert reach[c]["c8"]["sat"] >= 1 and reach[c]["merged"]["sat"] >= 1, c
        assert reach[c]["qf"] == (255, 255), c
    # in merged varblocks only
    c = ("half264", 0.004, PLAIN5)
    assert reach[c]["merged"]["sat"] >= 1 and reach[c]["c8"]["sat"] == 0
    assert reach[c]["qf"][0] < 255 and reach[c]["qf"][1] == 255
    # the global scale on either side of its clamp, nothing saturated
    assert reach[("half264", 0.0111, CJXL8)]["G"] < H.G_CLAMP
    assert reach[("half264", 0.0108, PLAIN5)]["G"] == H.G_CLAMP
    for c in (("half264", 0.0111, CJXL8), ("half264", 0.0108, PLAIN5)):
        assert reach[c]["merged"]["big"] >= 1 and reach[c]["merged"]["sat"] == 0, c
    # the top token class without the clamp, in 8x8-class blocks
    c = ("edge72", 0.004, CJXL7)
    assert reach[c]["c8"]["big"] >= 1 and reach[c]["c8"]["sat"] == reach[c]["merged"]["sat"] == 0
    # a masking field below the ceiling at the clamped global scale
    c = ("white72", 0.001, CJXL7)
    assert reach[c]["c8"]["big"] >= 64 and reach[c]["qf"][1] < 255
    # a 128 px varblock (raw id 21) with large coefficients
    r = H.oracle_ref("tri64", 0.001, CJXL8)
    assert (r.acs == 21).sum() >= 1
    assert reach[("tri64", 0.001, CJXL8)]["merged"]["big"] >= 1
    assert reach[("tri64", 0.001, PLAIN7)]["merged"]["big"] >= 16
    # X and B in the top token class
    c = ("corners72", 0.001, CJXL7)
    assert min(reach[c]["c8"]["max"]) >= 16384
    # everywhere else only Y gets there
    for c in H.CASES:
        if c[0] != "corners72":
            for cls in ("c8", "merged"):
                assert max(reach[c][cls]["max"][0], reach[c][cls]["max"][2]) < 16384, c


# ---------------------------------------------------------------------------
# the bottom of the distance range
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["white72", "half264"])
@pytest.mark.parametrize("setting", [CJXL7, PLAIN5], ids=H.setting_id)
def test_below_the_floor_is_the_floor(oracle, name, setting):
    ref = H.oracle_ref(name, H.FLOOR, setting)
    for d in BELOW_FLOOR:
        assert np.float32(d) > 0
        got = oracle.encode(H.images()[name], d, *setting)
        assert got.bytes == ref.bytes, (name, d)
        assert (got.global_scale, got.quant_dc) == (ref.global_scale, ref.quant_dc)
        assert np.array_equal(got.qf, ref.qf), (name, d)


@pytest.mark.parametrize("setting", H.SETTINGS, ids=H.setting_id)
def test_every_clamp_is_reached_well_above_the_floor(oracle, setting):
    """1e-4 and 1e-5 give the bytes of 1e-6: every quantity that depends on the
    distance is at its clamp there, so the floor changes no codestream of a
    distance that behaved before"""
    for name, img in H.images().items():
        ref = H.oracle_ref(name, H.FLOOR, setting)
        assert ref.global_scale == H.G_CLAMP and (ref.qf == 255).all(), name
        for d in (1e-4, 1e-5, 1e-9):
            assert oracle.encode(img, d, *setting).bytes == ref.bytes, (name, d)


def test_refused_distances_stay_refused(oracle):
    img = H.images()["white72"]
    for d in (0.0, -0.0, -1e-6, -1.0, float("nan"), 25.000002, float("inf")):
        with pytest.raises(RuntimeError):
            oracle.encode(img, d, 7, 0)
    oracle.encode(img, 25.0, 7, 0)


@pytest.mark.parametrize("setting", [PLAIN7, PLAIN5], ids=H.setting_id)
def test_quality_does_not_collapse(oracle, decoder, setting):
    """white noise, plain preset: the error at a smaller distance is never above
    the error at 0.001 (MSE ~0.006 down there; it was 119 at 1e-10 and 5554 at
    1e-17 before the floor)"""
    img = H.images()["white72"]
    at = oracle.encode(img, 0.001, *setting)
    mse_at, _ = decoder.mse_psnr(img, decoder.decode(at.bytes).rgb)
    for d in (H.FLOOR,) + BELOW_FLOOR:
        r = oracle.encode(img, d, *setting)
        mse, _ = decoder.mse_psnr(img, decoder.decode(r.bytes).rgb)
        print("white72 %s d %g: %d bytes, MSE %.6f (0.001: %d bytes, %.6f)" % (
            H.setting_id(setting), d, len(r.bytes), mse, len(at.bytes), mse_at))
        assert mse <= mse_at, d
        assert len(r.bytes) >= len(at.bytes), d


def test_finest_field_under_cjxl_defaults(oracle):
    """cjxl's preset on white noise: its decoded error sits near MSE 55 at any
    distance (the encoder-side inverse Gaborish on noise, clipped on the way
    back: 55.228 at 0.001, 55.240 at 1e-6), so it is no measure of the
    quantizer; what must not collapse is the field itself: the raw quant field
    is at its ceiling from the floor down and as many coefficients survive as
    at 0.001, where the masking field is still below the ceiling"""
    img = H.images()["white72"]
    at = H.oracle_ref("white72", 0.001, CJXL7)
    for d in (H.FLOOR,) + BELOW_FLOOR:
        r = oracle.encode(img, d, *CJXL7)
        assert (r.qf == 255).all() and r.global_scale == H.G_CLAMP, d
        assert (r.ac != 0).sum() >= (at.ac != 0).sum(), d
        assert np.abs(r.ac).sum() >= np.abs(at.ac).sum(), d


# ---------------------------------------------------------------------------
# the token record's edge
# ---------------------------------------------------------------------------
def test_token_formula_at_the_edges():
    tok, nbits, bits, top2 = H.token_of([1, -1, 7, -8, 8, 16383, 16384, -16384, 32767, -32767])
    assert tok.tolist() == [2, 1, 14, 15, 16, 59, 60, 59, 63, 63]
    assert nbits.tolist() == [0, 0, 0, 0, 2, 12, 13, 12, 13, 13]
    assert bits.tolist()[-2:] == [0x1FFE, 0x1FFD] and top2.tolist()[-2:] == [3, 3]
    # the record's fields hold the edge exactly: 6 bits of token, 4 of nbits, 14 of bits
    assert tok.max() < 1 << 6 and nbits.max() < 1 << 4 and bits.max() < 1 << 14


def test_widest_token_occurs():
    seen = set()
    for case in H.CASES:
        q = H.oracle_ref(*case).ac
        tok, nbits, bits, top2 = H.token_of(q[q != 0])
        top = tok >= 60
        assert (nbits[top] == 13).all() and (nbits[~top] < 13).all()
        seen |= set(top2[top].tolist())
        if REACH[case]["c8"]["sat"] + REACH[case]["merged"]["sat"]:
            assert (tok == 63).any(), case
            assert bits[np.abs(q[q != 0]) == 32767].min() >= 0x1FFD
    assert seen == {0, 1, 2, 3}


def test_dense_block_occurs():
    """white72: 8x8-class blocks with all 63 AC coefficients non-zero, in Y
    (the non-zero count's largest token of an 8x8 block)"""
    for setting in (CJXL7, PLAIN7):
        r = H.oracle_ref("white72", 0.001, setting)
        nz = (r.ac[:, :, :, 1:] != 0).sum(axis=3)
        assert not r.ac[:, :, :, 0].any()  # slot 0 is the DC image's
        c8, _ = H.class_masks(r.acs)
        assert (nz[c8][:, 1] == 63).any(), setting
    tok, nbits, _, _ = H.token_of(-32)  # (packs to 63, the count's value)
    assert (int(tok), int(nbits)) == (23, 3)


# ---------------------------------------------------------------------------
# oracle -> Python decoder
# ---------------------------------------------------------------------------
def _assert_read_back(d, r, what):
    assert np.array_equal(d.acs, r.acs), what
    assert np.array_equal(d.qf - 1, r.qf), what
    assert np.array_equal(d.dc, r.dc), what
    assert np.array_equal(d.ac, r.ac), what
    assert np.array_equal(d.ac_tokens, r.ac_tokens), what
    assert (d.global_scale, d.quant_dc) == (r.global_scale, r.quant_dc), what


@pytest.mark.parametrize("case", H.ALL_CASES, ids=H.case_id)
def test_round_trip(oracle, decoder, case):
    name, dist, (e, p, coder, mask) = case
    r = H.oracle_ref(*case)
    _assert_read_back(H.decoded(*case), r, "own coder")
    other = oracle.encode(H.images()[name], dist, e, p, 1 - coder, mask)
    assert np.array_equal(other.ac, r.ac) and other.bytes != r.bytes
    _assert_read_back(decoder.decode(other.bytes, want_pixels=False), other, "other coder")


# ---------------------------------------------------------------------------
# the reference of the pixel comparisons
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.RECON_CASES, ids=H.case_id)
def test_reference_self_difference(case):
    ref = H.reference_rgb(*case)
    f32 = crafted.reconstruct_f32(H.decoded(*case))
    worst, share, tile = crafted.tile_shares(ref, f32)
    print("self-difference %s: max %d, share %.3g, worst tile %.3g" % (
        H.case_id(case), worst, share, tile))
    assert worst <= 1
    assert share <= H.RECON_MAX_SHARE / 10
