"""CPU tests of the crafted codestreams (tests/crafted.py): streams written
from hand-made maps by the oracle's encode_maps, holding every varblock
placement the decoder accepts -- which no stream encoded from an image does.

  - encode_maps is the second half of the oracle encoder: from an encode's own
    maps it writes that encode's bytes, and it refuses maps that are not one
    consistent frame, each kind with its own code;
  - the float64 oracle decoder and the product's host path (csrc/jxg_decode.cpp
    + the decode core the GPU kernel shares) both return the crafted maps
    exactly, for every stream of S1 - S4;
  - a coefficient of 32768 (S5) is JXG_ERR_INVALID_ARG, a placement across a
    tile or a pass group JXG_ERR_UNSUPPORTED, both from the host parse;
  - the reference image of S1 - S3 stays in the gamut (fewer than 5 % of its
    samples are 0 or 255; measured: at most 1.9 %), so the pixel comparison of
    tests/test_gpu_crafted.py compares values, not clipping;
  - sensitivity: a decoder wrong in one small way (a tall shape's coefficients
    transposed, a coefficient one slot on, a varblock one block off, a tile's
    ytox / ytob or a varblock's qf off by one) moves a sample of that tile by 2
    or more in the float64 reference -- more than the pixel bound lets through;
  - the reference rounded to f32 between its stages differs from itself by at
    most 1, on less than a fifth of the per-tile cap of the pixel comparison.

Measured, sensitivity (the smallest move over s1_1, s2_128x64, s3_72x200_0):
transposed 29, next slot 4, shifted 15, ytox +-1 13, ytob +-1 2, qf +-1 4.
"""
import numpy as np
import pytest

import crafted
from test_recon_cases import CASES, case_image

INVALID_ARG, UNSUPPORTED = -1, -5

ALL = crafted.all_cases
ROUND_TRIP = ("natural_d1.5_epf", "natural_d12_all", "gradient_e8", "gradient_e8_all",
              "natural_prefix")


def _status(jxg_mod, data):
    return jxg_mod.load().jxg_decode_maps(None, data, len(data), None, None, None, None, None)


@pytest.mark.parametrize("name", ROUND_TRIP)
def test_encode_maps_of_an_encodes_maps_is_that_encode(oracle, name):
    """prefix codes and ANS, with and without the 128 / 256 px shapes and filters"""
    case = next(c for c in CASES if c[0] == name)
    d, e, p, coder, mask = case[5:]
    ref = oracle.encode(case_image(case), d, e, p, coder, mask)
    got = oracle.encode_maps(case[2], case[3], ref.acs, ref.qf, ref.dc, ref.ac, ref.cmap, d, coder,
                             mask)
    assert got.bytes == ref.bytes
    assert np.array_equal(got.ac_tokens, ref.ac_tokens)
    assert (got.global_scale, got.quant_dc) == (ref.global_scale, ref.quant_dc)


def test_round_trip_set_has_both_coders_and_big_shapes(oracle):
    cases = [next(c for c in CASES if c[0] == n) for n in ROUND_TRIP]
    assert {c[8] for c in cases} == {0, 1}
    assert {c[6] >= 8 for c in cases} == {False, True}


def _maps(case):
    return [getattr(case, k).copy() for k in crafted.MAPS]


def _refusal(oracle, case, edit):
    acs, qf, dc, ac, cmap = _maps(case)
    edit(acs, qf, dc, ac, cmap)
    with pytest.raises(oracle.MapsError) as e:
        oracle.encode_maps(case.w, case.h, acs, qf, dc, ac, cmap, case.distance, case.coder,
                           case.filters)
    return e.value.code


def test_encode_maps_refuses_inconsistent_maps(oracle):
    """a 64x64 px frame with a 16x16 px varblock at block (1, 3) and a 16x32 px one at (5, 2)"""
    case = crafted.make_case("consistent", "S4", 64, 64, 6.0, 1, 0, [(4, 1, 3), (11, 5, 2)], 700)
    oracle.encode_maps(case.w, case.h, *_maps(case), case.distance, case.coder, case.filters)

    def edit(fn):
        return _refusal(oracle, case, fn)

    def put(name, idx, v):
        def fn(acs, qf, dc, ac, cmap):
            dict(acs=acs, qf=qf, dc=dc, ac=ac, cmap=cmap)[name][idx] = v
        return fn

    for bad in (8, 9, 14, 17, 27, 0x7F):
        assert edit(put("acs", (0, 0), bad)) == oracle.MAPS_ID, bad
    # a 16x16 head in the last column / row; a 64x64 head at block (0, 1)
    assert edit(put("acs", (0, 7), 4)) == oracle.MAPS_FIT
    assert edit(put("acs", (7, 0), 6)) == oracle.MAPS_FIT
    assert edit(put("acs", (0, 1), 18)) == oracle.MAPS_FIT
    # cover flags: one missing, one of another id, one nobody owns, a head inside a varblock
    assert edit(put("acs", (2, 4), 0)) == oracle.MAPS_COVER
    assert edit(put("acs", (2, 4), 0x80 | 5)) == oracle.MAPS_COVER
    assert edit(put("acs", (0, 0), 0x80 | 4)) == oracle.MAPS_COVER
    assert edit(put("acs", (0, 2), 4)) == oracle.MAPS_COVER  # reaches into the one at (1, 3)
    assert edit(put("qf", (6, 5), int(case.qf[5, 2]) ^ 1)) == oracle.MAPS_QF
    # the DC slot of an 8x8-class block, the 4 / 8 LLF slots of the merged ones
    assert edit(put("ac", (0, 0, 1, 0), 1)) == oracle.MAPS_LLF
    assert edit(put("ac", (1, 3, 0, 3), -1)) == oracle.MAPS_LLF
    assert edit(put("ac", (5, 2, 2, 7), 5)) == oracle.MAPS_LLF
    maps = _maps(case)
    maps[3][5, 2, 2, 8] = 5  # slot 8 of a 2x4-block shape is a coefficient
    oracle.encode_maps(case.w, case.h, *maps, case.distance, case.coder, case.filters)
    assert edit(put("dc", (1, 3, 3), oracle.MAPS_DC_MAX + 1)) == oracle.MAPS_DC_RANGE
    assert edit(put("dc", (0, 0, 0), oracle.MAPS_DC_MIN - 1)) == oracle.MAPS_DC_RANGE
    assert len({oracle.MAPS_ID, oracle.MAPS_FIT, oracle.MAPS_COVER, oracle.MAPS_QF,
                oracle.MAPS_LLF, oracle.MAPS_DC_RANGE, oracle.MAPS_BAD_ARG}) == 7


def test_families_hold_what_they_claim():
    fam = crafted.families()
    # S1: each of the 267 placements of the nine shapes once, and every 8x8-class id at
    # every block position of a tile
    seen = set()
    at = {t: np.zeros((8, 8), bool) for t in crafted.CLASS8}
    for c in fam["S1"]:
        assert (c.w, c.h) == (512, 512)
        seen |= {(t, by % 8, bx % 8) for t, by, bx in c.heads}
        for t in crafted.CLASS8:
            ys, xs = np.nonzero(c.acs == t)
            at[t][ys % 8, xs % 8] = True
    assert seen == set(crafted.s1_placements()) and len(seen) == 267
    assert all(m.all() for m in at.values())
    assert {(c.coder, bool(c.filters)) for c in fam["S1"]} == {(0, False), (0, True), (1, False),
                                                               (1, True)}
    # S2: the offsets inside the pass group
    off = {}
    for c in fam["S2"]:
        for t, by, bx in c.heads:
            off.setdefault(t, set()).add((by % 32, bx % 32))
    assert off[21] >= {(0, 0), (16, 16), (3, 5), (16, 7)}
    assert off[22] >= {(0, 0), (16, 24)} and any(y % 8 and x % 8 for y, x in off[22])
    assert off[23] >= {(0, 0), (24, 16)} and any(y % 8 and x % 8 for y, x in off[23])
    assert off[24] == {(0, 0)}
    assert off[25] == {(0, 0), (0, 7), (0, 16)} and off[26] == {(0, 0), (7, 0), (16, 0)}
    assert any(c.filters == 3 for c in fam["S2"])
    # S3: every placement is flush with an edge; Gaborish and three EPF passes
    for c in fam["S3"]:
        bys, bxs = c.acs.shape
        assert (bys, bxs) in ((25, 9), (9, 25), (28, 12), (12, 28)) and c.filters == 3 and c.distance >= 4.0
        for t, by, bx in c.heads:
            cy, cx = crafted.shape_of(t)
            assert by + cy == bys or bx + cx == bxs
    corners = [(t, c.acs.shape) for c in fam["S3"] for t, by, bx in c.heads
               if (by + crafted.shape_of(t)[0], bx + crafted.shape_of(t)[1]) == c.acs.shape]
    assert {s for _, s in corners} == {(25, 9), (9, 25), (28, 12), (12, 28)}
    # flush with an edge somewhere: the shapes up to 32 px, 64x32 / 32x64 and 128x64 / 64x128
    assert {t for c in fam["S3"] for t, _, _ in c.heads} == {4, 5, 6, 7, 10, 11, 19, 20, 22, 23}
    # every accepted placement obeys the decoder's rule
    for c in ALL():
        for t, by, bx in c.heads:
            assert crafted.accepted(t, by, bx, *c.acs.shape), (c.name, t, by, bx)
    # S4
    s4 = {c.name: c for c in fam["S4"]}
    assert np.count_nonzero(s4["s4_dense64"].ac) == 3 * 4032
    assert np.count_nonzero(s4["s4_dense8"].ac) == 64 * 3 * 63
    assert {32767, -32767, -32768} <= set(np.unique(s4["s4_int16"].ac))
    assert set(np.unique(s4["s4_qf"].qf)) == {0, 255} and s4["s4_qf"].filters & 2
    assert {-128, 127} == set(np.unique(s4["s4_cmap"].cmap))
    assert s4["s4_dc"].dc.min() == -(1 << 29) and s4["s4_dc"].dc.max() == (1 << 29) - 1


@pytest.mark.parametrize("case", ALL(), ids=[c.name for c in ALL()])
def test_maps_come_back_exactly(jxg_mod, decoder, case):
    data = crafted.stream(case)
    ref = crafted.decoded_maps(decoder.decode(data, want_pixels=False))
    host = jxg_mod.decode_maps(data)
    for k in crafted.MAPS:
        want = getattr(case, k)
        assert ref[k].shape == want.shape and np.array_equal(ref[k], want), "oracle decoder: " + k
        assert host[k].shape == want.shape and np.array_equal(host[k], want), "host path: " + k
    info = jxg_mod.stream_info(data)
    assert (info["xsize"], info["ysize"]) == (case.w, case.h)
    assert info["num_groups"] == jxg_mod.group_count(case.w, case.h)
    assert info["num_lf_groups"] == 1 and info["num_hf_presets"] == 1
    assert info["ans"] == case.coder
    assert info["gaborish"] == (case.filters & 1)
    assert info["epf_iters"] == (0 if not case.filters & 2 else (2 if case.distance < 4 else 3))
    assert (info["global_scale"], info["quant_dc"]) == (case.global_scale, case.quant_dc)


def test_a_coefficient_outside_int16_is_invalid(jxg_mod, decoder):
    case = crafted.s5_case()
    data = crafted.stream(case)
    # the stream itself is sound: the oracle decoder reads the maps back, 32768 included
    ref = crafted.decoded_maps(decoder.decode(data, want_pixels=False))
    assert np.array_equal(ref["ac"], case.ac) and case.ac.max() == 32768
    assert _status(jxg_mod, data) == INVALID_ARG
    case.ac[case.ac == 32768] = 32767
    assert _status(jxg_mod, crafted.stream(case, cache=False)) == 0


@pytest.mark.parametrize("case", crafted.refused_cases(), ids=lambda c: c.name)
def test_placements_across_a_cell_are_unsupported(jxg_mod, decoder, case):
    """2x2 blocks at (7, 7) cross a tile, 16x16 at (24, 24) a pass group, 8x8 at (1, 0)
    a tile: sound streams (the oracle decoder takes them) the host parse refuses"""
    assert not crafted.accepted(*case.heads[0], *case.acs.shape)
    data = crafted.stream(case)
    ref = crafted.decoded_maps(decoder.decode(data, want_pixels=False))
    for k in crafted.MAPS:  # (ac: the non-zero predictor across the cell's border agrees)
        assert np.array_equal(ref[k], getattr(case, k)), k
    assert _status(jxg_mod, data) == UNSUPPORTED


@pytest.mark.parametrize("case", crafted.pixel_cases(), ids=lambda c: c.name)
def test_reference_image_stays_in_the_gamut(case):
    d, seconds = crafted.reference(case)
    share = float(np.mean((d.rgb == 0) | (d.rgb == 255)))
    print("%s: %.2f %% of the samples at 0 / 255, reference %.1f s" % (case.name, 100 * share,
                                                                      seconds))
    assert d.rgb.shape == (case.h, case.w, 3)
    assert share < 0.05



# ---------------------------------------------------------------------------
# what the pixel comparison can and cannot see
# ---------------------------------------------------------------------------
PER_TILE_CAP = 0.005  # tests/test_gpu_crafted.py MAX_SHARE


def _probed_frames():
    """one frame of S1, S2 and S3 (all with Gaborish and three EPF passes)"""
    fam = crafted.families()
    return [fam["S1"][1], next(c for c in fam["S2"] if c.name == "s2_128x64"), fam["S3"][0]]


@pytest.mark.parametrize("case", _probed_frames() + [crafted.families()["S1"][0]],
                         ids=lambda c: c.name)
def test_f32_rounding_stays_far_below_the_per_tile_cap(case):
    d, _ = crafted.reference(case)
    worst, share, tile = crafted.tile_shares(d.rgb, crafted.reconstruct_f32(d))
    print("%s: f64 vs f32 between stages: max |diff| %d, share %.3g, worst tile %.3g" % (
        case.name, worst, share, tile))
    assert worst <= 1
    assert tile < PER_TILE_CAP / 5


def test_f32_rounding_is_applied(decoder):
    """reconstruct_f32 swaps jxl_decode's stage functions: they exist under these names,
    and the swap changes the planes they return"""
    for name in ("gaborish", "_epf_step", "xyb_to_srgb8"):
        assert callable(getattr(decoder, name))
    case = crafted.families()["S3"][0]
    d, _ = crafted.reference(case)
    seen = []
    saved = decoder.xyb_to_srgb8
    decoder.xyb_to_srgb8 = lambda X, Y, B: seen.append(X.copy()) or saved(X, Y, B)
    try:
        decoder.reconstruct(d)
    finally:
        decoder.xyb_to_srgb8 = saved
    saved_step = decoder._epf_step
    crafted.reconstruct_f32(d)
    assert decoder._epf_step is saved_step and decoder.xyb_to_srgb8 is saved
    # the f64 planes are not f32 values; the f32 variant's are (checked at its last stage)
    assert not np.array_equal(seen[0], seen[0].astype(np.float32).astype(np.float64))
    got = []
    decoder.xyb_to_srgb8 = lambda X, Y, B: got.append(X.copy()) or saved(X, Y, B)
    try:
        crafted.reconstruct_f32(d)
    finally:
        decoder.xyb_to_srgb8 = saved
    assert np.array_equal(got[0], got[0].astype(np.float32).astype(np.float64))


def _tall_head(case):
    """a tall merged varblock off its shape's own grid"""
    for t, by, bx in case.heads:
        cy, cx = crafted.shape_of(t)
        if cy > cx and (by % cy or bx % cx):
            return t, by, bx
    raise AssertionError("no tall off-grid varblock in " + case.name)


def _perturbations(decoder, d, t, by, bx):
    """(name, perturbed copy of the decoded frame d) for each small mistake"""
    import copy

    cy, cx = crafted.shape_of(t)
    cb = cy * cx

    def clone():
        e = copy.copy(d)
        e.acs, e.qf, e.ac, e.cmap = d.acs.copy(), d.qf.copy(), d.ac.copy(), d.cmap.copy()
        return e

    def slot(k):
        return crafted.coef_slot(by, bx, cx, k)

    pos = [(k, c) for c in range(3) for k in range(cb, 64 * cb)
           if d.ac[slot(k)[0], slot(k)[1], c, k & 63]]
    assert pos
    out = []
    # the tall shape's coefficients at (kx, ky) instead of (ky, kx), where both exist
    kind = decoder.SHAPES[t][2]
    _, nat = decoder.kind_tables(kind, getattr(d, "qm_params", {}).get(kind))
    nat = np.array(nat)
    rows, cols = decoder.KIND_DIM[kind]
    where = {int(n): k for k, n in enumerate(nat)}
    e = clone()
    moved = 0
    for k, c in pos:
        sy, sx = divmod(int(nat[k]), cols)
        if sx < rows and sx != sy:
            k2 = where[sx * cols + sy]
            if k2 >= cb:
                y, x, s_ = slot(k)
                y2, x2, s2 = slot(k2)
                e.ac[y, x, c, s_] = 0
                e.ac[y2, x2, c, s2] = d.ac[y, x, c, s_]
                moved += 1
    assert moved
    out.append(("transposed", e))
    # one Y coefficient in the next natural-order slot
    k, c = next((k, c) for k, c in pos if c == 1 and k + 1 < 64 * cb)
    e = clone()
    y, x, s_ = slot(k)
    y2, x2, s2 = slot(k + 1)
    e.ac[y, x, c, s_] = 0
    e.ac[y2, x2, c, s2] = d.ac[y, x, c, s_] + d.ac[y2, x2, c, s2]
    out.append(("next slot", e))
    # the varblock one block to the right or left, over 8x8-class blocks
    dx = next(dx for dx in (1, -1) if crafted.accepted(t, by, bx + dx, d.bys, d.bxs) and
              all(int(v) in crafted.CLASS8
                  for v in d.acs[by:by + cy, bx + cx if dx > 0 else bx - 1]))
    e = clone()
    own = d.ac[by:by + cy, bx:bx + cx].copy()
    e.acs[by:by + cy, bx:bx + cx] = 0
    e.ac[by:by + cy, bx:bx + cx] = 0
    e.acs[by:by + cy, bx + dx:bx + dx + cx] = t | 0x80
    e.acs[by, bx + dx] = t
    e.qf[by:by + cy, bx + dx:bx + dx + cx] = d.qf[by, bx]
    e.ac[by:by + cy, bx + dx:bx + dx + cx] = own
    out.append(("shifted by one block", e))
    for i, what in ((0, "ytox"), (1, "ytob")):
        for step in (1, -1):
            e = clone()
            e.cmap[i, by // 8, bx // 8] += step
            out.append(("cmap %s %+d" % (what, step), e))
    for step in (1, -1):
        e = clone()
        e.qf[by:by + cy, bx:bx + cx] += step  # (the decoder's qf is raw: 1 .. 256)
        assert 1 <= e.qf[by, bx] <= 256
        out.append(("qf %+d" % step, e))
    return out


@pytest.mark.parametrize("case", _probed_frames(), ids=lambda c: c.name)
def test_small_mistakes_move_the_reference_by_two_or_more(decoder, case):
    d, _ = crafted.reference(case)
    t, by, bx = _tall_head(case)
    ty, tx = by // 8, bx // 8
    base = d.rgb.astype(np.int32)
    for what, e in _perturbations(decoder, d, t, by, bx):
        diff = np.abs(decoder.reconstruct(e).astype(np.int32) - base)
        moved = int(diff[ty * 64:ty * 64 + 64, tx * 64:tx * 64 + 64].max())
        print("%s, id %d at (%d, %d), %s: a sample of its tile moves by %d" % (
            case.name, t, by, bx, what, moved))
        assert moved >= 2, what
