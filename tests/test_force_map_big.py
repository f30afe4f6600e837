"""The forced encode's map validator and the kinds of 128 / 256 px (raw ids
21 - 26; csrc/jxg_force.cpp): accepted as first blocks on the
shape's own grid -- block row a multiple of its blocks down, block column a
multiple of its blocks across -- and nowhere else.  Run through the stand-alone
program of tests/test_force_map.py (g++ from jxg_force.cpp alone, ASan + UBSan
where the compiler has them).  What the validator must say is written down per
case: the status and the first offending block in raster order.

b1_map / b2_map are the crafted maps tests/test_gpu_forced_big.py encodes."""
import numpy as np
import pytest

import crafted
from test_force_map import INVALID, OK, UNSUPPORTED, blank, force_map, put, rotated  # noqa: F401

BIG = crafted.BIG_SHAPES  # id -> (blocks down, blocks across)


def gradient_rgb8(w, h, seed):
    """the generator of tests/test_gpu_bigvb.py"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 60 * np.sin(x / rng.uniform(150, 400) + y / rng.uniform(150, 400) + c)
                    for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


# the frames whose effort-8 search maps are forced back: w, h, distance, coder
# (0 prefix codes, 1 ANS), the oracle's filters mask (7: cjxl's defaults)
OWN_MAP_FRAMES = ((512, 512, 1.0, 1, 0), (768, 520, 2.0, 0, 0), (1024, 1024, 1.0, 1, 0),
                  (600, 300, 1.0, 1, 7))


def own_grid(t, by0, bx0, rows, cols):
    """every own-grid position of id t in the block rectangle at (by0, bx0)"""
    cy, cx = BIG[t]
    return [(t, by, bx) for by in range(by0, by0 + rows - cy + 1, cy)
            for bx in range(bx0, bx0 + cols - cx + 1, cx)]


# B1 (512 x 512: four pass groups): a 24 in group 0; two 25 in group 1; two 26
# in group 2; in group 3 a 21, two 22 and two 23, the remaining 128 x 128 filled
# with the 64 px shapes and the 8x8-class rotation
B1_HEADS = ((24, 0, 0), (25, 0, 32), (25, 0, 48), (26, 32, 0), (26, 48, 0),
            (21, 32, 32), (22, 32, 48), (22, 32, 56), (23, 48, 32), (23, 56, 32),
            (18, 48, 48), (19, 48, 56), (19, 48, 60), (20, 56, 48), (20, 60, 48))
# B2 (648 x 392: 81 x 49 blocks, a third group column of 17 blocks and a second
# group row of 17): what fits flush in the partial groups -- 21, 22 and 23 at
# column 64, 22 also at column 72; the same down the bottom row -- and big
# kinds in the two whole groups
B2_HEADS = ((21, 0, 64), (22, 16, 64), (22, 16, 72), (23, 32, 64), (23, 40, 64),
            (21, 32, 0), (22, 32, 16), (22, 32, 24), (23, 32, 32), (23, 40, 32), (21, 32, 48),
            (24, 0, 0), (26, 0, 32), (23, 16, 32), (23, 24, 32), (22, 16, 48), (22, 16, 56))
# B3 (the same frame): what else fits there -- placements the validator's rule
# admits and the search never produces (it merges whole 128 / 256 px squares)
B3_HEADS = ((25, 0, 64), (26, 32, 0), (26, 32, 32), (22, 32, 64), (22, 32, 72))


def crafted_map(bys, bxs, heads, shift=0):
    acs = np.full((bys, bxs), 255, np.uint8)
    for t, by, bx in heads:
        crafted.place(acs, t, by, bx)
    return rotated(acs, shift)


def b1_map():
    return crafted_map(64, 64, B1_HEADS)


def b2_map():
    return crafted_map(49, 81, B2_HEADS, 1)


def b3_map():
    return crafted_map(49, 81, B3_HEADS, 2)


def test_the_crafted_maps_hold_what_they_are_for():
    b1 = crafted.heads_of(b1_map())
    count = {t: sum(1 for h in b1 if h[0] == t) for t in BIG}
    assert count == {24: 1, 25: 2, 26: 2, 21: 1, 22: 2, 23: 2}
    assert set(crafted.CLASS8) <= {h[0] for h in b1} and {18, 19, 20} <= {h[0] for h in b1}
    b2 = [h for h in crafted.heads_of(b2_map()) if h[0] in BIG]
    assert sorted(h for h in b2 if h[2] >= 64) == sorted(
        [(21, 0, 64), (22, 16, 64), (22, 16, 72), (23, 32, 64), (23, 40, 64)])
    assert {h[0] for h in b2 if h[1] >= 32} == {21, 22, 23}
    for t, by, bx in b2:
        cy, cx = BIG[t]
        assert by % cy == 0 and bx % cx == 0


def accepted_cases(oracle):
    """[(name, w, h, map)]"""
    out = []
    # every own-grid position of one pass group (the last) of a 512 x 512 frame
    n = 0
    for t in sorted(BIG):
        for _, by, bx in own_grid(t, 32, 32, 32, 32):
            out.append(("own_grid_%d_%d_%d" % (t, by, bx), 512, 512,
                        crafted_map(64, 64, [(t, by, bx)], n)))
            n += 1
    assert n == 4 + 8 + 8 + 1 + 2 + 2
    out.append(("b1", 512, 512, b1_map()))
    # the partial groups of 648 x 392: one map per placement that fits, and B2
    for t, by, bx in B2_HEADS[:11]:
        out.append(("partial_%d_%d_%d" % (t, by, bx), 648, 392, crafted_map(49, 81, [(t, by, bx)], n)))
        n += 1
    for t, by, bx in B3_HEADS + ((21, 32, 64),):
        out.append(("partial_%d_%d_%d" % (t, by, bx), 648, 392, crafted_map(49, 81, [(t, by, bx)], n)))
        n += 1
    out.append(("b2", 648, 392, b2_map()))
    out.append(("b3", 648, 392, b3_map()))
    # the search's own choice (the oracle's effort-8 encodes)
    seen = set()
    for w, h, d, coder, filt in OWN_MAP_FRAMES:
        acs = oracle.encode(gradient_rgb8(w, h, w * 7 + h), d, 8, 0, coder, filt).acs
        seen |= {t for t, _, _ in crafted.heads_of(acs)}
        out.append(("oracle_e8_%dx%d" % (w, h), w, h, acs))
    assert set(BIG) <= seen, sorted(seen)
    return out


def test_accepted_maps(force_map, oracle):
    cases = accepted_cases(oracle)
    got = force_map(cases)
    bad = [(c[0], g) for c, g in zip(cases, got) if g != (OK, 0)]
    assert not bad, bad[:10]


def refused_maps():
    """[(name, w, h, map, status, first offending block)]"""
    out = []
    # on its grid, one block past the right edge, the bottom edge, the corner
    for name, w, h, by, bx in (("past_right_edge", 248, 256, 0, 16), ("past_bottom_edge", 256, 248, 16, 0),
                               ("past_corner", 248, 248, 16, 16)):
        acs = blank(w, h, 0)
        put(acs, 21, by, bx)
        out.append((name, w, h, acs, INVALID, by * ((w + 7) // 8) + bx))
    # ... and what the partial groups of 648 x 392 (81 x 49 blocks) do not hold
    for t, by, bx in ((24, 0, 64), (26, 0, 64), (24, 32, 0), (25, 32, 16), (26, 32, 64), (23, 32, 80),
                      (22, 0, 80), (21, 0, 80), (21, 48, 0), (22, 48, 8), (23, 48, 16)):
        acs = blank(648, 392, 0)
        put(acs, t, by, bx)
        out.append(("partial_group_%d_%d_%d" % (t, by, bx), 648, 392, acs, INVALID, by * 81 + bx))
    # cover bytes: a wrong one inside, an orphan, a first block inside
    acs = blank(256, 256, 0)
    put(acs, 21, 0, 0)
    acs[5, 5] = 0x80 | 24
    out.append(("cover_of_another_id", 256, 256, acs, INVALID, 5 * 32 + 5))
    acs = blank(256, 256, 0)
    acs[16, 16] = 0x80 | 21
    out.append(("orphan_cover", 256, 256, acs, INVALID, 16 * 32 + 16))
    acs = blank(256, 256, 0)
    put(acs, 21, 0, 0)
    acs[0, 16] = 0x80 | 21
    out.append(("orphan_beside_varblock", 256, 256, acs, INVALID, 16))
    acs = blank(256, 256, 0)
    put(acs, 24, 0, 0)
    acs[6, 5] = 0
    out.append(("first_block_inside", 256, 256, acs, INVALID, 6 * 32 + 5))
    # overlap with a tile shape declared after the big varblock's first block: a
    # first block inside it ...
    acs = blank(256, 256, 0)
    put(acs, 21, 16, 0)
    put(acs, 4, 20, 3)
    out.append(("tile_shape_inside", 256, 256, acs, INVALID, 20 * 32 + 3))
    # ... and declared before it: the big grid lies on tile borders, so a tile
    # shape reaches a big varblock from outside only across its tile, and its own
    # first block is the first offence in raster order
    for name, bbx, t, by, bx in (("tile_shape_from_above", 0, 6, 15, 2),
                                 ("tile_shape_from_the_left", 16, 7, 18, 15)):
        acs = blank(256, 256, 0)
        put(acs, 21, 16, bbx)
        put(acs, t, by, bx)
        out.append((name, 256, 256, acs, INVALID, by * 32 + bx))
    # two big varblocks: the second's first block inside the first, and both
    # claiming one block -- 22 (16 x 8) at (0, 8) and 23 (8 x 16) at (8, 0) meet at (8, 8)
    acs = blank(256, 256, 0)
    put(acs, 22, 0, 0)
    put(acs, 23, 8, 0)
    out.append(("big_first_block_inside_big", 256, 256, acs, INVALID, 8 * 32))
    for last in (22, 23):
        acs = blank(256, 256, 0)
        for t, by, bx in ((23, 8, 0), (22, 0, 8)) if last == 22 else ((22, 0, 8), (23, 8, 0)):
            put(acs, t, by, bx)
        out.append(("big_shared_block_%d" % last, 256, 256, acs, INVALID, 8 * 32 + 8))
    # off its own grid, on the 64 px grid, with room in the frame
    for t, by, bx in ((21, 8, 8), (21, 0, 8), (21, 16, 24), (24, 0, 16), (24, 16, 0), (24, 8, 8),
                      (22, 8, 0), (22, 24, 8), (23, 0, 8), (23, 8, 24), (25, 0, 8), (25, 16, 0),
                      (26, 0, 16), (26, 8, 0)):
        acs = blank(512, 512, 0)
        put(acs, t, by, bx)
        out.append(("off_grid_%d_%d_%d" % (t, by, bx), 512, 512, acs, UNSUPPORTED, by * 64 + bx))
    # ... and off the 64 px grid
    acs = blank(512, 512, 0)
    put(acs, 21, 3, 5)
    out.append(("off_grid_21_3_5", 512, 512, acs, UNSUPPORTED, 3 * 64 + 5))
    # the order of the checks on a first block: claimed, then placement, then the fit
    acs = blank(128, 128, 0)
    put(acs, 21, 8, 8)  # off its grid and past the frame
    out.append(("off_grid_before_fit", 128, 128, acs, UNSUPPORTED, 8 * 16 + 8))
    acs = blank(512, 512, 0)
    put(acs, 24, 0, 0)
    acs[8, 8] = 21  # claimed and off its grid
    out.append(("claimed_before_off_grid", 512, 512, acs, INVALID, 8 * 64 + 8))
    # AFV, 32X8 / 8X32 and ids past the last stay refused, on any grid
    for t in (8, 9, 14, 15, 16, 17, 27):
        for by, bx in ((0, 0), (32, 32)):
            acs = blank(512, 512, 0)
            acs[by, bx] = t
            out.append(("id_%d_at_%d" % (t, by), 512, 512, acs, UNSUPPORTED, by * 64 + bx))
    return out


def test_refused_maps_name_the_status_and_the_first_offending_block(force_map):
    cases = refused_maps()
    got = force_map([c[:4] for c in cases])
    wrong = [(c[0], g, c[4:]) for c, g in zip(cases, got) if g != tuple(c[4:])]
    assert not wrong, wrong


def test_make_strategy_map_places_the_big_kinds(jxg_mod, force_map):
    jxg = jxg_mod
    assert {t: jxg.FORCED_SHAPES[t] for t in BIG} == BIG
    for bys, bxs, heads, shift in ((64, 64, B1_HEADS, 0), (49, 81, B2_HEADS, 1)):
        acs = jxg.make_strategy_map(bys, bxs, heads, fill=12)
        ref = np.full((bys, bxs), 255, np.uint8)
        for t, by, bx in heads:
            crafted.place(ref, t, by, bx)
        ref[ref == 255] = 12
        assert acs.dtype == np.uint8 and np.array_equal(acs, ref)
        assert sorted(h for h in crafted.heads_of(acs) if h[0] != 12) == sorted(heads)
        assert force_map([("made", bxs * 8, bys * 8, acs)]) == [(OK, 0)]
    # off its grid the map is made, and the validator's to refuse
    acs = jxg.make_strategy_map(64, 64, [(21, 8, 8)])
    assert force_map([("made_off_grid", 512, 512, acs)]) == [(UNSUPPORTED, 8 * 64 + 8)]
    with pytest.raises(ValueError):
        jxg.make_strategy_map(64, 64, [(24, 0, 0), (21, 16, 16)])  # overlap
    with pytest.raises(ValueError):
        jxg.make_strategy_map(31, 32, [(21, 16, 0)])  # past the map
    with pytest.raises(ValueError):
        jxg.make_strategy_map(64, 64, [(27, 0, 0)])  # not an accepted id
    with pytest.raises(ValueError):
        jxg.make_strategy_map(64, 64, [], fill=21)  # not an 8x8-class fill
