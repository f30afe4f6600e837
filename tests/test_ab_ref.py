"""tests/ab_ref.py, the reference of the A/B report, pinned on
the CPU: a hand-made known answer, the dims table against the oracle's maps,
the properties of the report on oracle-encoded pairs, and the input condition
of the pairs tests/test_gpu_ab_report.py runs."""
import numpy as np
import pytest

import ab_ref
import rate_ref
from test_recon_cases import COVERAGE, case_image, gradient_rgb8

C = 0x80  # a covered, non-first block
KEYS = ("blocks", "pixels", "sse_a", "sse_b", "cost_a", "cost_b")

# name, image (generator, w, h, seed), then per side distance, effort, proposals,
# coder (1 ANS), filter mask -- the pairs of the GPU tests
_ALL = 7
PAIRS = [
    ("natural_hooks", ("natural", 200, 136, 6), (1.0, 7, 0, 1, _ALL), (1.0, 7, 3, 1, _ALL)),
    ("natural_prefix", ("natural", 333, 222, 8), (2.0, 7, 0, 0, _ALL), (2.0, 7, 3, 0, _ALL)),
    ("synth_edges_f", ("synth", 520, 264, 0x4A584C31), (1.0, 7, 0, 1, _ALL), (1.0, 7, 2, 1, _ALL)),
    ("gradient_e7_e8", ("gradient", 512, 512, 512 * 7 + 512), (1.0, 7, 0, 1, _ALL),
     (1.0, 8, 0, 1, _ALL)),
    ("natural_d1_d4", ("natural", 200, 136, 5), (1.0, 7, 0, 1, _ALL), (4.0, 7, 0, 1, _ALL)),
]


def pair_image(pair):
    gen, w, h, seed = pair[1]
    if gen == "gradient":
        return gradient_rgb8(w, h, seed)
    from jxg import synth

    return (synth.natural_rgb8 if gen == "natural" else synth.synth_rgb8)(w, h, seed)


def test_known_answer():
    """30 x 20 px, 4 x 3 blocks.  A: one DCT16X32 (4 across, 2 down) of cost 7
    -- less than its 8 blocks -- over 8x8 blocks; B: two DCT16X16 of costs 5 and
    1030 (1030 % 4 = 2) over 8x8 blocks"""
    acs_a = np.array([[11, 11 | C, 11 | C, 11 | C], [11 | C] * 4, [0, 0, 2, 0]], np.uint8)
    acs_b = np.array([[4, 4 | C, 4, 4 | C], [4 | C] * 4, [0, 1, 0, 3]], np.uint8)
    cost_a = np.array([[7, 0, 0, 0], [0, 0, 0, 0], [100, 0, 513, 77]], np.uint32)
    cost_b = np.array([[5, 0, 1030, 0], [0, 0, 0, 0], [9, 300, 0, 65536]], np.uint32)
    sse_a = np.array([[1, 11, 21, 31], [41, 51, 61, 71], [81, 91, 101, 111]], np.uint32)
    sse_b = np.array([[3, 10, 17, 24], [31, 38, 45, 52], [59, 66, 73, 80]], np.uint32)
    r = ab_ref.reference(acs_a, acs_b, sse_a, sse_b, cost_a, cost_b, 30, 20)
    assert r["share_a"].tolist() == [[1, 1, 1, 1], [1, 1, 1, 0], [100, 0, 513, 77]]
    assert r["share_b"].tolist() == [[2, 1, 258, 258], [1, 1, 257, 257], [9, 300, 0, 65536]]
    # (from, to): blocks, pixels, sse_a, sse_b, cost_a, cost_b
    want = {(11, 4): (8, 2 * (3 * 64 + 48), 288, 220, 7, 1035),
            (0, 0): (1, 32, 81, 59, 100, 9),
            (0, 1): (1, 32, 91, 66, 0, 300),
            (2, 0): (1, 32, 101, 73, 513, 0),
            (0, 3): (1, 24, 111, 80, 77, 65536)}
    for f in range(27):
        for t in range(27):
            got = tuple(int(r[k][f, t]) for k in KEYS)
            assert got == want.get((f, t), (0,) * 6), (f, t, got)
    assert r["pixels"].sum() == 30 * 20 and r["blocks"].sum() == 12
    assert r["block_delta"].dtype == np.int32
    assert r["block_delta"].tolist() == [
        [[2, -1, -4, -7], [-10, -13, -16, -19], [-22, -25, -28, -31]],
        [[1, 0, 257, 257], [0, 0, 256, 257], [-91, 300, -513, 65459]]]


def test_reference_refuses_maps_that_do_not_tile():
    acs = np.array([[4, 4 | C], [4 | C, 0]], np.uint8)  # a first block inside a varblock
    with pytest.raises(AssertionError):
        ab_ref.shares(acs, np.zeros((2, 2), np.uint32))


_enc = {}


def _encode(oracle, pair, side):
    key = (pair[0], side)
    if key not in _enc:
        _enc[key] = oracle.encode(pair_image(pair), *pair[2 + side])
    return _enc[key]


def _tiles(acs):
    """every first block's rectangle holds covered flags of its own id, every
    block is covered once, every varblock sits at a multiple of its own size"""
    bys, bxs = acs.shape
    seen = np.zeros(acs.shape, np.int32)
    for by, bx, t, down, across in ab_ref.first_blocks(acs):
        assert by % down == 0 and bx % across == 0, (by, bx, t)
        assert by + down <= bys and bx + across <= bxs, (by, bx, t)
        rect = acs[by:by + down, bx:bx + across].copy()
        assert rect[0, 0] == t
        rect[0, 0] |= C
        assert (rect == (t | C)).all(), (by, bx, t)
        seen[by:by + down, bx:bx + across] += 1
    assert (seen == 1).all()


@pytest.mark.parametrize("case", COVERAGE, ids=[c[0] for c in COVERAGE])
def test_dims_table_tiles_the_oracles_maps(oracle, case):
    d, e, p, coder, mask = case[5:]
    acs = oracle.encode(case_image(case), d, e, p, coder, mask).acs
    _tiles(acs)
    assert set(int(t) for t in np.unique(acs & 0x7F)) <= set(ab_ref.DIMS)


def _sides(oracle, pair, rng):
    """per side: strategy bytes, seeded error map, first-block costs of the stream"""
    out = []
    for side in (0, 1):
        r = _encode(oracle, pair, side)
        cost = rate_ref.reference(r.bytes)["block_cost"]
        sse = rng.integers(0, 64 * 3 * 255 * 255 + 1, size=r.acs.shape, dtype=np.uint32)
        out.append((np.asarray(r.acs), sse, cost))
    return out


def _marginal(acs, v):
    out = np.zeros(27, np.uint64)
    np.add.at(out, (acs & 0x7F).ravel(), np.asarray(v).astype(np.uint64).ravel())
    return out


@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[4]], ids=[PAIRS[0][0], PAIRS[4][0]])
def test_properties_on_oracle_pairs(oracle, pair):
    _, (_, w, h, _), _, _ = pair
    (acs_a, sse_a, cost_a), (acs_b, sse_b, cost_b) = _sides(oracle, pair, np.random.default_rng(18))
    r = ab_ref.reference(acs_a, acs_b, sse_a, sse_b, cost_a, cost_b, w, h)
    px = ab_ref.pixels(acs_a.shape[0], acs_a.shape[1], w, h)
    ones = np.ones(acs_a.shape, np.uint64)
    # every share map sums to its first-block map's total, varblock by varblock
    for acs, cost, sh in ((acs_a, cost_a, r["share_a"]), (acs_b, cost_b, r["share_b"])):
        assert int(sh.astype(np.uint64).sum()) == int(cost.astype(np.uint64).sum())
        for by, bx, t, down, across in ab_ref.first_blocks(acs):
            part = sh[by:by + down, bx:bx + across].astype(np.int64)
            assert int(part.sum()) == int(cost[by, bx]) and part.max() - part.min() <= 1
        assert (cost[(acs & C) != 0] == 0).all()
    # rows sum to side A's per-strategy sums, columns to side B's
    for k, va, vb in (("blocks", ones, ones), ("pixels", px, px)):
        assert np.array_equal(r[k].sum(axis=1), _marginal(acs_a, va)), k
        assert np.array_equal(r[k].sum(axis=0), _marginal(acs_b, vb)), k
    assert np.array_equal(r["sse_a"].sum(axis=1), _marginal(acs_a, sse_a))
    assert np.array_equal(r["sse_b"].sum(axis=0), _marginal(acs_b, sse_b))
    assert np.array_equal(r["cost_a"].sum(axis=1), _marginal(acs_a, r["share_a"]))
    assert np.array_equal(r["cost_b"].sum(axis=0), _marginal(acs_b, r["share_b"]))
    # a strategy's shares are its varblocks' costs
    assert np.array_equal(_marginal(acs_a, r["share_a"]), _marginal(acs_a, cost_a))
    assert np.array_equal(_marginal(acs_b, r["share_b"]), _marginal(acs_b, cost_b))
    assert int(r["pixels"].sum()) == w * h
    # a == b is diagonal
    d = ab_ref.reference(acs_a, acs_a, sse_a, sse_a, cost_a, cost_a, w, h)
    for k in KEYS:
        assert np.array_equal(d[k], np.diag(np.diag(d[k]))), k
    assert np.array_equal(np.diag(d["cost_a"]), _marginal(acs_a, cost_a))
    assert np.array_equal(d["cost_a"], d["cost_b"]) and not d["block_delta"].any()


# changed blocks and distinct off-diagonal cells per pair, counted with the CPU oracle
@pytest.mark.parametrize("pair", PAIRS, ids=[p[0] for p in PAIRS])
def test_gpu_pairs_move_enough_blocks(oracle, pair):
    a, b = (_encode(oracle, pair, s).acs & 0x7F for s in (0, 1))
    changed = int((a != b).sum())
    cells = len({(int(f), int(t)) for f, t in zip(a[a != b], b[a != b])})
    print(pair[0], a.size, changed, cells)
    assert cells >= 20 or changed >= 1000, (changed, cells)
    if pair[0] == "gradient_e7_e8":  # 128 px shapes on side B only
        assert set(np.unique(b[a != b]).tolist()) <= set(range(21, 27))
        assert not (a >= 21).any()
