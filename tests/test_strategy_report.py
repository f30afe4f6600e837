"""The strategy report's host side (no GPU): the numpy reference pinned by hand
on a crafted map, its invariants, the Python mirror of the C structs, the
strategy_stats.csv round trip and A/B difference, and the C symbols."""
import ctypes
import os

import numpy as np
import pytest

import crafted
import strategy_ref
from strategy_ref import reference_block_sse, reference_report


@pytest.fixture(scope="module")
def tiny(oracle):
    """17 x 9 px = 3 x 2 blocks: one 16x8 varblock (id 6: two blocks down, one
    across) at the left, DCT8 blocks beside it; the right column is 1 px wide
    and the bottom row 1 px tall.  Quant field, coefficients and the two images
    are set by hand."""
    case = crafted.make_case("report_tiny", "T", 17, 9, 2.0, 1, 0, [(6, 0, 0)], 9, rest=(0,))
    assert case.acs.tolist() == [[6, 0, 0], [6 | 0x80, 0, 0]]
    qf = np.array([[9, 19, 29], [9, 39, 49]], np.uint8)
    ac = np.zeros((2, 3, 3, 64), np.int32)
    ac[0, 0, 0, 5] = 1      # the varblock: X 1 + 1 (one in its covered block), Y 1, B 0
    ac[1, 0, 0, 63] = -2
    ac[0, 0, 1, 2] = 7
    ac[0, 1, 1, 1] = -1     # DCT8: Y 1 + 2, B 1
    ac[1, 2, 1, 3] = 4
    ac[1, 2, 1, 4] = 4
    ac[1, 1, 2, 63] = 1
    orig = np.zeros((9, 17, 3), np.uint8)
    dec = np.ones((9, 17, 3), np.uint8)        # every sample off by one
    dec[8, 0] = (3, 0, 1)                      # the covered block's only row: 9 + 0 + 1 at x = 0
    dec[8, 16] = (0, 0, 11)                    # the 1 x 1 corner block: 121
    return case.acs, qf, ac, orig, dec


def test_reference_pinned_by_hand(tiny):
    acs, qf, ac, orig, dec = tiny
    r = reference_report(acs, qf, ac, orig, dec, 17, 9)
    used = [t for t in range(27) if r["blocks"][t]]
    assert used == [0, 6]
    # covered blocks count toward the varblock's id; edge pixels are cropped
    assert (r["varblocks"][6], r["blocks"][6], r["pixels"][6]) == (1, 2, 64 + 8)
    assert (r["varblocks"][0], r["blocks"][0], r["pixels"][0]) == (4, 4, 64 + 8 + 8 + 1)
    assert r["nonzeros"][6].tolist() == [2, 1, 0]
    assert r["nonzeros"][0].tolist() == [0, 3, 1]
    assert r["qf_sum"][6] == 10 + 10 and r["qf_sum"][0] == 20 + 30 + 40 + 50
    # 3 per pixel, but (8, 0): 10 and (8, 16): 121
    assert r["sse"][6] == 3 * 72 - 3 + 10
    assert r["sse"][0] == 3 * 81 - 3 + 121
    b = reference_block_sse(orig, dec)
    assert b.tolist() == [[192, 192, 24], [3 * 7 + 10, 24, 121]]


def _invariants(r, nb, w, h, total_sse):
    assert int(r["blocks"].sum()) == nb
    assert int(r["pixels"].sum()) == w * h
    assert int(r["sse"].sum()) == total_sse
    assert np.all(r["varblocks"] <= r["blocks"])


def test_rows_sum_to_the_frame(tiny):
    acs, qf, ac, orig, dec = tiny
    total = int(((orig.astype(np.int64) - dec) ** 2).sum())
    _invariants(reference_report(acs, qf, ac, orig, dec, 17, 9), 6, 17, 9, total)
    # a random map of every shape's id on a frame with both edges partial
    rng = np.random.default_rng(3)
    w, h = 8 * 37 + 3, 8 * 33 + 5
    bys, bxs = 34, 38
    acs2 = np.full((bys, bxs), 255, np.uint8)
    crafted.place(acs2, 21, 0, 0)
    crafted.place(acs2, 18, 16, 8)
    crafted.place(acs2, 11, 30, 30)
    crafted.fill_rest(acs2)
    qf2 = rng.integers(0, 256, (bys, bxs)).astype(np.uint8)
    ac2 = rng.integers(-1, 2, (bys, bxs, 3, 64)).astype(np.int32)
    o2 = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    d2 = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    r = reference_report(acs2, qf2, ac2, o2, d2, w, h)
    _invariants(r, bys * bxs, w, h, int(((o2.astype(np.int64) - d2) ** 2).sum()))
    assert r["blocks"][21] == 256 and r["varblocks"][21] == 1 and r["blocks"][18] == 64
    assert int(r["nonzeros"].sum()) == int(np.count_nonzero(ac2))
    assert int(r["qf_sum"].sum()) == int(qf2.astype(np.int64).sum()) + bys * bxs
    assert int(reference_block_sse(o2, d2).sum()) == int(r["sse"].sum())


def test_python_mirror_layout(jxg_mod):
    assert ctypes.sizeof(jxg_mod._StrategyRow) == 64
    assert ctypes.sizeof(jxg_mod._StrategyReport) == 27 * 64
    assert jxg_mod.NUM_STRATEGIES == strategy_ref.NUM_STRATEGIES == len(jxg_mod.STRATEGY_NAMES)
    rep = jxg_mod._StrategyReport()
    rep.row[6].nonzeros[2] = 5
    rep.row[26].sse = 2 ** 40
    d = rep.as_dict()
    assert d["nonzeros"][6, 2] == 5 and d["sse"][26] == 2 ** 40 and d["names"][6] == "DCT16X8"
    assert all(d[k].dtype == np.uint64 for k in strategy_ref.FIELDS)


def test_new_symbols_are_exported(jxg_mod):
    lib = jxg_mod.load()
    for name in ("jxg_strategy_report_rgb8", "jxg_strategy_report_rgb8_device",
                 "jxg_set_sweep_report", "jxg_sweep_report"):
        assert name in jxg_mod.EXPORTS
        assert getattr(lib, name) is not None


def _report(jxg_mod, rows):
    """{id: (varblocks, blocks, pixels, (nzx, nzy, nzb), qf_sum, sse)} -> report dict"""
    rep = jxg_mod._StrategyReport()
    for t, (vb, nb, px, nz, q, e) in rows.items():
        r = rep.row[t]
        r.varblocks, r.blocks, r.pixels, r.qf_sum, r.sse = vb, nb, px, q, e
        for c in range(3):
            r.nonzeros[c] = nz[c]
    return rep.as_dict()


def test_csv_round_trip_and_diff(jxg_mod, tmp_path):
    from jxg import harness

    a = _report(jxg_mod, {0: (10, 10, 600, (1, 20, 3), 250, 1200), 6: (1, 2, 40, (0, 5, 0), 16, 30)})
    b = _report(jxg_mod, {0: (8, 8, 472, (1, 18, 2), 200, 944), 4: (1, 4, 168, (2, 9, 1), 28, 126)})
    f1, f2 = str(tmp_path / "a" / "strategy_stats.csv"), str(tmp_path / "b" / "strategy_stats.csv")
    rows_a = harness.strategy_stats("img.png", "img-0.1-7.jxl", 0.1, 7, a, 32, 20)
    rows_b = harness.strategy_stats("img.png", "img-0.1-7.jxl", 0.1, 7, b, 32, 20)
    harness.write_strategy_stats(rows_a, f1)
    harness.write_strategy_stats(rows_b, f2)
    text = open(f1).read().splitlines()
    assert text[0].split(",") == harness.STRATEGY_HEADER and len(harness.STRATEGY_HEADER) == 16
    # f32 distance and f64 ratios in Rust's to_string form
    assert text[1] == "img.png,img-0.1-7.jxl,0.1,7,0,DCT8,10,10,600,0.9375,1,20,3,25,1200," \
        "0.6666666666666666"
    assert text[2] == "img.png,img-0.1-7.jxl,0.1,7,6,DCT16X8,1,2,40,0.0625,0,5,0,8,30,0.25"
    assert harness.read_strategy_stats(f1) == rows_a
    harness.write_strategy_stats(rows_b, f1)       # appends, one header
    assert len(open(f1).read().splitlines()) == 5
    os.remove(f1)
    harness.write_strategy_stats(rows_a, f1)
    diffs = harness.compare_strategy_stats(f1, f2)
    assert [d.strategy for d in diffs] == [0, 4, 6] and [d.name for d in diffs] == [
        "DCT8", "DCT16X16", "DCT16X8"]
    assert diffs[0].diffs == [-2.0, -2.0, -128.0, 472 / 640 - 600 / 640, 0.0, -2.0, -1.0, 0.0,
                              -256.0, 944 / (3 * 472) - 1200 / 1800]
    assert diffs[1].diffs[:3] == [1.0, 4.0, 168.0] and diffs[1].diffs[7] == 7.0   # only in run 2
    assert diffs[2].diffs[:3] == [-1.0, -2.0, -40.0] and diffs[2].diffs[8] == -30.0  # only in run 1
    out = open(str(tmp_path / "a" / "strategy_diffs.csv")).read().splitlines()
    assert out[0].split(",") == harness.STRATEGY_DIFF_HEADER and len(out) == 4
    assert out[2] == "img.png,img-0.1-7.jxl,0.1,7,4,DCT16X16,1,4,168,0.2625,2,9,1,7,126,0.25"
