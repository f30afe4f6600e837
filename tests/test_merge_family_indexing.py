"""Index math of merge_eval's family workgroups (csrc/jxg_merge.hip:
family_rows, family_writeout, col_pass<R, 1, true>), restated in Python as
tests/test_merge_indexing.py does for the per-shape passes.  A family's row
phase must cover every (channel, image row, column) of the tile once, whatever
shape is evaluated later; the write-out must put a held value where the
shape's own row pass would have put it, and only into valid varblocks; every
LDS index stays inside the three-plane image.  CPU only."""
import pytest

from test_merge_indexing import KMS, KPLANE, THREADS, Pass, pass_plane, row_pass_indices

CO3 = 3 * KPLANE  # EvalLds::co
FAMILIES = {0: [(1, 0)], 1: [(0, 1), (1, 1), (2, 1)], 2: [(1, 2), (2, 2), (3, 2)],
            3: [(2, 3), (3, 3)]}  # lcx -> (lcy, lcx) of its shapes


def held_items(lcx):
    """(thread, slot of hv, channel, Y, first column, column step) of every
    held value of family_rows<lcx>'s Y / X pass"""
    C = 8 << lcx
    out = []
    if C == 64:
        for i in range(THREADS):
            h, row = (i >> 6) & 1, ((i >> 7) << 6) | (i & 63)
            c, Y = row >> 6, row & 63
            out += [(i, k, c, Y, 2 * k + h) for k in range(32)]
    else:
        lgx, lch = 3 - lcx, 9 - lcx
        per = (2 << lch) // THREADS
        for tid in range(THREADS):
            for k in range(per):
                r = tid + k * THREADS
                c, i = r >> lch, r & ((1 << lch) - 1)
                gx, Y = i & ((1 << lgx) - 1), i >> lgx
                out += [(tid, k * C + q, c, Y, gx * C + q) for q in range(C)]
    return out


def b_rows(lcx):
    """S.co indices of family_rows<lcx>'s B pass (plane 2)"""
    C = 8 << lcx
    out = []
    if C == 64:
        for i in range(128):
            h, Y = (i >> 6) & 1, i & 63
            out += [2 * KPLANE + Y * KMS + 2 * k + h for k in range(32)]
    else:
        lgx, lch = 3 - lcx, 9 - lcx
        nb = 1 << lch
        for r in range(nb):  # thread r % 256, item r // 256
            gx, Y = r & ((1 << lgx) - 1), r >> lgx
            out += [2 * KPLANE + Y * KMS + gx * C + q for q in range(C)]
    return out


@pytest.mark.parametrize("lcx", sorted(FAMILIES))
def test_held_values_cover_the_tile_once(lcx):
    items = held_items(lcx)
    assert len(items) == THREADS * 32
    assert len({(t, s) for t, s, _, _, _ in items}) == len(items)  # 32 slots per thread, each once
    assert all(0 <= s < 32 for _, s, _, _, _ in items)
    cells = {(c, Y, x) for _, _, c, Y, x in items}
    assert cells == {(c, Y, x) for c in (0, 1) for Y in range(64) for x in range(64)}
    idx = b_rows(lcx)
    assert len(idx) == len(set(idx)) == 4096
    assert min(idx) >= 2 * KPLANE and max(idx) < CO3


@pytest.mark.parametrize("lcx", sorted(FAMILIES))
def test_writeout_equals_the_shapes_row_pass(lcx):
    """with every varblock valid the write-out stores exactly the index set of
    row_pass<C, 2> of each shape of the family, and the varblock it tests for
    validity is the one that owns the index"""
    for lcy, lx in FAMILIES[lcx]:
        P = Pass(lcy, lx)
        want = sorted(row_pass_indices(P, 2, 0))
        got = []
        for _, _, c, Y, x in held_items(lcx):
            v = ((Y >> P.lR) << P.lGX) | (x >> P.lC)
            assert 0 <= v < P.NV
            off = P.off(v, pass_plane(0, c))
            assert 0 <= Y * KMS + x - (off - pass_plane(0, c) * KPLANE) < P.R * KMS
            got.append(pass_plane(0, c) * KPLANE + Y * KMS + x)
        assert sorted(got) == want


@pytest.mark.parametrize("lcy", [0, 1, 2, 3])
def test_b_columns_out_of_place(lcy):
    """col_pass<R, 1, true>: loads inside plane 2, stores inside plane 1"""
    R = 8 << lcy
    nb = 64 // R
    for pidx in range(nb * 32):
        X, band = pidx & 31, (pidx >> 5) & (nb - 1)
        assert pidx >> (5 + 6 - (3 + lcy)) == 0  # one channel
        off = 2 * KPLANE + band * R * KMS + X
        for k in range(R):
            for o in (off + k * KMS, off + 32 + k * KMS):
                assert 2 * KPLANE <= o < CO3
                assert KPLANE <= o - KPLANE < 2 * KPLANE
