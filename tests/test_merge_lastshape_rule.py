"""Which shape of a width family merge_eval evaluates last (csrc/jxg_merge.hip:
family_last), restated in Python as tests/test_merge_family_indexing.py does
for the family's index math.  The last evaluated shape consumes the family's
row-transformed B (plane 2 of the LDS image) in place, so the rule must name
the shape after which the workgroup's shape loop evaluates nothing, for every
effort and every tile size, and that shape's valid varblocks must lie inside
the rows the family's row phase wrote.  CPU only."""
import pytest

# kShapes order: (name, lcy, lcx)
SHAPES = [("16x8", 1, 0), ("8x16", 0, 1), ("16x16", 1, 1), ("32x16", 2, 1), ("16x32", 1, 2),
          ("32x32", 2, 2), ("64x32", 3, 2), ("32x64", 2, 3), ("64x64", 3, 3)]
FAMILY_FIRST = {0: 0, 1: 1, 2: 4, 3: 7}
FAMILY_COUNT = {0: 1, 1: 3, 2: 3, 3: 2}


def max_level(effort):
    """levels searched: 16 and 32 px at effort 5, also 64 px at 6 and 7"""
    return 2 if effort == 5 else 3


def level(si):
    return max(SHAPES[si][1], SHAPES[si][2])


def evaluated(si, maxl, nbx, nby):
    """the shape loop's own test"""
    ls = level(si)
    return ls <= maxl and (1 << ls) <= nbx and (1 << ls) <= nby


def family_runs(fam, maxl, nbx, nby):
    """the workgroup's early return: the family's lowest level"""
    lm = max(fam, 1)
    return lm <= maxl and (1 << lm) <= nbx and (1 << lm) <= nby


def family_last(fam, maxl, nbx, nby):
    """highest evaluated si of the family, or -1 (the kernel's rule)"""
    last = -1
    for si in range(FAMILY_FIRST[fam], FAMILY_FIRST[fam] + FAMILY_COUNT[fam]):
        if evaluated(si, maxl, nbx, nby):
            last = si
    return last


# the issue's table: row by (effort, smaller tile side), column by family
def table_row(effort, m):
    if m >= 8 and effort >= 6:
        return ("16x8", "32x16", "64x32", "64x64")
    if m >= 4:
        return ("16x8", "32x16", "32x32", None)
    if m >= 2:
        return ("16x8", "16x16", None, None)
    return (None, None, None, None)


@pytest.mark.parametrize("effort", [5, 6, 7])
def test_last_shape_matches_the_table(effort):
    maxl = max_level(effort)
    for nbx in range(1, 9):
        for nby in range(1, 9):
            want = table_row(effort, min(nbx, nby))
            for fam in range(4):
                si = family_last(fam, maxl, nbx, nby) if family_runs(fam, maxl, nbx, nby) else -1
                got = SHAPES[si][0] if si >= 0 else None
                assert got == want[fam], (effort, nbx, nby, fam, got)
                # a family that runs evaluates something, and one that does not, nothing
                assert (si >= 0) == family_runs(fam, maxl, nbx, nby)
                assert family_runs(fam, maxl, nbx, nby) or family_last(fam, maxl, nbx, nby) < 0


@pytest.mark.parametrize("effort", [5, 6, 7])
def test_nothing_is_evaluated_after_the_last_shape(effort):
    maxl = max_level(effort)
    for nbx in range(1, 9):
        for nby in range(1, 9):
            for fam in range(4):
                si = family_last(fam, maxl, nbx, nby)
                if si < 0:
                    continue
                later = range(si + 1, FAMILY_FIRST[fam] + FAMILY_COUNT[fam])
                assert not any(evaluated(s, maxl, nbx, nby) for s in later)
                assert evaluated(si, maxl, nbx, nby)
                # 8x16 is never last (16x16 is the same level): the last shape has
                # columns of 16 points or more
                assert SHAPES[si][0] != "8x16" and SHAPES[si][1] >= 1


def test_last_shapes_varblocks_lie_in_the_family_rows():
    """family_rows writes plane 2 for the segments the family's lowest level
    needs; every row segment of a valid varblock of the last shape is one"""
    for effort in (5, 6, 7):
        maxl = max_level(effort)
        for nbx in range(1, 9):
            for nby in range(1, 9):
                for fam in range(4):
                    si = family_last(fam, maxl, nbx, nby)
                    if si < 0:
                        continue
                    _, lcy, lcx = SHAPES[si]
                    assert lcx == fam
                    ls, lm = level(si), max(fam, 1)
                    for v in range(64 >> (lcx + lcy)):
                        bx0 = (v & ((8 >> lcx) - 1)) << lcx
                        by0 = (v >> (3 - lcx)) << lcy
                        if not ((((bx0 >> ls) + 1) << ls) <= nbx and (((by0 >> ls) + 1) << ls) <= nby):
                            continue
                        for by in range(by0, by0 + (1 << lcy)):  # need(Y, gx) of family_rows
                            assert (((bx0 >> lm) + 1) << lm) <= nbx and (((by >> lm) + 1) << lm) <= nby
