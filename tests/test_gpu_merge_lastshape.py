"""merge_eval's last-shape form: the last shape a family workgroup evaluates
runs B's columns in the same pass as Y's and X's, in place in plane 2, and
quantizes Y, X and B back to back (jxg_merge.hip).  Which shape is last depends
on the effort and on the tile's size in blocks:

    effort / tile       C = 8   C = 16   C = 32   C = 64
    e6-7, full tile     16x8    32x16    64x32    64x64
    e5, or 4-7 blocks   16x8    32x16    32x32    -
    2-3 blocks          16x8    16x16    -        -

Every GPU case compares the encode with the oracle -- codestream bytes and the
acs / qf / dc maps -- after asserting on the oracle's acs alone that the frame
shows what the case is about: the shapes chosen in its full tiles and in its
partial tiles of a given size (`full`, `part`: (blocks, shapes)).
test_cases_cover_every_last_shape runs on the CPU and checks the file as a
whole: every last shape of the table is chosen in a tile where it is the last
one, and some tile holds a last and a non-last shape side by side."""
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu

# raw ids: 16x8, 8x16, 16x16, 32x16, 16x32, 32x32, 64x32, 32x64, 64x64
S16x8, S8x16, S16x16, S32x16, S16x32, S32x32, S64x32, S32x64, S64x64 = 6, 7, 4, 10, 11, 5, 19, 20, 18
ALL = (S16x8, S8x16, S16x16, S32x16, S16x32, S32x32, S64x32, S32x64, S64x64)


def last_shapes(effort, m):
    """the table: last evaluated shapes of a tile whose smaller side is m blocks"""
    if m >= 8 and effort >= 6:
        return {S16x8, S32x16, S64x32, S64x64}
    if m >= 4:
        return {S16x8, S32x16, S32x32}
    if m >= 2:
        return {S16x8, S16x16}
    return set()


EVERY_LAST = {S16x8, S16x16, S32x16, S32x32, S64x32, S64x64}

# name: (frame kind, w, h, seed, distance, effort, proposals, cjxl, full, part)
#   full: shapes chosen in the whole 64x64 tiles; part: (m, shapes chosen in the
#   partial tiles whose smaller side is m blocks)
CASES = {
    "e5_lasts": ("synth", 152, 88, 5, 3.0, 5, 3, True, (S16x8, S32x16, S32x32), (3, (S16x16,))),
    "blocks3_lasts": ("synth", 152, 88, 1, 3.0, 5, 0, True, (), (3, (S16x8, S16x16))),
    "blocks7_lasts": ("synth", 120, 248, 1, 1.0, 7, 3, False, (S32x64,), (7, (S32x16, S32x32))),
    "last_64x32": ("natural", 120, 248, 5, 3.0, 7, 3, True,
                   (S64x32, S32x16, S16x8, S16x32, S32x32), None),
    "last_64x64": ("synth", 64, 64, 1, 3.0, 7, 0, True, (S64x64,), None),
    "wide3_tall8": ("synth", 88, 152, 1, 1.0, 6, 3, False, (S32x64,), (3, (S16x16, S16x8))),
}
# two ranks (35 x 19 blocks: rank 1's group is the 3-block tile column)
SHARD = ("synth", 280, 152, 5, 1.0, 7, 3, False)


@functools.lru_cache(maxsize=None)
def frame(kind, w, h, seed):
    import oracle_ffi

    oracle_ffi.build()
    if kind == "synth":
        img = oracle_ffi.synth_rgb8(w, h, seed)
    else:
        from jxg.synth import natural_rgb8

        img = natural_rgb8(w, h, seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def oracle_ref(kind, w, h, seed, distance, effort, proposals, cjxl):
    import oracle_ffi

    return oracle_ffi.encode(frame(kind, w, h, seed), distance, effort, proposals,
                             1 if cjxl else 0, 7 if cjxl else 0)


def chosen(acs):
    """raw ids of the merged varblocks' first blocks in an acs (sub)map"""
    return {t for t in ALL if (acs == t).any()}


def tiles(acs):
    """(nbx, nby, acs of the tile) of every 64x64 tile of the frame"""
    by, bx = acs.shape
    for ty in range((by + 7) // 8):
        for tx in range((bx + 7) // 8):
            t = acs[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
            yield t.shape[1], t.shape[0], t


def preconditions(name):
    """what the case is about, asserted on the oracle alone; returns its ref"""
    kind, w, h, seed, d, e, p, cjxl, full, part = CASES[name]
    ref = oracle_ref(kind, w, h, seed, d, e, p, cjxl)
    in_full, in_part = set(), set()
    for nbx, nby, t in tiles(ref.acs):
        if (nbx, nby) == (8, 8):
            in_full |= chosen(t)
        elif part is not None and min(nbx, nby) == part[0]:
            in_part |= chosen(t)
    assert set(full) <= in_full, (name, sorted(in_full))
    if part is not None:
        assert set(part[1]) <= in_part, (name, sorted(in_part))
    if name == "wide3_tall8":  # a tile 3 blocks wide and 8 tall holds one of them
        odd = set()
        for nbx, nby, t in tiles(ref.acs):
            if (nbx, nby) == (3, 8):
                odd |= chosen(t)
        assert odd & set(part[1]), sorted(odd)
    return ref


def test_cases_cover_every_last_shape():
    as_last = set()
    side_by_side = False
    for name in CASES:
        ref = preconditions(name)
        e = CASES[name][5]
        for nbx, nby, t in tiles(ref.acs):
            c = chosen(t)
            last = last_shapes(e, min(nbx, nby))
            as_last |= c & last
            side_by_side |= bool(c & last) and bool(c - last)
    assert as_last == EVERY_LAST, sorted(as_last)
    assert side_by_side
    assert {CASES[n][5] for n in CASES} == {5, 6, 7}
    assert any(CASES[n][6] == 3 for n in CASES) and any(CASES[n][6] == 0 for n in CASES)
    assert any(CASES[n][7] for n in CASES) and any(not CASES[n][7] for n in CASES)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_lastshape_matches_oracle(jxg_mod, name):
    kind, w, h, seed, d, e, p, cjxl = CASES[name][:8]
    ref = preconditions(name)
    flags = jxg_mod.FLAG_KEEP_MAPS | (jxg_mod.FLAGS_CJXL_DEFAULTS if cjxl else 0)
    with jxg_mod.Encoder(distance=d, effort=e, proposals=p, flags=flags) as enc:
        got = enc.encode(frame(kind, w, h, seed))
        st = enc.stats()
    assert np.array_equal(st["acs"], ref.acs)
    assert np.array_equal(st["qf"], ref.qf)
    assert np.array_equal(st["dc"], ref.dc)
    assert got == ref.bytes


@gpu
def test_lastshape_two_rank_shard(jxg_mod):
    """the sharded path hands merge_eval its tiles through a list: rank 0 owns
    the full tiles (64 px shapes last) and the 3-block bottom row, rank 1 the
    3-block right column (16x8 and 16x16 last)"""
    from test_gpu_shard import sharded_encode

    kind, w, h, seed, d, e, p, cjxl = SHARD
    ref = oracle_ref(kind, w, h, seed, d, e, p, cjxl)
    assert (w + 255) // 256 == 2 and (h + 255) // 256 == 1
    right = chosen(ref.acs[:, 32:])
    assert right and right <= {S16x8, S8x16, S16x16}, sorted(right)
    assert chosen(ref.acs[:, :32]) & {S32x16, S32x32, S64x32, S64x64}
    assert sharded_encode(jxg_mod, frame(kind, w, h, seed), 2, d, e, p) == ref.bytes
