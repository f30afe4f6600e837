"""merge_eval's family workgroups: one workgroup per (tile, row width) runs the
row DCTs once and evaluates every shape of that width from them
(jxg_merge.hip).  Every GPU case compares the encode with the oracle --
codestream bytes and the acs / qf / dc maps -- on the smallest frames on which
a family workgroup can go wrong: a single tile, and frames whose right tile
column and bottom tile row are 1, 3 or 7 blocks, so that a family has no valid
shape there, or only its lower level, or every level but 64 px.

Each case first asserts on the oracle's acs that the frame shows what the case
is about (`expect`: shapes chosen somewhere; `edge`: shapes chosen inside the
partial tiles; `absent`: shapes that must not occur).  test_cases_cover_* runs
on the CPU and checks the file as a whole: all nine shapes are chosen, and both
families with two levels (C = 16: 8x16, 16x16 | 32x16; C = 32: 16x32, 32x32 |
64x32) have a partial tile where the oracle chose a lower-level shape while
the upper one does not fit.  (C = 8 has one shape and C = 64 one level, whose
shapes fit together or not at all.)"""
import functools

import numpy as np
import pytest

gpu = pytest.mark.gpu

# raw ids: 16x8, 8x16, 16x16, 32x16, 16x32, 32x32, 64x32, 32x64, 64x64
S16x8, S8x16, S16x16, S32x16, S16x32, S32x32, S64x32, S32x64, S64x64 = 6, 7, 4, 10, 11, 5, 19, 20, 18
ALL = (S16x8, S8x16, S16x16, S32x16, S16x32, S32x32, S64x32, S32x64, S64x64)
LEVEL = {S16x8: 1, S8x16: 1, S16x16: 1, S32x16: 2, S16x32: 2, S32x32: 2,
         S64x32: 3, S32x64: 3, S64x64: 3}

# name: (frame kind, w, h, seed, distance, effort, proposals, cjxl, expect, edge, absent)
CASES = {
    # one 64x64 tile
    "tile_64x64": ("synth", 64, 64, 1, 3.0, 7, 3, True, (S64x64,), (), ()),
    "tile_32x64": ("synth", 64, 64, 3, 1.0, 6, 3, False, (S32x64,), (), ()),
    "tile_mixed": ("natural", 64, 64, 1, 3.0, 7, 0, False, (S16x16, S32x16, S16x32), (), ()),
    # 25 x 17 blocks: the last tile column and row are 1 block: no level fits
    "edge1_cjxl": ("natural", 200, 136, 1, 3.0, 7, 3, True,
                   (S16x8, S8x16, S16x16, S32x16, S32x32, S64x32), (), ()),
    "edge1_synth": ("synth", 200, 136, 1, 3.0, 7, 3, True, (S32x64, S64x64, S32x32), (), ()),
    "edge1_e5": ("synth", 200, 136, 5, 1.0, 5, 0, True, (S32x16, S16x32),
                 (), (S64x32, S32x64, S64x64)),
    # 19 x 11 blocks: the last tile column and row are 3 blocks: level 16 only
    "edge3_e6": ("synth", 152, 88, 5, 1.0, 6, 3, False, (S32x16,), (S8x16, S16x16), ()),
    "edge3_cjxl": ("natural", 152, 88, 1, 3.0, 7, 3, True, (S32x32,), (S16x8, S8x16, S16x16), ()),
    "edge3_e5": ("natural", 152, 88, 3, 1.0, 5, 0, True, (), (S16x8, S8x16, S16x16), ()),
    # 15 x 31 blocks: the last tile column and row are 7 blocks: levels 16 and 32
    "edge7_cjxl": ("synth", 120, 248, 5, 3.0, 7, 3, True, (S64x64,), (S16x8, S16x16, S32x16, S16x32), ()),
    "edge7_plain": ("natural", 120, 248, 2, 1.0, 7, 0, False, (), (S16x16, S32x16, S32x32), ()),
    "edge7_e6": ("synth", 120, 248, 1, 1.0, 6, 3, False, (S32x64,), (S16x16, S16x32), ()),
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


def partial_tiles(acs):
    """(nbx, nby, acs of the tile) of every tile smaller than 8 x 8 blocks"""
    by, bx = acs.shape
    out = []
    for ty in range((by + 7) // 8):
        for tx in range((bx + 7) // 8):
            t = acs[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
            if t.shape != (8, 8):
                out.append((t.shape[1], t.shape[0], t))
    return out


def preconditions(name):
    """what the case is about, asserted on the oracle alone; returns its ref"""
    kind, w, h, seed, d, e, p, cjxl, expect, edge, absent = CASES[name]
    ref = oracle_ref(kind, w, h, seed, d, e, p, cjxl)
    got = chosen(ref.acs)
    assert set(expect) <= got, (name, sorted(got))
    assert not (set(absent) & got), (name, sorted(got))
    parts = partial_tiles(ref.acs)
    assert bool(parts) == (w > 64 or h > 64)
    in_edge = set()
    for nbx, nby, t in parts:
        fits = [lv for lv in (1, 2, 3) if (1 << lv) <= min(nbx, nby)]
        for s in chosen(t):
            assert LEVEL[s] in fits, (name, s, nbx, nby)  # (the oracle's own rule)
        in_edge |= chosen(t)
    assert set(edge) <= in_edge, (name, sorted(in_edge))
    if e == 5:
        assert not any(LEVEL[s] == 3 for s in got), name
    return ref


def test_cases_cover_every_shape_and_partial_family():
    seen = set()
    low16 = low32 = False
    for name in CASES:
        ref = preconditions(name)
        seen |= chosen(ref.acs)
        for nbx, nby, t in partial_tiles(ref.acs):
            m = min(nbx, nby)
            c = chosen(t)
            low16 |= 2 <= m <= 3 and bool(c & {S8x16, S16x16})  # 32x16 does not fit
            low32 |= 4 <= m <= 7 and bool(c & {S16x32, S32x32})  # 64x32 does not fit
    assert seen == set(ALL), sorted(seen)
    assert low16 and low32
    assert {CASES[n][5] for n in CASES} == {5, 6, 7}
    assert any(CASES[n][6] == 3 for n in CASES) and any(CASES[n][6] == 0 for n in CASES)
    assert any(CASES[n][7] for n in CASES) and any(not CASES[n][7] for n in CASES)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_family_matches_oracle(jxg_mod, name):
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
def test_family_two_rank_shard(jxg_mod):
    """the sharded path hands merge_eval its tiles through a list: rank 0 owns
    the full tiles and the 3-block bottom row, rank 1 the 3-block right column"""
    from test_gpu_shard import sharded_encode

    kind, w, h, seed, d, e, p, cjxl = SHARD
    ref = oracle_ref(kind, w, h, seed, d, e, p, cjxl)
    assert (w + 255) // 256 == 2 and (h + 255) // 256 == 1
    right = chosen(ref.acs[:, 32:])
    assert right and all(LEVEL[s] == 1 for s in right), sorted(right)
    assert any(LEVEL[s] >= 2 for s in chosen(ref.acs[:, :32]))
    assert sharded_encode(jxg_mod, frame(kind, w, h, seed), 2, d, e, p) == ref.bytes
