"""What the sequences of tests/reuse_cases.py reach, from the oracle and the
Python decoder alone (no GPU): the guard against a sequence that quietly stops
exercising anything.  test_gpu_context_reuse.py pushes the same frames through
one kept context and compares every frame with the results asserted here.

* MAIN crosses, shrinking and growing, every structural boundary of the
  encoder's plan: one 64 px tile, one 256 px pass group, one LF chunk of 4096
  samples, one 2048 px LF group; its last frame is its first, and another frame
  of that size with other content lies in between;
* neighbouring frames differ in content class: with a search (effort >= 5)
  some frame holds every merged shape of that effort, the white-noise frames
  hold none, the flat frames code no AC coefficient at all (one token per
  varblock and channel, the non-zero count), and the serialised HfGlobal
  sections (context map and histograms) of neighbours differ;
* E8 changes, at every step, which explicit quant tables HfGlobal lists.
"""
import numpy as np
import pytest

import reuse_cases as R

LF_CHUNK = 4096  # csrc/jxg_kernels.h kLfChunkSamples


def _blocks(w, h):
    return (w + 7) // 8, (h + 7) // 8


def _shape(w, h):
    """(tiles, pass groups, LF groups, blocks) of a frame"""
    bxs, bys = _blocks(w, h)
    return (((w + 63) // 64) * ((h + 63) // 64), ((w + 255) // 256) * ((h + 255) // 256),
            ((w + 2047) // 2048) * ((h + 2047) // 2048), bxs * bys)


def test_presets_and_sequences():
    assert set(R.PRESETS) == {"e7_cjxl_pf", "e5_prefix", "e8_cjxl", "e3_plain", "e7_ans_keep"}
    assert R.PRESETS["e7_cjxl_pf"] == (1.0, 7, 3, R.ANS, 7, False, "main")
    assert R.PRESETS["e5_prefix"][1:5] == (5, 0, R.PREFIX, 0)
    assert R.PRESETS["e8_cjxl"] == (1.0, 8, 0, R.ANS, 7, False, "e8")
    assert R.PRESETS["e3_plain"][1:5] == (3, 0, R.PREFIX, 0)
    assert R.PRESETS["e7_ans_keep"][1:6] == (7, 0, R.ANS, 0, True)
    for p in R.SEARCHING:
        assert R.PRESETS[p][1] >= 5 and R.PRESETS[p][6] == "main"
    assert [(f[2], f[3]) for f in R.E8] == [(520, 300), (300, 200), (512, 256), (264, 264)]


def test_main_crosses_every_boundary():
    sizes = [(f[2], f[3]) for f in R.MAIN]
    shapes = [_shape(w, h) for w, h in sizes]
    # the single-tile frames, the one past a pass group, the two-LF-group one
    for wh in ((64, 64), (9, 7), (1, 1)):
        assert wh in sizes and _shape(*wh)[:3] == (1, 1, 1)
    assert (257, 65) in sizes and _shape(257, 65)[:3] == (10, 2, 1)
    assert (2100, 72) in sizes and _shape(2100, 72)[2] == 2
    # a frame above 512 x 512 whose LF streams take several chunks, followed by
    # one whose streams fit one chunk
    assert min(sizes[0]) > 512 and shapes[0][3] > LF_CHUNK
    assert 3 * shapes[1][3] <= LF_CHUNK
    # every count both grows and shrinks between neighbours somewhere
    for k in range(4):
        steps = [b[k] - a[k] for a, b in zip(shapes, shapes[1:])]
        assert min(steps) < 0 < max(steps), (k, steps)
    # from and to one tile / one group / one LF group
    for k in range(3):
        ones = [s[k] == 1 for s in shapes]
        assert (True, False) in zip(ones, ones[1:]) and (False, True) in zip(ones, ones[1:])
    # the repeat: the first frame again at the end, and its plan key with other
    # content in between
    fr = R.frames("main")
    assert np.array_equal(fr[0], fr[-1])
    same_key = [i for i in range(1, len(fr) - 1) if fr[i].shape == fr[0].shape]
    assert same_key and all(not np.array_equal(fr[i], fr[0]) for i in same_key)
    assert any(fr[i].shape != fr[0].shape for i in range(1, len(fr) - 1))
    # no two neighbours share a size, so every step changes the plan key
    assert all(a != b for a, b in zip(sizes, sizes[1:]))


def test_main_neighbours_differ_in_content_class():
    classes = [f[0] for f in R.MAIN]
    assert all(a != b for a, b in zip(classes, classes[1:]))
    # smooth -> noise -> flat, twice
    trip = list(zip(classes, classes[1:], classes[2:]))
    assert trip.count(("smooth", "noise", "flat")) == 2
    # every noise frame comes right after a frame with merges, every flat frame
    # right after one with AC tokens
    for i, c in enumerate(classes):
        if c == "noise":
            assert classes[i - 1] in ("smooth", "natural", "synth")
        if c == "flat":
            assert classes[i - 1] in ("noise", "synth")


@pytest.mark.parametrize("preset", R.SEARCHING)
def test_main_strategy_sets(oracle, preset):
    refs = R.oracle_refs(preset)
    effort, proposals = R.PRESETS[preset][1], R.PRESETS[preset][2]
    merged = set(R.MERGED if effort >= 6 else R.MERGED[:6])  # effort 5 stops at 32 px
    ids = [R.first_ids(r.acs) for r in refs]
    for (cls, _, w, h, _), got, r in zip(R.MAIN, ids, refs):
        assert got <= set(R.CLASS8) | merged
        assert (r.acs.shape[1], r.acs.shape[0]) == _blocks(w, h)
        if cls == "noise":
            assert not got & merged and not (r.acs & 0x80).any()
        if cls in ("smooth", "natural", "synth"):
            assert got & merged and (r.acs & 0x80).any()
        if cls == "flat" and not proposals & 2:
            assert got == {0}
    # every merged shape of the effort in one frame
    assert any(merged <= got for got in ids)
    if preset == "e7_cjxl_pf":
        assert merged <= ids[0]
    # the strategy sets of neighbours differ
    assert all(a != b for a, b in zip(ids, ids[1:]))


@pytest.mark.parametrize("preset", [p for p in R.PRESETS if R.PRESETS[p][6] == "main"])
def test_main_flat_frames_have_no_ac_tokens(oracle, preset):
    refs = R.oracle_refs(preset)
    for (cls, _, w, h, _), r in zip(R.MAIN, refs):
        varblocks = int(((r.acs & 0x80) == 0).sum())
        if cls == "flat":
            assert not r.ac.any()
            # one token per varblock and channel: its non-zero count, nothing else
            assert int(r.ac_tokens.sum()) == 3 * varblocks
        else:
            assert r.ac.any() and int(r.ac_tokens.sum()) > 3 * varblocks


@pytest.mark.parametrize("preset", sorted(R.PRESETS))
def test_neighbours_differ_in_hf_global(oracle, preset):
    """the context map and histograms as serialised: a frame of several groups
    (HfGlobal is a section of its own) never repeats its predecessor's"""
    refs = R.oracle_refs(preset)
    hf = [R.hf_global(r.bytes) for r in refs]
    seen = 0
    for (_, _, w, h, _), sec in zip(R.SEQUENCES[R.PRESETS[preset][6]], hf):
        assert (sec is None) == (_shape(w, h)[1] == 1)
    last = None
    for sec in hf:
        if sec is not None:
            if last is not None:
                assert sec != last
                seen += 1
            last = sec
    assert seen >= 3
    # the repeat gives the first frame's bytes again
    if R.PRESETS[preset][6] == "main":
        assert refs[0].bytes == refs[-1].bytes
        assert len({r.bytes for r in refs}) == len(refs) - 1


def test_e8_qm_params_sequence(oracle, decoder):
    refs = R.oracle_refs("e8_cjxl")
    big = set(R.BIG)
    kinds = []
    for (_, _, w, h, _), r in zip(R.E8, refs):
        assert _shape(w, h)[1] > 1
        d = decoder.decode(r.bytes, groups=[])  # headers, HfGlobal; no group decoded
        kinds.append(tuple(sorted(d.qm_params)))
        # exactly the kinds of the 128 / 256 px shapes in the strategy map
        # (jxl_decode.SHAPES: 128X64 / 64X128 are kind 6, 128X128 is kind 7)
        ids = R.first_ids(r.acs) & big
        assert kinds[-1] == tuple(sorted({decoder.SHAPES[t][2] for t in ids}))
    assert tuple(kinds) == R.E8_QM_KINDS
    # every transition changes what HfGlobal must list
    assert all(a != b for a, b in zip(kinds, kinds[1:]))
