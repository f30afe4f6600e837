"""merge_write's dense passes: a pass holds up to NV(shape) chosen varblocks
of one shape, taken from any tiles (jxg_merge_write.hip).  Every case compares the
GPU encode with the oracle -- codestream bytes and the acs / qf / dc maps --
and first asserts on the oracle's acs that the frame fills the passes the way
the case is about: full passes, partly filled last passes, lists shorter than
one pass, empty lists."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# raw id of a merged shape -> varblocks of it in one 64x64 pass
SLOTS = {6: 32, 7: 32, 4: 16, 10: 8, 11: 8, 5: 4, 19: 2, 20: 2, 18: 1}


def shape_counts(acs):
    """chosen varblocks per shape: first blocks carry the raw id without bit 7"""
    return {t: int((acs == t).sum()) for t in SLOTS}


@functools.lru_cache(maxsize=None)
def synth_frame():
    import oracle_ffi

    oracle_ffi.build()
    img = oracle_ffi.synth_rgb8(1000, 328, 5)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def natural_frame():
    from jxg.synth import natural_rgb8

    img = natural_rgb8(264, 520, 3)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def oracle_ref(frame, distance, effort, cjxl):
    import oracle_ffi

    oracle_ffi.build()
    img = {"synth": synth_frame, "natural": natural_frame}[frame]()
    return oracle_ffi.encode(img, distance, effort, 0, 1 if cjxl else 0, 7 if cjxl else 0)


def gpu_encode(jxg_mod, img, distance, effort, cjxl):
    flags = jxg_mod.FLAG_KEEP_MAPS | (jxg_mod.FLAGS_CJXL_DEFAULTS if cjxl else 0)
    with jxg_mod.Encoder(distance=distance, effort=effort, flags=flags) as enc:
        got = enc.encode(img)
        st = enc.stats()
    return got, st


def assert_matches(got, st, ref):
    assert np.array_equal(st["acs"], ref.acs)
    assert np.array_equal(st["qf"], ref.qf)
    assert np.array_equal(st["dc"], ref.dc)
    assert got == ref.bytes


@pytest.mark.parametrize("distance,cjxl", [(1.0, True), (1.0, False), (3.0, True), (3.0, False)])
def test_every_shape_full_and_partial_passes(jxg_mod, distance, cjxl):
    """125 x 41 blocks: the right tile column is 5 blocks wide, the bottom tile
    row 1 block high.  d1 with cjxl's defaults chooses all nine shapes
    (192 / 124 / 51 / 4 / 4 / 3 / 4 / 4 / 9 varblocks); the other parameters
    shift the counts (the oracle's, asserted below as far as they go)."""
    ref = oracle_ref("synth", distance, 7, cjxl)
    n = shape_counts(ref.acs)
    if cjxl and distance == 1.0:
        assert all(n.values()), n
        assert n[6] == 192 and n[7] == 124 and n[4] == 51 and n[5] == 3, n
    # a list that fills its passes exactly, one with full passes and a partly
    # filled last one, one shorter than a pass
    if cjxl:
        assert any(c and c % SLOTS[t] == 0 for t, c in n.items() if t != 18), n
    assert any(c > SLOTS[t] and c % SLOTS[t] for t, c in n.items()), n
    assert any(0 < c < SLOTS[t] for t, c in n.items()), n
    got, st = gpu_encode(jxg_mod, synth_frame(), distance, 7, cjxl)
    assert_matches(got, st, ref)


def test_empty_lists(jxg_mod, oracle):
    """a flat frame merges nothing: all nine lists stay empty"""
    img = np.full((136, 200, 3), 128, dtype=np.uint8)
    ref = oracle.encode(img, 1.0, 7, 0, 1, 7)
    assert not any(shape_counts(ref.acs).values()) and not (ref.acs & 0x80).any()
    got, st = gpu_encode(jxg_mod, img, 1.0, 7, True)
    assert_matches(got, st, ref)


@pytest.mark.parametrize("effort", [5, 7])
def test_levels_capped_at_32px(jxg_mod, effort):
    """e5 stops at 32x32 (the three 64 px lists stay empty); at e7 the same
    frame has a few 64x64.  Mostly 16x16 and larger: passes filled from many
    tiles."""
    ref = oracle_ref("natural", 1.0, effort, True)
    n = shape_counts(ref.acs)
    if effort == 5:
        assert n[19] == 0 and n[20] == 0 and n[18] == 0 and n[5] > 0, n
    else:
        assert n[18] > 0, n
    assert n[4] > 4 * SLOTS[4], n  # more 16x16 than any one tile holds
    got, st = gpu_encode(jxg_mod, natural_frame(), 1.0, effort, True)
    assert_matches(got, st, ref)


def test_batched_launch_matches_single(jxg_mod, oracle):
    """four queued frames share one merge launch (blockIdx.z): each frame's
    lists are its own"""
    frames = [oracle.synth_rgb8(256, 256, 11 + i) for i in range(4)]
    refs = [oracle.encode(f, 1.0, 7, 0, 1, 7) for f in frames]
    for r in refs:
        assert sum(shape_counts(r.acs).values()) > 32
    assert len({r.bytes for r in refs}) == 4
    flags = jxg_mod.FLAGS_CJXL_DEFAULTS
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=flags) as enc:
        single = [enc.encode(f) for f in frames]
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=flags) as enc:
        for f in frames:
            enc.submit(f)
        queued = []
        while enc.pending():
            queued.append(enc.receive())
    assert single == [r.bytes for r in refs]
    assert queued == single


def test_same_bytes_every_time(jxg_mod):
    """list order depends on which resolve workgroup's atomic lands first; the
    stored bytes do not"""
    ref = oracle_ref("synth", 1.0, 7, True)
    flags = jxg_mod.FLAGS_CJXL_DEFAULTS
    with jxg_mod.Encoder(distance=1.0, effort=7, flags=flags) as enc:
        outs = [enc.encode(synth_frame()) for _ in range(3)]
    assert outs[0] == ref.bytes
    assert outs[1] == outs[0] and outs[2] == outs[0]
