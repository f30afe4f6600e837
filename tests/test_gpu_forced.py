"""Forced encode on the GPU (jxg_encode_forced_rgb8): the
caller's AC-strategy map instead of the search.

1. the encoder's own map reproduces the encoder's bytes;
2. a block's result depends on its own forced id alone, and equals the search's
   where the search chose the same;
3. the stream says what was asked (decoded maps, the oracle's encode_maps, the
   two reconstructions, the reference decoder) at every placement the tile rule
   accepts (the S1 / S3 families of tests/crafted.py);
4. varblocks off their shape's grid are transformed from their own pixels;
5. the caller's quant field; 6. the reports; 7. nothing leaks between calls.
"""
import ctypes

import numpy as np
import pytest

import crafted
from sweep_cases import cached

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -5
MERGED = tuple(crafted.S1_ORDER)
MAX_SHARE = 0.005  # test_gpu_recon.py's parity bound: +-1, at most 0.5 % of the samples


def natural(w, h, seed):
    def make():
        from jxg.synth import natural_rgb8

        img = natural_rgb8(w, h, seed)
        img.setflags(write=False)
        return img

    return cached(("forced_natural", w, h, seed), make)


def natural_tile():
    """64x64: the window at (40, 24) of the 200 x 136 natural image, where the search
    merges three shapes or more at every setting of check 1 (most windows, and
    most 64 x 64 images of the generator, merge fewer at distance 1)"""
    def make():
        img = np.ascontiguousarray(natural(200, 136, 5)[40:104, 24:88])
        img.setflags(write=False)
        return img

    return cached("forced_natural_tile", make)


def search(jxg, img, d, e, flags, p=0):
    """(codestream, stats with maps) of a search encode on a fresh context"""
    with jxg.Encoder(distance=d, effort=e, proposals=p, flags=flags | jxg.FLAG_KEEP_MAPS) as enc:
        data = enc.encode(img)
        return data, enc.stats()


def forced_ctx(jxg, d, flags, effort=9, proposals=3):
    """a context for forced encodes: its effort and proposals play no part"""
    return jxg.Encoder(distance=d, effort=effort, proposals=proposals,
                       flags=flags | jxg.FLAG_KEEP_MAPS)


def merged_shapes(acs):
    heads = acs[(acs & 0x80) == 0]
    return sorted({int(t) for t in heads if int(t) in MERGED})


# ---------------------------------------------------------------------------
# 1. the encoder's own choice reproduces the encoder's bytes
# ---------------------------------------------------------------------------
FRAMES = {"200x136": lambda: natural(200, 136, 5),   # partial blocks, partial tiles
          "264x72": lambda: natural(264, 72, 5),     # two pass groups
          "2056x16": lambda: natural(2056, 16, 1),   # two LF groups
          "64x64": natural_tile}


@pytest.mark.parametrize("defaults", [True, False], ids=["cjxl_defaults", "flags0"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_own_map_reproduces_the_bytes(jxg_mod, frame, defaults):
    jxg = jxg_mod
    img = FRAMES[frame]()
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else 0
    for d in (1.0, 3.0):
        with forced_ctx(jxg, d, flags) as fenc:
            for e in (5, 6, 7):
                data, st = search(jxg, img, d, e, flags)
                shapes = merged_shapes(st["acs"])
                print("forced own-map %s %s d%g e%d: merged shapes %r" % (
                    frame, "defaults" if defaults else "flags0", d, e, shapes))
                # the case shows something only where merges occur
                assert len(shapes) >= 3, shapes
                got = fenc.encode_forced(img, st["acs"])
                fst = fenc.stats()
                assert got == data, "forced codestream differs (%d vs %d bytes)" % (len(got), len(data))
                for k in ("acs", "qf", "dc", "ac"):
                    assert np.array_equal(fst[k], st[k]), k
                assert "homog" not in fst
                # list order varies from run to run; the bytes do not
                assert fenc.encode_forced(img, st["acs"]) == data


def test_device_variant_gives_the_same_bytes(jxg_mod):
    import torch

    jxg = jxg_mod
    img = natural(200, 136, 5)
    data, st = search(jxg, img, 1.0, 7, jxg.FLAGS_CJXL_DEFAULTS)
    stride = 200 * 3 + 24
    buf = torch.zeros((136, stride), dtype=torch.uint8, device="cuda")
    buf[:, :600] = torch.from_numpy(img.reshape(136, 600).copy()).cuda()
    torch.cuda.synchronize()
    with forced_ctx(jxg, 1.0, jxg.FLAGS_CJXL_DEFAULTS) as fenc:
        assert fenc.encode_forced_device(buf.data_ptr(), 200, 136, st["acs"], row_stride=stride) == data
        assert fenc.encode_forced_device(buf.data_ptr(), 200, 136, st["acs"], st["qf"],
                                         row_stride=stride)  # (bytes: see the qf tests)


# ---------------------------------------------------------------------------
# 2. per-block independence
# ---------------------------------------------------------------------------
W2, H2 = 128, 72  # 16 x 9 blocks: two tiles across, a second tile row of one block row


def _uniform_runs(jxg):
    """{id: stats} of the six uniform 8x8-class maps, the rotation map's stats, the maps"""
    def make():
        img = natural(W2, H2, 5)
        out = {}
        with forced_ctx(jxg, 1.0, jxg.FLAGS_CJXL_DEFAULTS) as fenc:
            for t in crafted.CLASS8:
                fenc.encode_forced(img, np.full((9, 16), t, np.uint8))
                out[t] = fenc.stats()
            m = np.full((9, 16), 255, np.uint8)
            crafted.fill_rest(m)
            fenc.encode_forced(img, m)
            out["M"] = (m, fenc.stats())
        return out

    return cached("forced_uniform", make)


def test_a_block_depends_on_its_own_id_alone(jxg_mod):
    runs = _uniform_runs(jxg_mod)
    m, st = runs["M"]
    assert set(np.unique(m)) == set(crafted.CLASS8)
    assert np.array_equal(st["acs"], m)
    for t in crafted.CLASS8:
        u = runs[t]
        assert np.all(u["acs"] == t)
        at = m == t
        assert np.array_equal(st["ac"][at], u["ac"][at]), t
        assert np.array_equal(st["qf"][at], u["qf"][at]), t
        assert np.array_equal(st["dc"][:, at], u["dc"][:, at]), t
    # the six candidates differ: a block that got another's coefficients would show
    assert len({runs[t]["ac"].tobytes() for t in crafted.CLASS8}) == 6


@pytest.mark.parametrize("d,defaults", [(1.0, True), (3.0, False)])
def test_unmerged_blocks_equal_the_search(jxg_mod, d, defaults):
    jxg = jxg_mod
    img = natural(W2, H2, 5)
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else 0
    _, st = search(jxg, img, d, 7, flags)
    seen = 0
    with forced_ctx(jxg, d, flags) as fenc:
        for t in crafted.CLASS8:
            at = st["acs"] == t
            if not at.any():
                continue
            fenc.encode_forced(img, np.full((9, 16), t, np.uint8))
            u = fenc.stats()
            seen += 1
            assert np.array_equal(u["ac"][at], st["ac"][at]), t
            assert np.array_equal(u["qf"][at], st["qf"][at]), t
            assert np.array_equal(u["dc"][:, at], st["dc"][:, at]), t
    assert seen >= 3


def test_merged_varblocks_equal_the_search(jxg_mod):
    """a frame tiled with one aligned shape, against the search wherever the search
    chose that varblock"""
    jxg = jxg_mod
    img = natural(W2, H2, 5)
    compared = {}
    for d, flags in ((1.0, jxg.FLAGS_CJXL_DEFAULTS), (3.0, 0), (6.0, 0)):
        _, st = search(jxg, img, d, 7, flags)
        with forced_ctx(jxg, d, flags) as fenc:
            for t in merged_shapes(st["acs"]):
                cy, cx = crafted.TILE_SHAPES[t]
                vbs = [(t, by, bx) for by in range(0, 9 - cy + 1, cy) for bx in range(0, 16, cx)
                       if by % 8 + cy <= 8]
                fenc.encode_forced(img, jxg.make_strategy_map(9, 16, vbs))
                u = fenc.stats()
                for _, by, bx in [h for h in crafted.heads_of(st["acs"]) if h[0] == t]:
                    assert by % cy == 0 and bx % cx == 0  # the search's placements are aligned
                    sl = (slice(by, by + cy), slice(bx, bx + cx))
                    assert np.array_equal(u["acs"][sl], st["acs"][sl])
                    assert np.array_equal(u["ac"][sl], st["ac"][sl]), (t, by, bx)
                    assert np.array_equal(u["qf"][sl], st["qf"][sl]), (t, by, bx)
                    assert np.array_equal(u["dc"][(slice(None),) + sl], st["dc"][(slice(None),) + sl])
                    compared[t] = compared.get(t, 0) + 1
    print("forced merged-vs-search: varblocks compared per shape %r" % compared)
    assert len(compared) >= 3, compared


# ---------------------------------------------------------------------------
# 3. the stream says what was asked; 4. unaligned placements
# ---------------------------------------------------------------------------
def _s3_maps():
    """the nine shapes flush with the right edge (at an odd row), the bottom edge
    (at an odd column) and the corner of the S3 frame sizes, packed into as few
    maps as do not overlap: [(name, w, h, map, heads)]"""
    out = []
    for w, h in crafted.S3_SIZES:
        bys, bxs = h // 8, w // 8
        left = [p for p in crafted.s3_placements(bys, bxs) if p[0] in crafted.TILE_SHAPES]
        n = 0
        while left:
            acs = np.full((bys, bxs), 255, np.uint8)
            heads, rest = [], []
            for t, by, bx in left:
                cy, cx = crafted.shape_of(t)
                if np.all(acs[by:by + cy, bx:bx + cx] == 255):
                    crafted.place(acs, t, by, bx)
                    heads.append((t, by, bx))
                else:
                    rest.append((t, by, bx))
            crafted.fill_rest(acs, crafted.CLASS8, n)
            out.append(("s3_%dx%d_%d" % (w, h, n), w, h, acs, heads))
            left = rest
            n += 1
    return out


S1_NAMES = ["s1_%d" % i for i in range(5)]
S3_MAPS = _s3_maps()
S3_NAMES = [m[0] for m in S3_MAPS]


def _placement_cases(oracle):
    """[(name, w, h, map, heads, distance, coder, filters)]: the five S1 frames of
    tests/crafted.py (all 267 placements, one per tile) with their stream
    parameters, the S3 maps at distance 6 with every filter on"""
    def make():
        out = [(c.name, c.w, c.h, c.acs.copy(), list(c.heads), c.distance, c.coder, c.filters)
               for c in crafted.s1_cases()]
        out += [(name, w, h, acs, heads, 6.0, i % 2, 3)
                for i, (name, w, h, acs, heads) in enumerate(S3_MAPS)]
        return out

    return cached("forced_placements", make)


def _flags_of(jxg, coder, filters):
    return ((jxg.FLAG_ANS if coder else 0) | (jxg.FLAG_GABORISH if filters & 1 else 0) |
            (jxg.FLAG_EPF if filters & 2 else 0))


def _placement_run(jxg, oracle, name):
    """the forced encode of a placement case on a natural image, once: stream,
    stats, the two reconstructions, the block error map, decoded maps"""
    def make():
        case = next(c for c in _placement_cases(oracle) if c[0] == name)
        _, w, h, acs, heads, d, coder, filters = case
        img = natural(w, h, 7)
        with forced_ctx(jxg, d, _flags_of(jxg, coder, filters)) as fenc:
            data = fenc.encode_forced(img, acs)
            st = fenc.stats()
            rec = fenc.reconstruct()
            rep = fenc.strategy_report(img, block_map=True)
            try:
                dec = fenc.decode(data)
            except jxg.JxgError as e:  # (the checks below say what is wrong with the stream)
                dec = e
        try:
            maps = jxg.decode_maps(data)
        except jxg.JxgError as e:
            maps = e
        return dict(case=case, img=img, data=data, st=st, rec=rec, rep=rep, dec=dec, maps=maps)

    return cached(("forced_placement_run", name), make)


def test_the_placement_cases_hold_every_s1_placement(oracle):
    cases = _placement_cases(oracle)
    seen = {(t, by % 8, bx % 8) for c in cases[:5] for t, by, bx in c[4]}
    assert seen == set(crafted.s1_placements()) and len(seen) == 267
    edge = [h for c in cases[5:] for h in c[4]]
    # (64x64 fits flush with no edge of the S3 sizes inside a tile; S1 holds it)
    assert {t for t, _, _ in edge} == set(crafted.TILE_SHAPES) - {18}


@pytest.mark.parametrize("name", S1_NAMES + S3_NAMES)
def test_the_stream_says_what_was_asked(jxg_mod, oracle, decoder, name):
    r = _placement_run(jxg_mod, oracle, name)
    _, w, h, acs, heads, d, coder, filters = r["case"]
    st, maps = r["st"], r["maps"]
    assert len(heads) >= 1 and jxg_mod.check_strategy_map(acs, w, h) == (0, 0)
    assert np.array_equal(st["acs"], acs)
    assert not isinstance(maps, Exception), "jxg_decode_maps refuses the stream: %s" % maps
    assert np.array_equal(maps["acs"], acs)
    for k in ("qf", "dc", "ac"):
        assert np.array_equal(maps[k], st[k]), k
    ref = oracle.encode_maps(w, h, st["acs"], st["qf"], st["dc"], st["ac"], maps["cmap"], d, coder,
                             filters)
    assert ref.bytes == r["data"], "the oracle's encode_maps writes another stream"
    assert not isinstance(r["dec"], Exception), "jxg_decode_rgb8 refuses the stream: %s" % r["dec"]
    assert np.array_equal(r["rec"], r["dec"]), "jxg_reconstruct_rgb8 != jxg_decode_rgb8"
    want = decoder.decode(r["data"]).rgb
    diff = np.abs(r["rec"].astype(np.int32) - want.astype(np.int32))
    share = float(np.count_nonzero(diff)) / diff.size
    print("forced %s: max |diff| %d, differing share %.3g" % (name, diff.max(), share))
    assert diff.max() <= 1 and share <= MAX_SHARE


# Mean squared error per sample of a varblock, from the strategy report's block
# map.  Check 2 pins the grid placements bit for bit, so on each S1 frame the
# largest value among the varblocks of a shape that sit on its grid is the
# yardstick for those that do not: a varblock transformed from another block's
# pixels codes content that is not there.  Measured once on the five frames
# (natural image, seed 7; figures in DESIGN.md 3.19): the largest off-grid /
# on-grid-maximum ratios of the five frames are 2.19, 1.43, 2.93, 5.63 and 1.02
# (UNALIGNED_RATIO_SEEN: a 16x16 at block (61, 42) of s1_3 that holds the
# frame's busiest 16x16 of pixels, against two on-grid ones); the first frame
# coded from pixels one block to the left (the image rolled by 8 px, reported
# against the unrolled one) has SHIFTED_RATIO_SEEN times a varblock's error at
# the median (2.77 at the least: a smooth varblock hardly notices).  The margin
# covers the first with room for content differences and stays under the second.
UNALIGNED_RATIO_SEEN = 5.633
SHIFTED_RATIO_SEEN = 12.46
UNALIGNED_MARGIN = 8.0


def _varblock_mse(bmap, t, by, bx):
    cy, cx = crafted.shape_of(t)
    return float(bmap[by:by + cy, bx:bx + cx].sum()) / (cy * cx * 64 * 3)


def _on_grid(t, by, bx):
    cy, cx = crafted.shape_of(t)
    return by % cy == 0 and bx % cx == 0


@pytest.mark.parametrize("name", S1_NAMES)
def test_unaligned_varblocks_code_their_own_pixels(jxg_mod, oracle, name):
    r = _placement_run(jxg_mod, oracle, name)
    heads, bmap = r["case"][4], r["rep"]["block_sse"]
    yard = {}
    for t, by, bx in heads:
        if _on_grid(t, by, bx):
            yard[t] = max(yard.get(t, 0.0), _varblock_mse(bmap, t, by, bx))
    ratios = [(_varblock_mse(bmap, t, by, bx) / yard[t], t, by, bx) for t, by, bx in heads
              if not _on_grid(t, by, bx) and yard.get(t, 0.0) > 0.0]
    print("forced %s: %d off-grid varblocks against on-grid ones of their shape, largest ratio "
          "%.3f at %r" % (name, len(ratios), max(ratios)[0], max(ratios)[1:]))
    assert len(ratios) >= 4  # (the fifth frame holds the last 11 placements)
    assert max(ratios)[0] <= UNALIGNED_MARGIN, max(ratios)


def test_a_shifted_source_would_show(jxg_mod, oracle):
    """for scale: the same frame coded from pixels one block to the left"""
    jxg = jxg_mod
    r = _placement_run(jxg, oracle, "s1_0")
    _, w, h, acs, heads, d, coder, filters = r["case"]
    img = r["img"]
    with forced_ctx(jxg, d, _flags_of(jxg, coder, filters)) as fenc:
        fenc.encode_forced(np.ascontiguousarray(np.roll(img, 8, axis=1)), acs)
        shifted = fenc.strategy_report(img, block_map=True)["block_sse"]
    ratios = [_varblock_mse(shifted, t, by, bx) / max(_varblock_mse(r["rep"]["block_sse"], t, by, bx), 1e-9)
              for t, by, bx in heads]
    print("forced shifted source: error ratio min %.2f median %.2f" % (min(ratios), np.median(ratios)))
    assert np.median(ratios) > UNALIGNED_MARGIN


# ---------------------------------------------------------------------------
# 5. the caller's quant field
# ---------------------------------------------------------------------------
def _mixed_map(jxg, bys, bxs):
    vbs = [(4, 0, 0), (7, 0, 4), (6, 2, 5), (5, 4, 0), (10, 0, 6), (11, 8, 8), (20, 12, 8)]
    return jxg.make_strategy_map(bys, bxs, [v for v in vbs if v[1] + crafted.shape_of(v[0])[0] <= bys
                                            and v[2] + crafted.shape_of(v[0])[1] <= bxs], fill=3), vbs


@pytest.mark.parametrize("defaults", [True, False], ids=["cjxl_defaults", "flags0"])
def test_quant_field_constant_and_ramp(jxg_mod, defaults):
    jxg = jxg_mod
    img = natural(200, 136, 5)
    bys, bxs = 17, 25
    acs, _ = _mixed_map(jxg, bys, bxs)
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else 0
    with forced_ctx(jxg, 2.0, flags) as fenc:
        for c in (0, 37, 255):
            data = fenc.encode_forced(img, acs, np.full((bys, bxs), c, np.uint8))
            assert np.all(fenc.stats()["qf"] == c)
            assert np.all(jxg.decode_maps(data)["qf"] == c)
        ramp = ((np.arange(bys)[:, None] * 29 + np.arange(bxs)[None, :] * 7) % 251).astype(np.uint8)
        data = fenc.encode_forced(img, acs, ramp)
        got = fenc.stats()["qf"]
        want = ramp.copy()
        for t, by, bx in crafted.heads_of(acs):
            cy, cx = crafted.shape_of(t)
            want[by:by + cy, bx:bx + cx] = ramp[by:by + cy, bx:bx + cx].max()
        assert np.array_equal(got, want)
        assert np.array_equal(jxg.decode_maps(data)["qf"], want)
        assert np.array_equal(jxg.decode_maps(data)["acs"], acs)
        # NULL keeps the context's own field
        fenc.encode_forced(img, acs)
        own = fenc.stats()["qf"]
        assert not np.array_equal(own, want)


def test_forcing_a_search_encodes_own_maps(jxg_mod):
    jxg = jxg_mod
    img = natural(200, 136, 5)
    for flags in (jxg.FLAGS_CJXL_DEFAULTS, 0):
        _, st = search(jxg, img, 1.0, 7, flags)
        with forced_ctx(jxg, 1.0, flags) as fenc:
            data = fenc.encode_forced(img, st["acs"], st["qf"])
        maps = jxg.decode_maps(data)
        assert np.array_equal(maps["acs"], st["acs"]) and np.array_equal(maps["qf"], st["qf"])


# ---------------------------------------------------------------------------
# 6. reports
# ---------------------------------------------------------------------------
def test_ab_report_of_a_search_and_its_forced_copy_is_diagonal(jxg_mod):
    jxg = jxg_mod
    img = natural(200, 136, 5)
    flags = jxg.FLAGS_CJXL_DEFAULTS | jxg.FLAG_KEEP_MAPS
    with jxg.Encoder(distance=1.0, effort=7, flags=flags) as a, forced_ctx(jxg, 1.0, flags) as b:
        data = a.encode(img)
        assert b.encode_forced(img, a.stats()["acs"]) == data
        rep = jxg.ab_report(a, b, img, block_delta=True)
        ra, rb = a.rate_report(), b.rate_report()
    off = ~np.eye(27, dtype=bool)
    assert rep["blocks"].sum() == 17 * 25 and not rep["blocks"][off].any()
    assert np.array_equal(rep["sse_a"], rep["sse_b"]) and np.array_equal(rep["cost_a"], rep["cost_b"])
    assert rep["cost_a"].sum() > 0 and not rep["block_delta"].any()
    assert np.array_equal(ra["cost"], rb["cost"]) and ra["ac_bits"] == rb["ac_bits"]


def test_strategy_report_counts_the_forced_varblocks(jxg_mod):
    jxg = jxg_mod
    img = natural(200, 136, 5)
    acs, _ = _mixed_map(jxg, 17, 25)
    crafted_rest = acs == 3
    rot = np.full(acs.shape, 255, np.uint8)
    crafted.fill_rest(rot)
    acs[crafted_rest] = rot[crafted_rest]
    with forced_ctx(jxg, 2.0, jxg.FLAGS_CJXL_DEFAULTS) as fenc:
        fenc.encode_forced(img, acs)
        rep = fenc.strategy_report(img)
    want = np.zeros(27, np.uint64)
    blocks = np.zeros(27, np.uint64)
    for t, _, _ in crafted.heads_of(acs):
        want[t] += 1
        blocks[t] += crafted.shape_of(t)[0] * crafted.shape_of(t)[1]
    assert np.array_equal(rep["varblocks"], want) and np.array_equal(rep["blocks"], blocks)
    assert len(np.nonzero(want)[0]) >= 12


# ---------------------------------------------------------------------------
# 7. no leak
# ---------------------------------------------------------------------------
def _refused_maps(jxg):
    """one map per refusal kind for a 200 x 136 frame: (name, map, status)"""
    def base():
        return np.zeros((17, 25), np.uint8)

    out = []
    m = base(); m[3, 5] = 21; out.append(("unsupported_id", m, UNSUPPORTED))
    m = base(); m[0, 24] = 7; out.append(("past_the_frame", m, INVALID_ARG))
    m = base(); m[3, 7] = 4; m[3, 8] = m[4, 7] = m[4, 8] = 0x84
    out.append(("across_a_tile", m, INVALID_ARG))
    m = jxg.make_strategy_map(17, 25, [(4, 2, 2)]); m[2, 3] = 0x85
    out.append(("cover_of_another_id", m, INVALID_ARG))
    m = base(); m[5, 5] = 0x84; out.append(("orphan_cover", m, INVALID_ARG))
    m = jxg.make_strategy_map(17, 25, [(4, 2, 2)]); m[3, 3] = 4; m[3, 4] = m[4, 3] = m[4, 4] = 0x84
    out.append(("overlap", m, INVALID_ARG))
    return out


def test_search_forced_search_on_one_context(jxg_mod):
    jxg = jxg_mod
    img = natural(200, 136, 5)
    acs, _ = _mixed_map(jxg, 17, 25)
    for flags, p in ((jxg.FLAGS_CJXL_DEFAULTS, 3), (0, 0)):
        with jxg.Encoder(distance=1.0, effort=7, proposals=p, flags=flags | jxg.FLAG_KEEP_MAPS) as enc:
            first = enc.encode(img)
            homog = enc.stats().get("homog")
            enc.encode_forced(img, acs, np.full(acs.shape, 9, np.uint8))
            assert "homog" not in enc.stats()
            third = enc.encode(img)
            assert third == first
            if p:
                assert np.array_equal(enc.stats()["homog"], homog)


def test_a_refused_map_leaves_the_context_as_it_was(jxg_mod):
    jxg = jxg_mod
    lib = jxg.load()
    img, other = natural(200, 136, 5), natural(200, 136, 6)
    flags = jxg.FLAGS_CJXL_DEFAULTS
    with jxg.Encoder(distance=1.0, effort=7, flags=flags) as fresh:
        want = fresh.encode(img)
    with jxg.Encoder(distance=1.0, effort=7, flags=flags) as enc:
        enc.encode(other)
        rec = enc.reconstruct()
        for name, m, status in _refused_maps(jxg):
            assert jxg.check_strategy_map(m, 200, 136)[0] == status, name
            buf = jxg._Buffer()
            buf.size = 5  # (the call resets its output whatever it holds)
            st = lib.jxg_encode_forced_rgb8(enc._ctx, img.ctypes.data, 200, 136, 600,
                                            m.ctypes.data, None, ctypes.byref(buf))
            assert st == status, name
            assert not buf.data and buf.size == 0, name
            assert np.array_equal(enc.reconstruct(), rec), name  # still the earlier frame
        assert enc.encode(img) == want
    # null arguments, a short stride
    with forced_ctx(jxg, 1.0, flags) as enc:
        ok = np.zeros((17, 25), np.uint8)
        buf = jxg._Buffer()
        call = lib.jxg_encode_forced_rgb8
        assert call(enc._ctx, None, 200, 136, 600, ok.ctypes.data, None, ctypes.byref(buf)) == INVALID_ARG
        assert call(enc._ctx, img.ctypes.data, 200, 136, 600, None, None, ctypes.byref(buf)) == INVALID_ARG
        assert call(enc._ctx, img.ctypes.data, 200, 136, 599, ok.ctypes.data, None, ctypes.byref(buf)) == INVALID_ARG
        assert call(enc._ctx, img.ctypes.data, 200, 136, 600, ok.ctypes.data, None, None) == INVALID_ARG
        assert call(None, img.ctypes.data, 200, 136, 600, ok.ctypes.data, None, ctypes.byref(buf)) == INVALID_ARG


def test_a_forced_call_while_a_frame_is_pending_is_refused(jxg_mod):
    jxg = jxg_mod
    lib = jxg.load()
    img = natural(200, 136, 5)
    flags = jxg.FLAGS_CJXL_DEFAULTS
    with jxg.Encoder(distance=1.0, effort=7, flags=flags) as fresh:
        want = fresh.encode(img)
    with jxg.Encoder(distance=1.0, effort=7, flags=flags) as enc:
        enc.submit(img)
        ok = np.zeros((17, 25), np.uint8)
        buf = jxg._Buffer()
        assert lib.jxg_encode_forced_rgb8(enc._ctx, img.ctypes.data, 200, 136, 600, ok.ctypes.data,
                                          None, ctypes.byref(buf)) == INVALID_ARG
        assert not buf.data
        got = enc.receive()
        assert bytes(got) == want
        assert enc.encode_forced(img, ok)  # and the context serves forced encodes afterwards
