"""Forced encode with the kinds of 128 / 256 px (raw ids 21 - 26 on their own
grid; force_big_list_kernel + big_write_kernel).

1. an effort-8 search's map, forced on contexts of effort 7 and 5, reproduces
   the search's bytes;
2. crafted maps on a natural image: the stream says what was asked (decoded
   maps, the oracle's encode_maps, the two reconstructions, the reference
   decoder, HfGlobal's quant tables);
3. a big varblock depends on its own bytes alone;
4. it codes its own pixels (against the same region tiled with DCT64X64);
5. nothing leaks between calls on a kept context; reports; refused maps;
6. jxg_cjxl round-trips an effort-8 map.
"""
import ctypes
import struct
import subprocess
import zlib

import numpy as np
import pytest

import crafted
from sweep_cases import cached
from test_force_map_big import (B1_HEADS, B2_HEADS, B3_HEADS, BIG, OWN_MAP_FRAMES, b1_map, b2_map,
                                b3_map, gradient_rgb8)

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -5
MAX_SHARE = 0.005  # test_gpu_forced.py's parity bound: +-1, at most 0.5 % of the samples
QM_KIND = {22: 6, 23: 6, 21: 7, 25: 8, 26: 8, 24: 9}  # raw id -> quant table of HfGlobal


def natural(w, h, seed):
    def make():
        from jxg.synth import natural_rgb8

        img = natural_rgb8(w, h, seed)
        img.setflags(write=False)
        return img

    return cached(("forced_natural", w, h, seed), make)


def big_heads(acs):
    return [h for h in crafted.heads_of(acs) if h[0] in BIG]


# ---------------------------------------------------------------------------
# 1. an effort-8 map reproduces its bytes
# ---------------------------------------------------------------------------
def _own_flags(jxg, coder, filt):
    return (jxg.FLAGS_CJXL_DEFAULTS if filt else (jxg.FLAG_ANS if coder else 0)) | jxg.FLAG_KEEP_MAPS


def _e8_search(jxg, i):
    """(image, flags, codestream, stats with maps) of the effort-8 search of frame i"""
    def make():
        w, h, d, coder, filt = OWN_MAP_FRAMES[i]
        img = gradient_rgb8(w, h, w * 7 + h)
        flags = _own_flags(jxg, coder, filt)
        with jxg.Encoder(distance=d, effort=8, proposals=0, flags=flags) as enc:
            data = enc.encode(img)
            return img, flags, data, enc.stats()

    return cached(("forced_big_e8", i), make)


@pytest.mark.parametrize("i", range(len(OWN_MAP_FRAMES)),
                         ids=["%dx%d" % f[:2] for f in OWN_MAP_FRAMES])
def test_an_effort8_map_reproduces_its_bytes(jxg_mod, i):
    jxg = jxg_mod
    img, flags, data, st = _e8_search(jxg, i)
    d = OWN_MAP_FRAMES[i][2]
    heads = big_heads(st["acs"])
    print("forced big own-map %dx%d: varblocks of ids 21..26: %r" % (
        OWN_MAP_FRAMES[i][0], OWN_MAP_FRAMES[i][1],
        [sum(1 for h in heads if h[0] == t) for t in range(21, 27)]))
    assert heads, "no big varblock: the case shows nothing"
    for effort in (7, 5):
        with jxg.Encoder(distance=d, effort=effort, proposals=0, flags=flags) as fenc:
            for qf in (st["qf"], None):
                got = fenc.encode_forced(img, st["acs"], qf)
                fst = fenc.stats()
                assert got == data, "forced codestream differs (%d vs %d bytes), effort %d, %s" % (
                    len(got), len(data), effort, "own qf" if qf is not None else "no qf")
                for k in ("acs", "qf", "dc", "ac"):
                    assert np.array_equal(fst[k], st[k]), (k, effort)


def test_the_effort8_maps_hold_all_six_kinds(jxg_mod):
    seen = set()
    for i in range(3):
        seen |= {t for t, _, _ in big_heads(_e8_search(jxg_mod, i)[3]["acs"])}
    assert seen == set(BIG), sorted(seen)


# ---------------------------------------------------------------------------
# 2. crafted maps on a natural image
# ---------------------------------------------------------------------------
# name -> (w, h, map, the big varblocks)
CRAFTED = {"b1": (512, 512, b1_map, B1_HEADS), "b2": (648, 392, b2_map, B2_HEADS),
           "b3": (648, 392, b3_map, B3_HEADS)}
# settings: (distance, cjxl's defaults or flags 0)
SETTINGS = {"cjxl_defaults": (1.0, True), "flags0": (2.0, False)}
RUNS = [(m, s) for m in CRAFTED for s in SETTINGS]
RUN_IDS = ["%s-%s" % r for r in RUNS]


def _tiled64(acs):
    """the map with every big varblock's region tiled with DCT64X64"""
    out = acs.copy()
    for t, by, bx in big_heads(acs):
        cy, cx = BIG[t]
        for ty in range(by, by + cy, 8):
            for tx in range(bx, bx + cx, 8):
                out[ty:ty + 8, tx:tx + 8] = 0x80 | 18
                out[ty, tx] = 18
    return out


def _crafted_run(jxg, name, setting):
    """the forced encode of a crafted map, once: stream, stats, the two
    reconstructions, the block error map, decoded maps; the block error maps of
    the same frame with the big regions tiled with DCT64X64 at the same quant
    field, and of the big map coded from the image rolled by 64 px"""
    def make():
        w, h, make_map, heads = CRAFTED[name]
        d, defaults = SETTINGS[setting]
        acs = make_map()
        img = natural(w, h, 7)
        flags = (jxg.FLAGS_CJXL_DEFAULTS if defaults else 0) | jxg.FLAG_KEEP_MAPS
        with jxg.Encoder(distance=d, effort=7, flags=flags) as fenc:
            data = fenc.encode_forced(img, acs)
            st = fenc.stats()
            rec = fenc.reconstruct()
            bsse = fenc.strategy_report(img, block_map=True)["block_sse"]
            try:
                dec = fenc.decode(data)
            except jxg.JxgError as e:  # (the checks say what is wrong with the stream)
                dec = e
            fenc.encode_forced(img, _tiled64(acs), st["qf"])
            assert np.array_equal(fenc.stats()["qf"], st["qf"])
            bsse64 = fenc.strategy_report(img, block_map=True)["block_sse"]
            fenc.encode_forced(np.ascontiguousarray(np.roll(img, 64, axis=1)), acs, st["qf"])
            rolled = fenc.strategy_report(img, block_map=True)["block_sse"]
        try:
            maps = jxg.decode_maps(data)
        except jxg.JxgError as e:
            maps = e
        return dict(w=w, h=h, d=d, defaults=defaults, acs=acs, heads=[h for h in heads if h[0] in BIG],
                    img=img, data=data, st=st, rec=rec, dec=dec, maps=maps, bsse=bsse, bsse64=bsse64,
                    rolled=rolled)

    return cached(("forced_big_run", name, setting), make)


@pytest.mark.parametrize("name,setting", RUNS, ids=RUN_IDS)
def test_the_stream_says_what_was_asked(jxg_mod, oracle, decoder, name, setting):
    jxg = jxg_mod
    r = _crafted_run(jxg, name, setting)
    w, h, acs, st, maps = r["w"], r["h"], r["acs"], r["st"], r["maps"]
    assert jxg.check_strategy_map(acs, w, h) == (0, 0)
    assert sorted(big_heads(acs)) == sorted(r["heads"])
    assert np.array_equal(st["acs"], acs)
    assert not isinstance(maps, Exception), "jxg_decode_maps refuses the stream: %s" % maps
    assert np.array_equal(maps["acs"], acs)
    for k in ("qf", "dc", "ac"):
        assert np.array_equal(maps[k], st[k]), k
    coder, filters = (1, 3) if r["defaults"] else (0, 0)
    ref = oracle.encode_maps(w, h, st["acs"], st["qf"], st["dc"], st["ac"], maps["cmap"], r["d"], coder,
                             filters)
    assert ref.bytes == r["data"], "the oracle's encode_maps writes another stream"
    assert not isinstance(r["dec"], Exception), "jxg_decode_rgb8 refuses the stream: %s" % r["dec"]
    assert np.array_equal(r["rec"], r["dec"]), "jxg_reconstruct_rgb8 != jxg_decode_rgb8"
    want = decoder.decode(r["data"])
    # HfGlobal carries the quant tables of exactly the kinds the map uses
    assert sorted(want.qm_params) == sorted({QM_KIND[t] for t, _, _ in r["heads"]})
    diff = np.abs(r["rec"].astype(np.int32) - want.rgb.astype(np.int32))
    share = float(np.count_nonzero(diff)) / diff.size
    print("forced big %s %s: max |diff| %d, differing share %.3g" % (name, setting, diff.max(), share))
    assert diff.max() <= 1 and share <= MAX_SHARE


# ---------------------------------------------------------------------------
# 3. a varblock depends on its own bytes alone
# ---------------------------------------------------------------------------
def test_a_big_varblock_depends_on_its_own_bytes_alone(jxg_mod):
    jxg = jxg_mod
    r = _crafted_run(jxg, "b1", "cjxl_defaults")
    st = r["st"]
    one_of_each = {t: (t, by, bx) for t, by, bx in reversed(r["heads"])}
    assert set(one_of_each) == set(BIG)
    with jxg.Encoder(distance=r["d"], effort=7, flags=jxg.FLAGS_CJXL_DEFAULTS | jxg.FLAG_KEEP_MAPS) as fenc:
        for t, by, bx in one_of_each.values():
            fenc.encode_forced(r["img"], jxg.make_strategy_map(64, 64, [(t, by, bx)]))
            u = fenc.stats()
            cy, cx = BIG[t]
            sl = (slice(by, by + cy), slice(bx, bx + cx))
            assert np.array_equal(u["acs"][sl], st["acs"][sl]), t
            assert np.array_equal(u["ac"][sl], st["ac"][sl]), t
            assert np.array_equal(u["qf"][sl], st["qf"][sl]), t
            assert np.array_equal(u["dc"][(slice(None),) + sl], st["dc"][(slice(None),) + sl]), t
            assert np.any(u["ac"][sl]), t


# ---------------------------------------------------------------------------
# 4. it codes its own pixels
# ---------------------------------------------------------------------------
# Mean squared error per sample of a big varblock (the strategy report's block
# map over its pixels) against the same region of the same image coded as
# DCT64X64 varblocks at the same quant field: both code the same pixels with
# the same step, so the ratio stays near 1 -- the big kinds' quant tables are
# coarser at high frequencies, which costs some -- while a row pass reading
# another tile column codes content that is not there.  Measured on the three
# maps at the two settings (figures per frame in DESIGN.md 3.19): the largest
# ratio is OWN_RATIO_SEEN (a 128X256 in B3's bottom group row; 0.92 the
# smallest); with the image rolled by 64 px against the map the smallest of
# the six medians is ROLLED_MEDIAN_SEEN and the smallest single ratio 59.6.
# The margin is the project's 8 (the off-grid check of test_gpu_forced.py):
# five times the first, a twentieth of the second.
OWN_RATIO_SEEN = 1.490
ROLLED_MEDIAN_SEEN = 180.06
OWN_PIXELS_MARGIN = 8.0


def _region_mse(bmap, t, by, bx):
    cy, cx = BIG[t]
    return float(bmap[by:by + cy, bx:bx + cx].sum()) / (cy * cx * 64 * 3)


def _ratios(r, key):
    return [(_region_mse(r[key], t, by, bx) / max(_region_mse(r["bsse64"], t, by, bx), 1e-9), t, by, bx)
            for t, by, bx in r["heads"]]


@pytest.mark.parametrize("name,setting", RUNS, ids=RUN_IDS)
def test_big_varblocks_code_their_own_pixels(jxg_mod, name, setting):
    r = _crafted_run(jxg_mod, name, setting)
    ratios = _ratios(r, "bsse")
    assert len(ratios) == len(big_heads(r["acs"]))  # no varblock is left out
    assert all(_region_mse(r["bsse64"], t, by, bx) > 0.01 for _, t, by, bx in ratios)
    print("forced big %s %s: error against the DCT64X64 tiling, ratio min %.3f median %.3f max %.3f at %r"
          % (name, setting, min(ratios)[0], np.median([x[0] for x in ratios]), max(ratios)[0],
             max(ratios)[1:]))
    assert max(ratios)[0] <= OWN_PIXELS_MARGIN, max(ratios)


@pytest.mark.parametrize("name,setting", RUNS, ids=RUN_IDS)
def test_a_rolled_source_would_show(jxg_mod, name, setting):
    """for scale: the same map coded from pixels 64 px to the left"""
    r = _crafted_run(jxg_mod, name, setting)
    ratios = [x[0] for x in _ratios(r, "rolled")]
    print("forced big %s %s: rolled source, ratio min %.2f median %.2f max %.2f" % (
        name, setting, min(ratios), np.median(ratios), max(ratios)))
    assert np.median(ratios) > OWN_PIXELS_MARGIN


# ---------------------------------------------------------------------------
# 5. nothing leaks
# ---------------------------------------------------------------------------
def _after(enc, img, data):
    rate = enc.rate_report(block_map=True)
    rep = enc.strategy_report(img, block_map=True)
    return dict(data=data, rec=enc.reconstruct(), rate=rate, rep=rep)


def _same(a, b, what):
    assert a["data"] == b["data"], what
    assert np.array_equal(a["rec"], b["rec"]), what
    for k in a["rate"]:
        assert np.array_equal(a["rate"][k], b["rate"][k]), (what, "rate_report", k)
    for k in a["rep"]:
        assert np.array_equal(a["rep"][k], b["rep"][k]), (what, "strategy_report", k)


def test_a_kept_context_serves_big_and_other_encodes_in_turn(jxg_mod):
    jxg = jxg_mod
    img = natural(512, 512, 7)
    b1 = b1_map()
    small = jxg.make_strategy_map(64, 64, [(18, 0, 0), (5, 8, 8), (20, 32, 32)], fill=1)
    qf = ((np.arange(64)[:, None] * 5 + np.arange(64)[None, :] * 3) % 97 + 40).astype(np.uint8)
    steps = (("forced b1", lambda e: e.encode_forced(img, b1)),
             ("plain encode", lambda e: e.encode(img)),
             ("forced map without a big id", lambda e: e.encode_forced(img, small)),
             ("forced b1 with a quant field", lambda e: e.encode_forced(img, b1, qf)))
    flags = jxg.FLAGS_CJXL_DEFAULTS | jxg.FLAG_KEEP_MAPS
    with jxg.Encoder(distance=1.0, effort=7, flags=flags) as kept:
        for what, step in steps:
            got = _after(kept, img, step(kept))
            with jxg.Encoder(distance=1.0, effort=7, flags=flags) as fresh:
                want = _after(fresh, img, step(fresh))
            _same(got, want, what)
    # (the reports are of what was coded: the big kinds' rows are filled)
    assert all(got["rep"]["varblocks"][t] for t in BIG) and all(got["rate"]["cost"][t].sum() for t in BIG)


def test_ab_report_of_an_effort8_search_and_its_forced_copy_is_diagonal(jxg_mod):
    jxg = jxg_mod
    w, h, d, coder, filt = OWN_MAP_FRAMES[0]
    img = gradient_rgb8(w, h, w * 7 + h)
    flags = _own_flags(jxg, coder, filt)
    with jxg.Encoder(distance=d, effort=8, flags=flags) as a, \
            jxg.Encoder(distance=d, effort=7, flags=flags) as b:
        data = a.encode(img)
        acs = a.stats()["acs"]
        assert big_heads(acs)
        assert b.encode_forced(img, acs) == data
        rep = jxg.ab_report(a, b, img, block_delta=True)
        ra, rb = a.rate_report(), b.rate_report()
    off = ~np.eye(27, dtype=bool)
    assert rep["blocks"].sum() == 64 * 64 and not rep["blocks"][off].any()
    assert any(rep["blocks"][t, t] for t in BIG)
    assert np.array_equal(rep["sse_a"], rep["sse_b"]) and np.array_equal(rep["cost_a"], rep["cost_b"])
    assert rep["cost_a"].sum() > 0 and not rep["block_delta"].any()
    assert np.array_equal(ra["cost"], rb["cost"]) and ra["ac_bits"] == rb["ac_bits"]


def test_a_refused_big_map_leaves_the_context_as_it_was(jxg_mod):
    jxg = jxg_mod
    lib = jxg.load()
    img, other = natural(648, 392, 7), natural(648, 392, 8)
    off_grid = np.zeros((49, 81), np.uint8)
    off_grid[8:24, 8:24] = 0x80 | 21
    off_grid[8, 8] = 21
    past = np.zeros((49, 81), np.uint8)
    past[32:, 64:] = 0x80 | 24
    past[32, 64] = 24
    flags = jxg.FLAGS_CJXL_DEFAULTS
    with jxg.Encoder(distance=1.0, effort=7, flags=flags) as enc:
        enc.encode_forced(other, b2_map())
        rec = enc.reconstruct()
        for name, m, status, bad in (("off its grid", off_grid, UNSUPPORTED, 8 * 81 + 8),
                                     ("past the frame", past, INVALID_ARG, 32 * 81 + 64)):
            assert jxg.check_strategy_map(m, 648, 392) == (status, bad), name
            buf = jxg._Buffer()
            buf.size = 5  # (the call resets its output whatever it holds)
            st = lib.jxg_encode_forced_rgb8(enc._ctx, img.ctypes.data, 648, 392, 648 * 3,
                                            m.ctypes.data, None, ctypes.byref(buf))
            assert st == status, name
            assert not buf.data and buf.size == 0, name
            # still the earlier frame, big varblocks and all
            assert np.array_equal(enc.reconstruct(), rec), name
        with jxg.Encoder(distance=1.0, effort=7, flags=flags) as fresh:
            want = fresh.encode_forced(img, b2_map())
        assert enc.encode_forced(img, b2_map()) == want


# ---------------------------------------------------------------------------
# 6. CLI
# ---------------------------------------------------------------------------
def _png(path, img):
    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body))

    h, w, _ = img.shape
    raw = b"".join(b"\0" + img[y].tobytes() for y in range(h))
    path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                     + chunk(b"IDAT", zlib.compress(raw, 1)) + chunk(b"IEND", b""))
    return path


def test_cli_round_trips_an_effort8_map(jxg_mod, tmp_path):
    jxg = jxg_mod
    src = _png(tmp_path / "grad.png", gradient_rgb8(768, 520, 768 * 7 + 520))
    a, b = tmp_path / "A.jxl", tmp_path / "B.jxl"
    s, q = tmp_path / "S.pgm", tmp_path / "Q.pgm"

    def cli(*args):
        return subprocess.run([jxg.CLI_PATH] + [str(x) for x in args], capture_output=True, text=True)

    r = cli(src, a, "--effort=8", "--distance=2", "--jxg_strategy_out=%s" % s, "--jxg_qf_out=%s" % q)
    assert r.returncode == 0, r.stderr
    head = b"P5\n96 65\n255\n"
    raw = s.read_bytes()
    assert raw.startswith(head)
    acs = np.frombuffer(raw[len(head):], np.uint8).reshape(65, 96)
    assert big_heads(acs), "no big varblock: the case shows nothing"
    r = cli(src, b, "--effort=7", "--distance=2", "--jxg_strategy_in=%s" % s, "--jxg_qf_in=%s" % q)
    assert r.returncode == 0, r.stderr
    assert a.read_bytes() == b.read_bytes()
