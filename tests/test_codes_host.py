"""The encoder's host-only code builder, run as itself (no GPU, nothing loaded
into Python): tests/native/codes_host.cpp is built by g++ from
csrc/jxg_codes.cpp, jxg_dequant.cpp, jxg_bitstream.cpp, jxg_plan.cpp and
jxg_layout.cpp alone -- under ASan + UBSan where the compiler has them -- and
prints LfGlobal, HfGlobal, the AC / LF codes, the arena layouts and the
mirrored arenas' sections.  The sections are read back by oracle/jxl_decode.py
(LfGlobal also compared with the oracle's stream byte for byte), the layouts
compared with their formulas restated here."""
import os
import shutil
import subprocess

import pytest

from test_decode_host import _sanitizer_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jpeg-xl-lossy-image-compression-thesis_amd", "csrc")
N_CTX, N_CLUSTERS, ALPHA, ANS_MAX_HISTS = 15 * (37 + 458), 132, 128, 8
ANS_TAB_BYTES = ANS_MAX_HISTS * 128 * 4 + ANS_MAX_HISTS * 4096 * 2 + 136
GEOMETRIES = [(200, 136, 1, 0), (2056, 24, 1, 0), (7680, 4320, 8, 3)]


@pytest.fixture(scope="module")
def codes_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp("ch")
    san = _sanitizer_flags(d)
    if not san:
        print("codes_host: the compiler does not accept the sanitizers; built without them")
    flags = ["-O1", "-std=c++17", "-Wall"] + san + os.environ.get("JXG_NATIVE_CFLAGS", "").split()
    exe = d / "codes_host"
    subprocess.check_call(["g++", *flags, os.path.join(ROOT, "tests", "native", "codes_host.cpp"),
                           *[os.path.join(PKG, f) for f in ("jxg_codes.cpp", "jxg_dequant.cpp",
                                                            "jxg_bitstream.cpp", "jxg_plan.cpp",
                                                            "jxg_layout.cpp")],
                           "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True,
                           timeout=120, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        return [ln.split() for ln in r.stdout.splitlines()]

    print("codes_host sanitizers: %s" % ("on" if san else "NOT available"))
    return run


def _ints(ln):
    return list(map(int, ln[1:]))


def _bits(ln):
    """'tag NBITS hex...' -> (bytes, nbits)"""
    return bytes(int(b, 16) for b in ln[2:]), int(ln[1])


def _lengths(code, n=ALPHA):
    """code lengths of a decoder PrefixCode, per symbol"""
    out = [0] * n
    if code.single is None:
        for s, l in zip(code.sym, code.len):
            out[s] = l
    return out


# ---- 1. LfGlobal ----
G_DISTS = (("b", 11, 1), ("b", 11, 2049), ("b", 12, 4097), ("b", 16, 8193))
QDC_DISTS = (("v", 16), ("b", 5, 1), ("b", 8, 1), ("b", 16, 1))


def test_lfglobal_equals_the_oracle_section(codes_host, oracle, decoder):
    """the 2056 x 24 frame (13 sections): LfGlobal for the oracle's scales,
    padded to a byte, is the oracle stream's section 0"""
    from jxg.synth import synth_rgb8

    ref = oracle.encode(synth_rgb8(2056, 24, 0x4A584C00), 1.0, 7, 0, 1, 0)
    toc = decoder.decode(ref.bytes, toc_only=True)
    assert len(toc.section_sizes) == 13
    o, s = toc.section_offsets[0], toc.section_sizes[0]
    got, _ = _bits(codes_host("lfglobal", ref.global_scale, ref.quant_dc)[0])
    assert got == ref.bytes[o:o + s]


@pytest.mark.parametrize("G", [1, 2048, 2049, 4096, 4097, 8192, 8193, 65535])
@pytest.mark.parametrize("qdc", [16, 1, 32, 33, 256, 257, 65536])
def test_lfglobal_selector_ranges(codes_host, decoder, G, qdc):
    """both ends of all four selector ranges of the global scale and of the DC
    quantizer, read back with the decoder's U32 reader"""
    data, nbits = _bits(codes_host("lfglobal", G, qdc)[0])
    br = decoder.BitReader(data)
    assert br.bool()  # default LF dequantization
    assert br.u32(*G_DISTS) == G
    assert br.u32(*QDC_DISTS) == qdc
    assert br.bool() and br.bool() and not br.bool()
    assert (br.pos + 7) // 8 * 8 == nbits


# ---- 2. HfGlobal ----
def _hfglobal(codes_host, decoder, coder, case, mask, ngroups):
    out = codes_host("hfglobal", coder, case, mask, ngroups)
    assert not [ln for ln in out if ln[0] == "blobsym_mismatch"]
    one = {ln[0]: ln for ln in out if ln[0] not in ("freq", "counts", "lens")}
    acl, used, ctxmap = _ints(one["acluster"]), _ints(one["used"]), _ints(one["ctxmap"])
    nhist = int(one["nhist"][1])
    assert len(acl) == len(ctxmap) == N_CTX and len(used) == N_CLUSTERS
    data, nbits = _bits(one["hf"])
    assert (data, nbits) == _bits(one["hf_direct"])  # cached context map == written in place
    br = decoder.BitReader(data, 0, nbits)
    qm = decoder.read_dequant_matrices(br)
    assert sorted(qm) == [6 + k for k in range(4) if mask >> k & 1]
    assert br.read(decoder.ceil_log2(ngroups)) + 1 == 1  # one HF preset
    assert br.u32(("v", 0x5F), ("v", 0x13), ("v", 0), ("b", 13, 0)) == 0
    es = decoder.EntropyStream(br, N_CTX)
    assert br.pos == nbits
    assert es.ctxmap == ctxmap
    assert max(ctxmap) + 1 == nhist
    assert es.prefix == (coder == "prefix")
    # dense ids in order of first appearance, empty clusters on histogram 0
    firsts = []
    for ctx in range(N_CTX):
        if used[acl[ctx]] and ctxmap[ctx] not in firsts:
            firsts.append(ctxmap[ctx])
        if not used[acl[ctx]]:
            assert ctxmap[ctx] == 0
    assert firsts == list(range(nhist)) or (not any(used) and nhist == 1)
    return out, one, es, acl, used, ctxmap, nhist


@pytest.mark.parametrize("case,nclusters", [("zero", 0), ("one", 1), ("all", 132)])
def test_hfglobal_prefix_codes_read_back(codes_host, decoder, case, nclusters):
    out, one, es, acl, used, ctxmap, nhist = _hfglobal(codes_host, decoder, "prefix", case, 0, 9)
    # one histogram per used static cluster (no token at all: one empty histogram)
    assert sum(used) == nclusters and nhist == max(nclusters, 1)
    lens = {int(ln[1]): _ints(ln[1:]) for ln in out if ln[0] == "lens"}
    assert sorted(lens) == list(range(N_CLUSTERS))
    hist_of = {acl[ctx]: ctxmap[ctx] for ctx in range(N_CTX)}
    assert sorted(hist_of) == list(range(N_CLUSTERS))
    for cl in range(N_CLUSTERS):
        if used[cl]:  # every prefix length read == the length in `packed`
            assert _lengths(es.codes[hist_of[cl]]) == lens[cl], cl
        else:
            assert lens[cl] == [0] * ALPHA


@pytest.mark.parametrize("case,mask", [("zero", 0), ("one", 0), ("all", 0), ("many", 0b1111),
                                       ("bigbin", 0), ("bigbin", 0b1111)])
def test_hfglobal_ans_tables_read_back(codes_host, decoder, case, mask):
    out, one, es, acl, used, ctxmap, nhist = _hfglobal(codes_host, decoder, "ans", case, mask, 9)
    assert nhist <= ANS_MAX_HISTS
    if case == "many":  # more distinct clusters than histograms: clustered again
        assert sum(used) > ANS_MAX_HISTS and nhist == ANS_MAX_HISTS
    if case == "all":
        assert sum(used) == N_CLUSTERS
    if case in ("zero", "one"):
        assert nhist == 1
    freq = {int(ln[1]): _ints(ln[1:]) for ln in out if ln[0] == "freq"}
    assert sorted(freq) == list(range(nhist))
    for h in range(nhist):  # every ANS count read == the builder's table frequency
        assert es.freqs[h] == freq[h], h
        assert sum(freq[h]) == 4096
    if case == "bigbin":
        counts = [_ints(ln) for ln in out if ln[0] == "counts"]
        assert max(max(c) for c in counts) > 65535
    # the blob's static cluster -> histogram bytes are the context map's
    blobmap = _ints(one["blobmap"])
    assert len(blobmap) == N_CLUSTERS
    for ctx in range(N_CTX):
        assert blobmap[acl[ctx]] == ctxmap[ctx]


# ---- 3. context-map cache ----
@pytest.mark.parametrize("coder", ["prefix", "ans"])
def test_context_map_cache(codes_host, decoder, coder):
    """equal maps: identical HfGlobal bytes and one serialisation; a changed
    map is serialised again and is what the decoder reads"""
    out = codes_host("cache", coder)
    writes = [int(ln[1]) for ln in out if ln[0] == "writes"]
    maps = [_ints(ln) for ln in out if ln[0] == "ctxmap"]
    hfs = [_bits(ln) for ln in out if ln[0] == "hf"]
    assert writes == [1, 1, 2]
    assert maps[0] == maps[1] != maps[2]
    assert hfs[0] == hfs[1] != hfs[2]
    for (data, nbits), cm in zip(hfs, maps):
        br = decoder.BitReader(data, 0, nbits)
        assert decoder.read_dequant_matrices(br) == {}
        br.read(decoder.ceil_log2(9))
        br.u32(("v", 0x5F), ("v", 0x13), ("v", 0), ("b", 13, 0))
        assert decoder.EntropyStream(br, N_CTX).ctxmap == cm


# ---- 4. bit layouts and chain order ----
@pytest.mark.parametrize("ans", [0, 1])
@pytest.mark.parametrize("w,h,world,rank", GEOMETRIES)
def test_bit_layouts(codes_host, w, h, world, rank, ans):
    out = {ln[0]: _ints(ln) for ln in codes_host("layout", w, h, world, rank, ans)}
    groups, ntok, bound, gbase = out["groups"], out["ntok"], out["bound"], out["gbase"]
    ngroups = -(-w // 256) * -(-h // 256)
    assert len(gbase) == len(bound) == ngroups and (world > 1 or groups == list(range(ngroups)))
    tok = [sum(ntok[3 * g:3 * g + 3]) for g in range(ngroups)]
    cursor = 0
    for g in groups:  # the parent's formulas: bound (+ tokens + state) to 32 bits, one spare word
        assert gbase[g] == cursor and cursor % 32 == 0
        size = bound[g] + (tok[g] + 32 if ans else 0)
        step = (size + 63) & ~31
        assert step >= size + 32 and step % 32 == 0  # non-overlapping
        cursor += step
    assert out["ac_words"] == [(cursor // 32 + 2 + 63) & ~63]
    untouched = 2 ** 64 - 1  # (gbase is written for the plan's groups only)
    assert all(gbase[g] == untouched for g in range(ngroups) if g not in set(groups))
    owns, sbound, sbase = out["owns"], out["sbound"], out["sbase"]
    cursor = 0
    for i in range(len(sbound)):
        assert sbase[i] == cursor and cursor % 32 == 0
        if owns[i // 2]:
            cursor += (sbound[i] + 63) & ~31
    assert out["lf_words"] == [cursor // 32 + 2]
    # chain order: a stable longest-first permutation of the launch slots
    order = out["order"]
    assert sorted(order) == list(range(len(groups)))
    assert order == sorted(range(len(groups)), key=lambda i: -tok[groups[i]])
    assert out["max_tokens"] == [max(tok[g] for g in groups)]
    assert len(set(tok[g] for g in groups)) < len(groups) or len(groups) == 1  # ties exist


# ---- 5. mirrored arenas ----
def _al(x):
    return (x + 255) & ~255


@pytest.mark.parametrize("w,h,world,rank", GEOMETRIES)
def test_arena_sections(codes_host, w, h, world, rank):
    out = codes_host("arenas", w, h, world, rank)
    ngroups, nlf, ng = _ints(next(ln for ln in out if ln[0] == "frame"))
    assert ngroups == -(-w // 256) * -(-h // 256) and nlf == -(-w // 2048) * -(-h // 2048)
    assert ng == ngroups if world == 1 else 0 < ng < ngroups
    ns = 2 * nlf
    arenas, cur = {}, None
    for ln in out:
        if ln[0] == "arena":
            cur = arenas.setdefault(ln[1], [])
        elif ln[0] == "section":
            cur.append((ln[1], int(ln[2]), int(ln[3]), int(ln[4]) * int(ln[5])))
    # the documented order and the sizes of every section, in bytes
    want = {"stat": [("hist_ac", N_CLUSTERS * ALPHA * 4), ("bound", ngroups * 4),
                     ("ntok", ngroups * 12), ("bandtok", ngroups * 16), ("bigcount", 16),
                     ("lfhist", ns * 4 * ALPHA * 4), ("sbound", ns * 4), ("vcount", nlf * 4)],
            "up": [("codes_ac", N_CLUSTERS * ALPHA * 4), ("gbase", ngroups * 8),
                   ("ans_order", max(1, ng) * 4), ("ans_tab", ANS_TAB_BYTES),
                   ("lfcodes", ns * 4 * ALPHA * 4), ("stream_base", ns * 8)],
            "bits": [("gbits", ngroups * 4), ("stream_bits", ns * 4)]}
    assert [int(x) for x in next(ln for ln in out if ln[0] == "tab_bytes")[1:]] == [ANS_TAB_BYTES]
    total = dict(zip(("stat", "up", "bits"), _ints(next(ln for ln in out if ln[0] == "bytes"))))
    assert _ints(next(ln for ln in out if ln[0] == "layout_bytes")) == list(total.values())
    offs = {}
    for name, secs in want.items():
        got = arenas[name]
        assert [(s[0], s[3]) for s in got] == secs
        end = 0
        for sec, d_off, h_off, nbytes in got:
            assert d_off == h_off  # h - host_base == d - dev_base
            assert d_off % 256 == 0 and d_off >= end
            assert d_off == _al(end)  # back to back
            end = d_off + nbytes
            offs[sec] = d_off
        assert total[name] == _al(end)
    # the partial-copy boundaries: the parent's formulas
    stat_lf = (_al(N_CLUSTERS * ALPHA * 4) + _al(ngroups * 4) + _al(ngroups * 12) +
               _al(ngroups * 16) + _al(16))
    up_gbase = _al(N_CLUSTERS * ALPHA * 4)
    up_ac = up_gbase + _al(ngroups * 8)
    up_lf = up_ac + _al(max(1, ng) * 4) + _al(ANS_TAB_BYTES)
    assert _ints(next(ln for ln in out if ln[0] == "marks")) == [stat_lf, up_gbase, up_ac, up_lf]
    assert (offs["lfhist"], offs["gbase"], offs["ans_order"], offs["lfcodes"]) == (
        stat_lf, up_gbase, up_ac, up_lf)


# ---- 6. LF-group codes ----
@pytest.mark.parametrize("epf", [0, 1])
def test_lf_codes_read_back(codes_host, decoder, epf):
    """the preludes of the two LF groups of a 2056 x 24 frame: tree and leaf
    codes read back to the builder's lengths, the varblock count field"""
    out = codes_host("lfcodes", 2056, 24, epf)
    groups = [_ints(ln) for ln in out if ln[0] == "lfgroup"]
    assert len(groups) == 2
    preA = [_bits(ln) for ln in out if ln[0] == "preA"]
    preB = [_bits(ln) for ln in out if ln[0] == "preB"]
    lens = {(int(ln[1]), int(ln[2])): _ints(ln[2:]) for ln in out if ln[0] == "lens"}
    assert len(lens) == 2 * 2 * 4

    def prelude(br, nleaves_want):
        assert not br.read(1) and br.read(1)  # local tree, default weighted-predictor header
        assert br.u32(("v", 0), ("v", 1), ("b", 4, 2), ("b", 8, 18)) == 0  # no transforms
        nodes, nleaves = decoder.read_tree(br)
        assert nleaves == nleaves_want
        return nodes, decoder.EntropyStream(br, nleaves)

    for lg, bw, bh, vcount in groups:
        br = decoder.BitReader(preA[lg][0], 0, preA[lg][1])
        assert br.read(2) == 0  # extra_precision
        nodes, es = prelude(br, 3)
        assert br.pos == preA[lg][1]
        for leaf in range(3):
            assert _lengths(es.codes[es.ctxmap[leaf]]) == lens[(2 * lg, leaf)]
        assert lens[(2 * lg, 3)] == [0] * ALPHA  # (stream A has three leaves)
        br = decoder.BitReader(preB[lg][0], 0, preB[lg][1])
        assert br.read(decoder.ceil_log2(bw * bh)) == vcount - 1
        nodes, es = prelude(br, 4)
        assert br.pos == preB[lg][1]
        for leaf in range(4):
            assert _lengths(es.codes[es.ctxmap[leaf]]) == lens[(2 * lg + 1, leaf)]
        # the EPF tree differs from the plain one in its sharpness leaf's offset
        offsets = sorted(n[3] for n in nodes if n[0] == "leaf")
        assert (4 in offsets) == bool(epf)
