"""Search trace on the GPU (jxg_encode_traced_rgb8 / jxg_search_trace, DESIGN.md
3.20): every estimate the AC-strategy search compared.

1. a traced encode is the plain encode: bytes, maps, reconstruction, rate report;
2. the 8x8 scan's estimates equal the oracle's jxo_quantize_block / jxo_hook_f
   bit for bit;
3. the merged planes equal jxo_varblock, the big planes the oracle's
   debug_big_costs, NaN exactly where no candidate exists;
4. a numpy replay of the search from the planes alone gives the encode's
   strategy map and final estimates;
5. the summary equals a numpy reduction of the planes;
6. refusals.

Bit equality in 2 and 3 is derived, not measured: the kernels' sums follow the
oracle's op order by design, 8 * dist is exact (so contraction could not change
bits + 8 * dist), * tmul is one rounding.
"""
import ctypes

import numpy as np
import pytest

from sweep_cases import cached

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -5
FLT_MAX = np.float32(np.finfo(np.float32).max)
SCAN_IDS = (0, 3, 2, 12, 13, 1)  # DCT8, DCT4X4, DCT2X2, DCT4X8, DCT8X4, IDENTITY
SCAN_INDEX = {t: i for i, t in enumerate(SCAN_IDS)}
# (raw id, blocks down, blocks across), plane order of `merged` and of `big`
MERGED = ((6, 2, 1), (7, 1, 2), (4, 2, 2), (10, 4, 2), (11, 2, 4), (5, 4, 4),
          (19, 8, 4), (20, 4, 8), (18, 8, 8))
BIG = ((22, 16, 8), (23, 8, 16), (21, 16, 16), (25, 32, 16), (26, 16, 32), (24, 32, 32))


def u32(a):
    """float32 array by its bits (NaN == NaN, -0 != +0)"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def natural(w, h, seed=5):
    def make():
        from jxg.synth import natural_rgb8

        img = natural_rgb8(w, h, seed)
        img.setflags(write=False)
        return img

    return cached(("trace_natural", w, h, seed), make)


def flat_edges():
    """synth_rgb8(200, 136, 5): flat areas with straight edges.  With cjxl's
    defaults at d1 some thirty blocks have a homogeneity pair of 0 / 0 or x / 0,
    hook F's factor is inf or NaN there, every compared estimate stops being
    below FLT_MAX and the scan falls back to DCT8 by index -- where the raw
    estimates chose DCT4X8 / DCT8X4: the decisions hook F flips.  (On the
    natural images the factor is a positive finite number per block, which
    cannot reorder the block's six candidates.)"""
    def make():
        from jxg.synth import synth_rgb8

        img = synth_rgb8(200, 136, 5)
        img.setflags(write=False)
        return img

    return cached("trace_flat_edges", make)


def gradient(w, h):
    def make():
        from test_gpu_bigvb import gradient_rgb8

        img = gradient_rgb8(w, h, w * 7 + h)
        img.setflags(write=False)
        return img

    return cached(("trace_gradient", w, h), make)


def traced(jxg, img_key, img, d, e, p, flags):
    """(codestream, stats with maps, trace) of a traced encode on a fresh context"""
    def make():
        with jxg.Encoder(distance=d, effort=e, proposals=p, flags=flags | jxg.FLAG_KEEP_MAPS) as enc:
            data = enc.encode_traced(img)
            st = enc.stats()
            tr = enc.search_trace()
        return data, st, tr

    return cached(("traced", img_key, d, e, p, flags), make)


def beats(ea, ia, eb, ib):
    """front_kernel's order on (estimate, scan index)"""
    va, vb = bool(ea < FLT_MAX), bool(eb < FLT_MAX)
    if va and vb:
        return bool(ea < eb) or (bool(ea == eb) and ia < ib)
    if va != vb:
        return va
    return ia < ib


def scan_winner(e6):
    w = 0
    for i in range(1, 6):
        if beats(e6[i], i, e6[w], w):
            w = i
    return w


def max_level_blocks(effort):
    return 4 if effort == 5 else 8


# ---------------------------------------------------------------------------
# 1. a traced encode is the plain encode
# ---------------------------------------------------------------------------
def _plain_and_traced(jxg, img, d, e, p, flags):
    kw = dict(distance=d, effort=e, proposals=p, flags=flags | jxg.FLAG_KEEP_MAPS)
    with jxg.Encoder(**kw) as enc:
        data = enc.encode(img)
        st = enc.stats()
        rec = enc.reconstruct()
        rate = enc.rate_report(block_map=True)
    with jxg.Encoder(**kw) as enc:
        got = enc.encode_traced(img)
        tst = enc.stats()
        tr = enc.search_trace()
        assert got == data, "traced codestream differs (%d vs %d bytes)" % (len(got), len(data))
        for k in ("acs", "qf", "dc", "ac"):
            assert np.array_equal(tst[k], st[k]), k
        if p & 3:
            assert np.array_equal(u32(tst["homog"]), u32(st["homog"]))
        assert np.array_equal(enc.reconstruct(), rec)
        trate = enc.rate_report(block_map=True)
        assert sorted(trate) == sorted(rate)
        for k in rate:
            assert np.array_equal(trate[k], rate[k]), k
        # the fetch changed nothing, and gives the same bits again
        tr2 = enc.search_trace()
        for k in tr:
            a, b = np.asarray(tr[k]), np.asarray(tr2[k])
            assert np.array_equal(u32(a), u32(b)) if a.dtype == np.float32 else np.array_equal(a, b), k
        assert np.array_equal(enc.reconstruct(), rec)
        # a plain encode on the traced context gives the same bytes again
        assert enc.encode(img) == data
        with pytest.raises(jxg.JxgError):
            enc.search_trace()
    return st, tr


@pytest.mark.parametrize("defaults", [False, True], ids=["flags0", "cjxl_defaults"])
@pytest.mark.parametrize("effort", [5, 6, 7, 8])
def test_traced_encode_is_the_plain_encode(jxg_mod, effort, defaults):
    jxg = jxg_mod
    img = natural(200, 136)
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else 0
    for p in range(4):
        st, tr = _plain_and_traced(jxg, img, 1.0, effort, p, flags)
        assert tr["blocks"] == 25 * 17
        assert tr["max_px"] == {5: 32, 6: 64, 7: 64, 8: 256}[effort]
        if not p & 2:  # without hook F the two planes are one
            assert np.array_equal(u32(tr["cand8_raw"]), u32(tr["cand8"]))


FRAMES = {"136x72": (lambda: natural(136, 72), 1.0, 7, 3, True),
          "264x72": (lambda: natural(264, 72), 3.0, 6, 1, False),
          "512x512": (lambda: gradient(512, 512), 1.0, 8, 2, False),
          "520x776": (lambda: gradient(520, 776), 3.0, 8, 3, True)}


@pytest.mark.parametrize("frame", list(FRAMES))
def test_traced_encode_is_the_plain_encode_other_frames(jxg_mod, frame):
    jxg = jxg_mod
    make, d, e, p, defaults = FRAMES[frame]
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else jxg.FLAG_ANS
    st, tr = _plain_and_traced(jxg, make(), d, e, p, flags)
    if e == 8:  # the big shapes are chosen on these (test_gpu_bigvb.py)
        heads = st["acs"][(st["acs"] & 0x80) == 0]
        assert any(21 <= int(t) <= 26 for t in heads)
        assert np.isfinite(tr["big"]).any()


def test_device_variant_gives_the_same_bytes_and_trace(jxg_mod):
    import torch

    jxg = jxg_mod
    img = natural(200, 136)
    data, st, tr = traced(jxg, "n200", img, 1.0, 7, 3, jxg.FLAGS_CJXL_DEFAULTS)
    stride = 200 * 3 + 24
    buf = torch.zeros((136, stride), dtype=torch.uint8, device="cuda")
    buf[:, :600] = torch.from_numpy(img.reshape(136, 600).copy()).cuda()
    torch.cuda.synchronize()
    with jxg.Encoder(distance=1.0, effort=7, proposals=3, flags=jxg.FLAGS_CJXL_DEFAULTS) as enc:
        assert enc.encode_traced_device(buf.data_ptr(), 200, 136, row_stride=stride) == data
        got = enc.search_trace()
    for k in tr:
        a, b = np.asarray(tr[k]), np.asarray(got[k])
        assert np.array_equal(u32(a), u32(b)) if a.dtype == np.float32 else np.array_equal(a, b), k


# ---------------------------------------------------------------------------
# the oracle's stage functions (oracle/jxo_internal.h) through ctypes
# ---------------------------------------------------------------------------
class _Frame(ctypes.Structure):  # jxo_frame
    _fields_ = [(k, ctypes.c_uint32) for k in ("w", "h", "bxs", "bys", "xp", "yp", "gxs", "gys",
                                               "ngroups", "lfxs", "lfys", "nlf")] + [
        ("distance", ctypes.c_float), ("effort", ctypes.c_int), ("proposals", ctypes.c_uint32),
        ("qf_base", ctypes.c_float), ("inv_g", ctypes.c_float), ("G", ctypes.c_uint32),
        ("qdc", ctypes.c_uint32), ("dc_mul", ctypes.c_float * 3), ("dc_step", ctypes.c_float * 3),
        ("wts", ctypes.c_float * (5 * 3 * 64)), ("sdw", ctypes.c_float * (6 * 3 * 64))]


class _Shape(ctypes.Structure):  # jxo_shape
    _fields_ = [("type", ctypes.c_uint8), ("cy", ctypes.c_uint8), ("cx", ctypes.c_uint8),
                ("kind", ctypes.c_uint8), ("tmul", ctypes.c_float)]


class Stage:
    """the oracle's inputs of one encode: XYB (inverse Gaborish applied where
    the flags ask for it), the frame scalars, chroma-from-luma factors per tile"""

    def __init__(self, oracle, jxg, img, d, e, p, flags, data):
        self.lib = lib = oracle.lib()
        fp = ctypes.POINTER(_Frame)
        lib.jxo_frame_init.argtypes = [fp, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.POINTER(oracle._Params)]
        lib.jxo_frame_init.restype = None
        lib.jxo_quantize_block.argtypes = [fp, ctypes.c_int, ctypes.c_void_p, ctypes.c_float,
                                           ctypes.c_void_p, ctypes.c_void_p]
        lib.jxo_quantize_block.restype = ctypes.c_float
        lib.jxo_varblock.argtypes = [fp, ctypes.POINTER(_Shape), ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]
        lib.jxo_varblock.restype = ctypes.c_float
        lib.jxo_cfl_factors.argtypes = [ctypes.c_int8, ctypes.c_int8, ctypes.c_void_p]
        lib.jxo_cfl_factors.restype = None
        lib.jxo_gab_inverse.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
        lib.jxo_gab_inverse.restype = None
        self.shapes = (_Shape * 15).in_dll(lib, "jxo_shapes")
        h, w, _ = img.shape
        self.xyb = oracle.srgb8_to_xyb(img)
        _, yp, xp = self.xyb.shape
        if flags & jxg.FLAG_GABORISH:
            lib.jxo_gab_inverse(self.xyb.ctypes.data, xp, yp)
        self.f = _Frame()
        prm = oracle._Params(d, e, p, 1 if flags & jxg.FLAG_ANS else 0, 0)
        lib.jxo_frame_init(ctypes.byref(self.f), w, h, ctypes.byref(prm))
        self.cmap = jxg.decode_maps(data)["cmap"]

    def cfl(self, by, bx):
        out = (ctypes.c_float * 2)()
        self.lib.jxo_cfl_factors(int(self.cmap[0, by // 8, bx // 8]), int(self.cmap[1, by // 8, bx // 8]),
                                 out)
        return out

    def scale(self, raw):
        return np.float32(np.float32(self.f.G) * np.float32(raw)) / np.float32(65536.0)

    def block(self, t, by, bx, raw):
        px = np.ascontiguousarray(self.xyb[:, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]).reshape(3, 64)
        return np.float32(self.lib.jxo_quantize_block(ctypes.byref(self.f), t, px.ctypes.data,
                                                      float(self.scale(raw)), None, self.cfl(by, bx)))

    def varblock(self, si, by, bx, raw):
        return np.float32(self.lib.jxo_varblock(ctypes.byref(self.f), ctypes.byref(self.shapes[si]),
                                                self.xyb.ctypes.data, bx * 8, by * 8, int(raw), None,
                                                None, None, self.cfl(by, bx)))


def _hook_f(oracle, e, h3):
    return np.float32(oracle.hook_f(float(e), float(h3[0]), float(h3[1]), float(h3[2])))


# ---------------------------------------------------------------------------
# 2. the 8x8 scan's estimates against the oracle, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("defaults", [False, True], ids=["flags0", "cjxl_defaults"])
@pytest.mark.parametrize("d", [1.0, 3.0])
@pytest.mark.parametrize("p", [0, 3])
def test_scan_estimates_equal_the_oracle(jxg_mod, oracle, p, d, defaults):
    jxg = jxg_mod
    img = natural(136, 72)
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else 0
    data, st, tr = traced(jxg, "n136", img, d, 7, p, flags)
    S = Stage(oracle, jxg, img, d, 7, p, flags, data)
    assert S.f.G == st["global_scale"]
    bad = []
    for by in range(9):
        for bx in range(17):
            raw = int(tr["qf8"][by, bx]) + 1
            for i, t in enumerate(SCAN_IDS):
                want = S.block(t, by, bx, raw)
                got = tr["cand8_raw"][i, by, bx]
                if u32(want) != u32(got):
                    bad.append(("raw", by, bx, t, float(want), float(got)))
                if p & 2:
                    want = _hook_f(oracle, want, st["homog"][by, bx])
                got = tr["cand8"][i, by, bx]
                if u32(want) != u32(got):
                    bad.append(("compared", by, bx, t, float(want), float(got)))
    assert not bad, "%d estimates differ from the oracle, first: %r" % (len(bad), bad[:5])


# ---------------------------------------------------------------------------
# 3. merged and big estimates, bit for bit; NaN exactly where the rules say
# ---------------------------------------------------------------------------
def merged_candidates(bys, bxs, effort):
    """[(plane, by, bx)] of every candidate varblock the merge stage evaluates"""
    out = []
    for si, (_, cy, cx) in enumerate(MERGED):
        s = max(cy, cx)
        if s > max_level_blocks(effort):
            continue
        for by in range(0, bys, cy):
            for bx in range(0, bxs, cx):
                if (by // s + 1) * s <= min(bys, (by // 8 + 1) * 8) and \
                        (bx // s + 1) * s <= min(bxs, (bx // 8 + 1) * 8):
                    out.append((si, by, bx))
    return out


@pytest.mark.parametrize("defaults", [False, True], ids=["flags0", "cjxl_defaults"])
@pytest.mark.parametrize("size", [(136, 72), (200, 136)], ids=["136x72", "200x136"])
@pytest.mark.parametrize("effort", [5, 7])
def test_merged_estimates_equal_the_oracle(jxg_mod, oracle, effort, size, defaults):
    jxg = jxg_mod
    w, h = size
    img = natural(w, h)
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else 0
    bys, bxs = (h + 7) // 8, (w + 7) // 8
    for p in (0, 3):
        data, st, tr = traced(jxg, "n%d" % w, img, 1.0, effort, p, flags)
        S = Stage(oracle, jxg, img, 1.0, effort, p, flags, data)
        cands = merged_candidates(bys, bxs, effort)
        assert cands
        want = np.full((9, bys, bxs), np.nan, np.float32)
        for si, by, bx in cands:
            _, cy, cx = MERGED[si]
            raw = int(tr["qf8"][by:by + cy, bx:bx + cx].max()) + 1
            e = S.varblock(si, by, bx, raw)
            if p & 2:
                e = _hook_f(oracle, e, st["homog"][by, bx])
            want[si, by, bx] = e
        got = tr["merged"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
        diff = np.argwhere(u32(got) != u32(want))
        diff = [tuple(int(v) for v in i) for i in diff if not np.isnan(want[tuple(i)])]
        assert not diff, "%d merged estimates differ, first (plane, by, bx): %r: %r vs %r" % (
            len(diff), diff[0], float(got[diff[0]]), float(want[diff[0]]))
        assert np.isnan(tr["big"]).all()


def big_slots(bys, bxs):
    """{(group, slot of the [25] layout): (plane, by, bx)} of every fitting candidate"""
    out = {}
    gxs = (bxs + 31) // 32
    for L, s in ((0, 16), (1, 32)):
        for by0 in range(0, bys - s + 1, s):
            for bx0 in range(0, bxs - s + 1, s):
                g = (by0 // 32) * gxs + bx0 // 32
                o = ((by0 % 32) // 16 * 2 + (bx0 % 32) // 16) * 5 if L == 0 else 20
                tall, wide, full = 3 * L, 3 * L + 1, 3 * L + 2
                for j, (k, by, bx) in enumerate(((full, by0, bx0), (tall, by0, bx0),
                                                 (tall, by0, bx0 + s // 2), (wide, by0, bx0),
                                                 (wide, by0 + s // 2, bx0))):
                    out[(g, o + j)] = (k, by, bx)
    return out


BIG_CASES = {"512x512_d1_ans": (512, 512, 1.0, False), "520x776_d3_defaults": (520, 776, 3.0, True)}


@pytest.mark.parametrize("case", list(BIG_CASES))
@pytest.mark.parametrize("p", [0, 3], ids=["hookF_off", "hookF_on"])
def test_big_estimates_equal_the_oracle(jxg_mod, oracle, p, case):
    jxg = jxg_mod
    w, h, d, defaults = BIG_CASES[case]
    img = gradient(w, h)
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else jxg.FLAG_ANS
    data, st, tr = traced(jxg, "g%d" % w, img, d, 8, p, flags)
    ref, costs = oracle.debug_big_costs(np.array(img), d, 8, p, 1, 7 if defaults else 0)
    assert data == ref.bytes
    bys, bxs = (h + 7) // 8, (w + 7) // 8
    want = np.full((6, bys, bxs), np.nan, np.float32)
    slots = big_slots(bys, bxs)
    for g in range(costs.shape[0]):
        for o in range(25):
            if (g, o) in slots:
                want[slots[(g, o)]] = costs[g, o]
            else:
                assert np.isnan(costs[g, o])  # the oracle evaluated nothing there either
    got = tr["big"]
    assert not np.isinf(got).any(), "a traced job evaluates every candidate in full"
    assert not np.isnan(want[[k for k, _, _ in slots.values()],
                             [y for _, y, _ in slots.values()],
                             [x for _, _, x in slots.values()]]).any()
    assert np.array_equal(u32(got), u32(want)), "%d big estimates differ" % int(
        (u32(got) != u32(want)).sum())


# ---------------------------------------------------------------------------
# 4. the trace explains the encode: a replay from the planes alone
# ---------------------------------------------------------------------------
def _sum_raster(ent, by0, bx0, s):
    cur = np.float32(0.0)
    with np.errstate(over="ignore"):  # (FLT_MAX + FLT_MAX = inf, as on the device)
        for v in ent[by0:by0 + s, bx0:bx0 + s].ravel():
            cur = np.float32(cur + v)
    return cur


def _try_merge(acs, ent, by0, bx0, s, ids, e):
    """the TryMergeAcs comparison of one s x s region: e = the five candidates'
    estimates (full, tall left / right, wide top / bottom)"""
    cur = _sum_raster(ent, by0, bx0, s)
    et, ew = np.float32(e[1] + e[2]), np.float32(e[3] + e[4])
    best, choice = cur, 0
    for c, v in ((1, e[0]), (2, et), (3, ew)):
        if not v >= best:
            best, choice = v, c
    if not choice:
        return
    tall, wide, full = ids
    h = s // 2
    vbs = {1: [(full, s, s, by0, bx0, e[0])],
           2: [(tall, s, h, by0, bx0, e[1]), (tall, s, h, by0, bx0 + h, e[2])],
           3: [(wide, h, s, by0, bx0, e[3]), (wide, h, s, by0 + h, bx0, e[4])]}[choice]
    for t, cy, cx, by, bx, est in vbs:
        acs[by:by + cy, bx:bx + cx] = t | 0x80
        ent[by:by + cy, bx:bx + cx] = 0.0
        acs[by, bx] = t
        ent[by, bx] = est


def replay(tr, effort):
    """(scan winners' ids, final strategy map, final estimates) from the planes"""
    _, bys, bxs = tr["cand8"].shape
    scan = np.zeros((bys, bxs), np.uint8)
    ent = np.zeros((bys, bxs), np.float32)
    for by in range(bys):
        for bx in range(bxs):
            e6 = tr["cand8"][:, by, bx]
            w = scan_winner(e6)
            scan[by, bx] = SCAN_IDS[w]
            # (the scan's best starts at FLT_MAX: what is not below it never replaces it)
            ent[by, bx] = e6[w] if e6[w] < FLT_MAX else FLT_MAX
    # hook P: the front kernel's byte where it overrode a DCT8 win
    acs = tr["front8"].copy()
    assert ((acs == scan) | (scan == 0)).all()
    with np.errstate(invalid="ignore"):
        for L, s in enumerate((2, 4, 8)):
            if s > max_level_blocks(effort):
                break
            for by0 in range(0, bys, s):
                for bx0 in range(0, bxs, s):
                    if by0 + s > min(bys, (by0 // 8 + 1) * 8) or bx0 + s > min(bxs, (bx0 // 8 + 1) * 8):
                        continue
                    m, h = tr["merged"], s // 2
                    e = (m[3 * L + 2, by0, bx0], m[3 * L, by0, bx0], m[3 * L, by0, bx0 + h],
                         m[3 * L + 1, by0, bx0], m[3 * L + 1, by0 + h, bx0])
                    _try_merge(acs, ent, by0, bx0, s, [MERGED[3 * L + i][0] for i in range(3)], e)
        if effort >= 8:
            for L, s in enumerate((16, 32)):
                for by0 in range(0, bys - s + 1, s):
                    for bx0 in range(0, bxs - s + 1, s):
                        m, h = tr["big"], s // 2
                        e = (m[3 * L + 2, by0, bx0], m[3 * L, by0, bx0], m[3 * L, by0, bx0 + h],
                             m[3 * L + 1, by0, bx0], m[3 * L + 1, by0 + h, bx0])
                        _try_merge(acs, ent, by0, bx0, s, [BIG[3 * L + i][0] for i in range(3)], e)
    return scan, acs, ent


REPLAY = {"e5": (lambda: natural(200, 136), "n200", 1.0, 5, False),
          "e7": (lambda: natural(200, 136), "n200", 1.0, 7, True),
          "e7_flat_edges": (flat_edges, "s200", 1.0, 7, True),
          "e8_512": (lambda: gradient(512, 512), "g512", 1.0, 8, False),
          "e8_520x776": (lambda: gradient(520, 776), "g520", 3.0, 8, True)}


@pytest.mark.parametrize("case", list(REPLAY))
@pytest.mark.parametrize("p", [0, 3])
def test_the_trace_explains_the_encode(jxg_mod, p, case):
    jxg = jxg_mod
    make, key, d, e, defaults = REPLAY[case]
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else (jxg.FLAG_ANS if e == 8 else 0)
    data, st, tr = traced(jxg, key, make(), d, e, p, flags)
    scan, acs, ent = replay(tr, e)
    assert np.array_equal(scan, tr["scan8"])
    assert np.array_equal(acs, st["acs"]), "%d strategy bytes differ" % int((acs != st["acs"]).sum())
    assert np.array_equal(u32(ent), u32(tr["chosen"]))
    if not p & 1:
        assert np.array_equal(tr["front8"], tr["scan8"])
    assert (st["acs"] & 0x80).any(), "no merged varblock: the case shows nothing"
    if case == "e7_flat_edges" and p == 3:  # estimates that are not below FLT_MAX take part
        assert not np.isfinite(tr["cand8"]).all()


# ---------------------------------------------------------------------------
# 5. the summary
# ---------------------------------------------------------------------------
def summarize(tr, acs):
    _, bys, bxs = tr["cand8"].shape
    out = {"flip": np.zeros((6, 6), np.uint32), "hook_p": np.zeros(6, np.uint32),
           "merged_over": np.zeros(6, np.uint32), "margin": np.zeros((6, 8), np.uint32),
           "margin_skipped": np.zeros(6, np.uint32)}
    for by in range(bys):
        for bx in range(bxs):
            e6 = tr["cand8"][:, by, bx]
            sw = SCAN_INDEX[int(tr["scan8"][by, bx])]
            out["flip"][scan_winner(tr["cand8_raw"][:, by, bx]), sw] += 1
            if tr["front8"][by, bx] != tr["scan8"][by, bx]:
                out["hook_p"][SCAN_INDEX[int(tr["front8"][by, bx])]] += 1
            if int(acs[by, bx] & 0x7F) not in SCAN_INDEX:
                out["merged_over"][sw] += 1
            b1 = scan_winner(e6)
            b2 = 1 if b1 == 0 else 0
            for i in range(6):
                if i != b1 and i != b2 and beats(e6[i], i, e6[b2], b2):
                    b2 = i
            best, second = e6[b1], e6[b2]
            if not best < FLT_MAX or best <= 0:
                out["margin_skipped"][sw] += 1
            else:
                with np.errstate(over="ignore"):
                    n = sum(bool(second >= np.float32(best * np.float32(1.0 + 2.0 ** -k)))
                            for k in range(7))
                out["margin"][sw, n] += 1
    return out


SUMMARY = {"n200_e5": (lambda: natural(200, 136), "n200", 1.0, 5, False),
           "n200_e7": (lambda: natural(200, 136), "n200", 1.0, 7, True),
           "n136_e7_d3": (lambda: natural(136, 72), "n136", 3.0, 7, False),
           "s200_e7": (flat_edges, "s200", 1.0, 7, True),
           "g512_e8": (lambda: gradient(512, 512), "g512", 1.0, 8, False)}


@pytest.mark.parametrize("case", list(SUMMARY))
@pytest.mark.parametrize("p", [0, 3])
def test_summary_equals_a_reduction_of_the_planes(jxg_mod, p, case):
    jxg = jxg_mod
    make, key, d, e, defaults = SUMMARY[case]
    flags = jxg.FLAGS_CJXL_DEFAULTS if defaults else (jxg.FLAG_ANS if e == 8 else 0)
    data, st, tr = traced(jxg, key, make(), d, e, p, flags)
    want = summarize(tr, st["acs"])
    nb = st["acs"].size
    assert tr["blocks"] == nb
    for k, v in want.items():
        assert np.array_equal(tr[k], v), (k, tr[k], v)
    assert np.array_equal(tr["margin"].sum(1) + tr["margin_skipped"], tr["flip"].sum(0))
    assert int(tr["flip"].sum()) == nb
    if p == 0:
        assert not (tr["flip"] - np.diag(np.diag(tr["flip"]))).any()
        assert not tr["hook_p"].any()
    if case == "s200_e7" and p == 3:
        assert tr["margin_skipped"].any()


def test_both_hooks_show_in_the_summary(jxg_mod):
    """proposals 3 at d1 e7 with cjxl's defaults: hook F flips decisions and hook
    P overrides DCT8 wins.  The 200 x 136 natural image shows no flip (219 + 4 +
    77 + 49 + 43 + 33 blocks on the diagonal, 56 overrides), so the image is
    flat_edges(), of the same size (the counts are recorded in DESIGN.md 3.20)"""
    jxg = jxg_mod
    data, st, tr = traced(jxg, "s200", flat_edges(), 1.0, 7, 3, jxg.FLAGS_CJXL_DEFAULTS)
    off = tr["flip"] - np.diag(np.diag(tr["flip"]))
    print("flip:\n%r\nhook_p %r merged_over %r\nmargin:\n%r\nskipped %r" % (
        tr["flip"], tr["hook_p"], tr["merged_over"], tr["margin"], tr["margin_skipped"]))
    assert off.any(), "hook F flipped nothing"
    assert tr["hook_p"].any(), "hook P overrode nothing"


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def _raw_traced(jxg, enc, img):
    h, w, _ = img.shape
    buf = jxg._Buffer()
    st = jxg.load().jxg_encode_traced_rgb8(enc._ctx, img.ctypes.data, w, h, w * 3, ctypes.byref(buf))
    return st, buf


def test_effort_4_is_unsupported_and_touches_nothing(jxg_mod):
    jxg = jxg_mod
    img = np.array(natural(200, 136))
    with jxg.Encoder(distance=1.0, effort=4) as enc:
        enc.encode(img)
        rec = enc.reconstruct()
        st, buf = _raw_traced(jxg, enc, img)
        assert st == UNSUPPORTED and not buf.data and buf.size == 0
        assert np.array_equal(enc.reconstruct(), rec)
        assert jxg.load().jxg_search_trace(enc._ctx, None, None) == INVALID_ARG


def test_search_trace_needs_a_traced_encode(jxg_mod):
    jxg = jxg_mod
    lib = jxg.load()
    img = np.array(natural(200, 136))
    s = jxg._TraceSummary()
    with jxg.Encoder(distance=1.0, effort=7, flags=jxg.FLAG_KEEP_MAPS) as enc:
        trace = lambda: lib.jxg_search_trace(enc._ctx, None, ctypes.byref(s))  # noqa: E731
        assert trace() == INVALID_ARG  # no encode at all
        data = enc.encode_traced(img)
        assert trace() == 0 and s.blocks == 25 * 17
        assert lib.jxg_search_trace(enc._ctx, None, None) == 0
        acs = enc.stats()["acs"]
        assert enc.encode(img) == data
        assert trace() == INVALID_ARG  # a plain encode
        enc.encode_traced(img)
        assert trace() == 0
        enc.encode_forced(img, acs)
        assert trace() == INVALID_ARG  # a forced encode
        enc.encode_traced(img)
        enc.decode(data)
        assert trace() == INVALID_ARG  # a decode
        enc.encode_traced(img)
        enc.warmup(200, 136)
        assert trace() == INVALID_ARG  # a warm-up encode
        enc.encode_traced(img)
        enc.submit(img)
        assert trace() == INVALID_ARG  # a frame pending
        st, buf = _raw_traced(jxg, enc, img)
        assert st == INVALID_ARG and not buf.data
        enc.receive()
        assert trace() == INVALID_ARG  # a streamed encode
        assert enc.encode_traced(img) == data
        assert trace() == 0


def test_null_arguments(jxg_mod):
    jxg = jxg_mod
    lib = jxg.load()
    img = np.array(natural(200, 136))
    buf = jxg._Buffer()
    with jxg.Encoder(distance=1.0, effort=7) as enc:
        for fn in (lib.jxg_encode_traced_rgb8, lib.jxg_encode_traced_rgb8_device):
            assert fn(None, img.ctypes.data, 200, 136, 600, ctypes.byref(buf)) == INVALID_ARG
            assert fn(enc._ctx, None, 200, 136, 600, ctypes.byref(buf)) == INVALID_ARG
            assert fn(enc._ctx, img.ctypes.data, 200, 136, 600, None) == INVALID_ARG
            assert fn(enc._ctx, img.ctypes.data, 200, 136, 599, ctypes.byref(buf)) == INVALID_ARG
            assert fn(enc._ctx, img.ctypes.data, 0, 136, 600, ctypes.byref(buf)) == INVALID_ARG
        assert lib.jxg_search_trace(None, None, None) == INVALID_ARG
