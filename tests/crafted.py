"""Crafted codestreams: every varblock placement the decoder accepts, written
from hand-made maps by the oracle's encode_maps (oracle/encode.c
jxo_encode_maps) -- streams no encoder writes from an image.  A helper module
of tests/test_crafted_streams.py (CPU) and tests/test_gpu_crafted.py.

A case starts from the oracle's effort-4 encode of a smooth mid-grey frame
(in-gamut DC, a quant field, chroma-from-luma factors), replaces the strategy
map by the crafted layout (a block's DC is its mean under any strategy, so the
DC image stays valid), gives every varblock its head's qf and a few seeded
non-zero coefficients per channel.  Nothing is stored: the cases are seeded.

Families:
  S1  every placement inside a 64x64 tile of the nine shapes up to 64 px (267),
      one per tile of five 512x512 frames, the other blocks the six 8x8-class
      ids in rotation
  S2  the 128 / 256 px shapes at aligned and unaligned offsets of a pass group
  S3  merged shapes flush with the right edge, the bottom edge and the corner
      of 72x200 / 200x72 (9x25 / 25x9 blocks) and 96x224 / 224x96 (12x28 / 28x12)
      frames, Gaborish + 3 EPF passes
  S4  value extremes (maps only: the pixels leave the gamut)
  S5  a coefficient of 32768: the decoder's own limit
  REFUSED  placements that cross a tile / pass group: the host parse refuses them
"""
import functools
import time

import numpy as np

CLASS8 = (0, 1, 2, 3, 12, 13)
# raw id -> (blocks down, blocks across)
TILE_SHAPES = {6: (2, 1), 7: (1, 2), 4: (2, 2), 10: (4, 2), 11: (2, 4), 5: (4, 4),
               19: (8, 4), 20: (4, 8), 18: (8, 8)}
BIG_SHAPES = {22: (16, 8), 23: (8, 16), 21: (16, 16), 25: (32, 16), 26: (16, 32), 24: (32, 32)}
SHAPES = {**TILE_SHAPES, **BIG_SHAPES}
S1_ORDER = (4, 5, 6, 7, 10, 11, 18, 19, 20)

# 8x8-class blocks keep the base encode's quant field (93 - 95 raw at these
# distances) and get coefficients of these magnitudes (quantized units) per
# channel X, Y, B.  Merged varblocks get a crafted, coarse quant field instead
# (raw qf + 1 of 8 - 12, so a step of 1 in qf is a change of about a tenth) and
# coefficients of +-1: MERGED_N of them per channel.  A coefficient's amplitude
# goes with value / (qf + 1): a Y coefficient of 1 at raw 10 moves pixels by
# some 40 levels, an X one would move them by hundreds, so the merged
# varblocks' X gets its content through chroma from luma (CMAP_X) only.  The
# sensitivity test of test_crafted_streams.py holds these choices to what
# they are for; the gamut and f32 self-difference tests to what they may cost.
MAG8 = ((1, 2), (3, 6), (2, 4))
MERGED_QF = (7, 11)
MERGED_N = (0, 2, 1)
CMAP_X, CMAP_B = (-2, 2), (-4, 4)  # crafted ytox, ytob per tile


class Case:
    """one crafted frame: geometry, stream parameters and the five maps"""

    def __init__(self, name, family, w, h, distance, coder, filters, pixels=True):
        self.name, self.family, self.w, self.h = name, family, w, h
        self.distance, self.coder, self.filters, self.pixels = distance, coder, filters, pixels
        self.heads = []  # (id, block row, block column) of the merged varblocks placed

    def __repr__(self):
        return "Case(%s)" % self.name


def grey_rgb8(w, h):
    """smooth mid-grey frame"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 128 + 10 * np.sin(x / 97.0 + y / 131.0)
    return np.repeat(np.clip(v, 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)


def shape_of(t):
    return SHAPES.get(int(t) & 0x7F, (1, 1))


def place(acs, t, by, bx):
    """write a varblock's head and cover flags; its blocks must be unclaimed (255)"""
    cy, cx = shape_of(t)
    assert by + cy <= acs.shape[0] and bx + cx <= acs.shape[1], (t, by, bx)
    assert np.all(acs[by:by + cy, bx:bx + cx] == 255), "overlap at %r" % ((t, by, bx),)
    acs[by:by + cy, bx:bx + cx] = t | 0x80
    acs[by, bx] = t


def fill_rest(acs, ids=CLASS8, shift=0):
    """unclaimed blocks get the given 8x8-class ids in rotation"""
    bys, bxs = acs.shape
    yy, xx = np.mgrid[0:bys, 0:bxs]
    # position in the tile + tile number: over the tiles of a frame every id
    # comes to every block position of a tile
    rot = np.array(ids, np.uint8)[((yy % 8) * 8 + xx % 8 + (yy // 8) * ((bxs + 7) // 8) + xx // 8
                                   + shift) % len(ids)]
    acs[acs == 255] = rot[acs == 255]


def heads_of(acs):
    """[(id, by, bx)] of every varblock, raster order"""
    ys, xs = np.nonzero((acs & 0x80) == 0)
    return [(int(acs[y, x]), int(y), int(x)) for y, x in zip(ys, xs)]


def coef_slot(by, bx, cx, k):
    """(block row, block column, slot) of natural-order position k of the varblock at (by, bx)"""
    sl = k >> 6
    return by + sl // cx, bx + sl % cx, k & 63


def seed_coefficients(case, rng):
    """qf constant per varblock; a few non-zero coefficients per varblock and
    channel at low natural-order positions (the Python reference reads a token
    per position up to the last non-zero one); seeded chroma-from-luma factors"""
    acs = case.acs
    ac = np.zeros(acs.shape + (3, 64), np.int32)
    for t, by, bx in heads_of(acs):
        cy, cx = shape_of(t)
        cb = cy * cx
        if cb > 1:
            case.qf[by:by + cy, bx:bx + cx] = int(rng.integers(MERGED_QF[0], MERGED_QF[1] + 1))
        span = 12 if cb == 1 else min(64 * cb - cb, max(24, 6 * cb))
        for c in range(3):
            if cb == 1:
                n = 1 if (c == 1 or rng.random() < 0.25) else 0
                lo, hi = MAG8[c]
            else:
                n = MERGED_N[c]
                lo, hi = 1, 1
            for k in cb + rng.choice(span, size=n, replace=False):
                y, x, s = coef_slot(by, bx, cx, int(k))
                ac[y, x, c, s] = int(rng.integers(lo, hi + 1)) * (1 if rng.random() < 0.5 else -1)
    case.ac = ac
    case.cmap[0] = rng.integers(CMAP_X[0], CMAP_X[1] + 1, size=case.cmap[0].shape)
    case.cmap[1] = rng.integers(CMAP_B[0], CMAP_B[1] + 1, size=case.cmap[1].shape)


@functools.lru_cache(maxsize=None)
def _base(w, h, distance, coder, filters):
    import oracle_ffi

    return oracle_ffi.encode(grey_rgb8(w, h), distance, 4, 0, coder, filters)


def make_case(name, family, w, h, distance, coder, filters, heads, seed, pixels=True,
              rest=CLASS8):
    """heads: [(id, block row, block column)] of the merged varblocks"""
    base = _base(w, h, distance, coder, filters)
    case = Case(name, family, w, h, distance, coder, filters, pixels)
    acs = np.full((base.bys, base.bxs), 255, np.uint8)
    for t, by, bx in heads:
        place(acs, t, by, bx)
    fill_rest(acs, rest, seed)
    case.heads = list(heads)
    case.acs, case.qf, case.dc, case.cmap = acs, base.qf.copy(), base.dc.copy(), base.cmap.copy()
    seed_coefficients(case, np.random.default_rng(0xC4AF7ED0 + seed))
    return case


# ---------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------
def s1_placements():
    """(id, row, column inside a tile) of every position the tile rule accepts: 267"""
    out = []
    for t in S1_ORDER:
        cy, cx = TILE_SHAPES[t]
        out += [(t, oy, ox) for oy in range(9 - cy) for ox in range(9 - cx)]
    return out


# S1 frames: (coder, filters) -- ANS / prefix codes and filters off / all on alternate
S1_FRAMES = ((1, 0), (0, 3), (1, 3), (0, 0), (1, 3))
S1_DISTANCES = (4.0, 6.0, 5.0, 8.0, 7.0)


def s1_cases():
    pl = s1_placements()
    # interleave the shapes over the frames, so every frame holds every size
    pl = [pl[i] for i in np.random.default_rng(267).permutation(len(pl))]
    cases = []
    for f in range(5):
        heads = [(t, (i // 8) * 8 + oy, (i % 8) * 8 + ox)
                 for i, (t, oy, ox) in enumerate(pl[f * 64:(f + 1) * 64])]
        coder, filters = S1_FRAMES[f]
        cases.append(make_case("s1_%d" % f, "S1", 512, 512, S1_DISTANCES[f], coder, filters,
                               heads, 100 + f))
    return cases


def unaligned_count(case):
    """placements of a case that no encoder makes: off the shape's own grid"""
    n = 0
    for t, by, bx in case.heads:
        cy, cx = shape_of(t)
        n += bool(by % cy or bx % cx)
    return n


# S2: (name, distance, coder, filters, [(id, row, column inside the pass group)] for the
# four pass groups of a 512x512 frame in raster order)
S2_FRAMES = (
    ("s2_128", 4.0, 1, 0, ((21, 0, 0), (21, 16, 16), (21, 3, 5), (21, 16, 7))),
    ("s2_128x64", 6.0, 0, 3, ((22, 0, 0), (22, 16, 24), (22, 5, 3), (22, 11, 21))),
    ("s2_64x128", 5.0, 1, 0, ((23, 0, 0), (23, 24, 16), (23, 3, 5), (23, 21, 11))),
    ("s2_256", 8.0, 0, 0, ((24, 0, 0), (25, 0, 0), (25, 0, 7), (25, 0, 16))),
    ("s2_128x256", 7.0, 1, 3, ((26, 0, 0), (26, 7, 0), (26, 16, 0), (21, 9, 2))),
)


def s2_cases():
    cases = []
    for i, (name, d, coder, filters, groups) in enumerate(S2_FRAMES):
        heads = [(t, (g // 2) * 32 + oy, (g % 2) * 32 + ox) for g, (t, oy, ox) in enumerate(groups)]
        cases.append(make_case(name, "S2", 512, 512, d, coder, filters, heads, 200 + i, rest=(0,)))
    return cases


def cell_of(t):
    return 32 if t >= 21 else 8


def accepted(t, by, bx, bys, bxs):
    """the decoder's placement rule (csrc/jxg_decode.cpp decode_lf_group)"""
    cy, cx = shape_of(t)
    cell = cell_of(t)
    return (by >= 0 and bx >= 0 and by + cy <= bys and bx + cx <= bxs and
            by % cell + cy <= cell and bx % cell + cx <= cell)


def s3_placements(bys, bxs):
    """every merged shape, where the rule accepts it, flush with the right edge (at
    an odd row), the bottom edge (at an odd column) and the corner"""
    out = []
    for t in sorted(SHAPES):
        cy, cx = shape_of(t)
        right = [(t, by, bxs - cx) for by in (1, 3, 9, 0) if accepted(t, by, bxs - cx, bys, bxs)
                 and by + cy < bys]
        bottom = [(t, bys - cy, bx) for bx in (1, 3, 9, 0) if accepted(t, bys - cy, bx, bys, bxs)
                  and bx + cx < bxs]
        corner = [(t, bys - cy, bxs - cx)] if accepted(t, bys - cy, bxs - cx, bys, bxs) else []
        out += right[:1] + bottom[:1] + corner
    return out


# 9x25 / 25x9 blocks: one block in the last tile column / row, so only shapes one block
# wide / tall and 128x64 / 64x128 fit flush; 12x28 / 28x12: four blocks there, the shapes
# up to 32 px fit
S3_SIZES = ((72, 200), (200, 72), (96, 224), (224, 96))


def s3_cases():
    """the placements of each frame size packed into as few streams as do not overlap"""
    cases = []
    for w, h in S3_SIZES:
        bys, bxs = h // 8, w // 8
        left = s3_placements(bys, bxs)
        n = 0
        while left:
            used = np.zeros((bys, bxs), bool)
            heads, rest = [], []
            for t, by, bx in left:
                cy, cx = shape_of(t)
                if used[by:by + cy, bx:bx + cx].any():
                    rest.append((t, by, bx))
                else:
                    used[by:by + cy, bx:bx + cx] = True
                    heads.append((t, by, bx))
            cases.append(make_case("s3_%dx%d_%d" % (w, h, n), "S3", w, h, 6.0, n % 2, 3, heads,
                                   300 + 10 * len(cases)))
            left = rest
            n += 1
    return cases


def s4_cases():
    cases = []
    rng = np.random.default_rng(4)

    def nonzero(shape):
        v = rng.integers(1, 40, size=shape).astype(np.int32)
        return np.where(rng.random(shape) < 0.5, v, -v)

    # every AC coefficient of a 64x64 varblock non-zero (DCT64X64 is raw id 18)
    c = make_case("s4_dense64", "S4", 64, 64, 6.0, 1, 0, [(18, 0, 0)], 400, pixels=False)
    c.ac = nonzero(c.ac.shape)
    c.ac[0, 0, :, :] = 0  # the 64 slots the DC image carries
    cases.append(c)
    # a tile of DCT8 blocks with all 63
    c = make_case("s4_dense8", "S4", 64, 64, 6.0, 0, 0, [], 401, pixels=False, rest=(0,))
    c.ac = nonzero(c.ac.shape)
    c.ac[:, :, :, 0] = 0
    cases.append(c)
    # the ends of int16
    c = make_case("s4_int16", "S4", 64, 64, 6.0, 1, 3, [(4, 1, 3), (11, 5, 2)], 402, pixels=False)
    nzy, nzx, nzc, nzk = np.nonzero(c.ac)
    ends = (32767, -32767, -32768)
    for i in range(len(nzy)):
        c.ac[nzy[i], nzx[i], nzc[i], nzk[i]] = ends[i % 3]
    cases.append(c)
    # qf 0 and 255 side by side, EPF on
    c = make_case("s4_qf", "S4", 64, 64, 6.0, 0, 3, [(4, 2, 2), (7, 6, 5)], 403, pixels=False)
    for t, by, bx in heads_of(c.acs):
        cy, cx = shape_of(t)
        c.qf[by:by + cy, bx:bx + cx] = 255 * ((by + bx) & 1)
    assert set(np.unique(c.qf)) == {0, 255}
    cases.append(c)
    # chroma from luma at the ends of int8, two tiles
    c = make_case("s4_cmap", "S4", 128, 64, 6.0, 1, 0, [(5, 3, 1), (10, 2, 13)], 404, pixels=False)
    c.cmap[:, 0, 0] = (-128, 127)
    c.cmap[:, 0, 1] = (127, -128)
    cases.append(c)
    # dc at the ends of the range the oracle's DC coding accepts
    import oracle_ffi

    c = make_case("s4_dc", "S4", 64, 64, 6.0, 0, 0, [(6, 0, 7), (4, 5, 5)], 405, pixels=False)
    ends = np.array((oracle_ffi.MAPS_DC_MIN, oracle_ffi.MAPS_DC_MAX, 0, -1), np.int32)
    c.dc[:] = ends[rng.integers(0, 4, size=c.dc.shape)]
    c.dc[:, 0, :4] = ends[None, :]
    cases.append(c)
    return cases


def s5_case():
    c = make_case("s5_32768", "S5", 64, 64, 6.0, 1, 0, [(4, 1, 3)], 500, pixels=False)
    y, x, s = coef_slot(1, 3, 2, 9)
    c.ac[y, x, 1, s] = 32768
    return c


def refused_cases():
    """placements the maps allow and the decoder's tile / pass-group rule does not"""
    return [make_case("refused_tile", "REFUSED", 128, 128, 6.0, 1, 0, [(4, 7, 7)], 600),
            make_case("refused_group", "REFUSED", 512, 512, 6.0, 0, 0, [(21, 24, 24)], 601,
                      rest=(0,)),
            make_case("refused_64_at_1_0", "REFUSED", 128, 128, 6.0, 1, 0, [(18, 1, 0)], 602)]


@functools.lru_cache(maxsize=None)
def families():
    """{family: [Case]} of S1 - S4, built once"""
    return {"S1": s1_cases(), "S2": s2_cases(), "S3": s3_cases(), "S4": s4_cases()}


def all_cases():
    f = families()
    return f["S1"] + f["S2"] + f["S3"] + f["S4"]


def pixel_cases():
    return [c for c in all_cases() if c.pixels]


def most_unaligned_s1():
    return max(families()["S1"], key=unaligned_count)


_streams = {}


def stream(case, cache=True) -> bytes:
    """the case's codestream, written once (cache=False: from the maps as they are now)"""
    if not cache or case.name not in _streams:
        import oracle_ffi

        r = oracle_ffi.encode_maps(case.w, case.h, case.acs, case.qf, case.dc, case.ac, case.cmap,
                                   case.distance, case.coder, case.filters)
        case.global_scale, case.quant_dc = r.global_scale, r.quant_dc
        if not cache:
            return r.bytes
        _streams[case.name] = r.bytes
    return _streams[case.name]


# ---------------------------------------------------------------------------
# the float64 reference, and the same rounded to f32 between its stages
# ---------------------------------------------------------------------------
MAPS = ("acs", "qf", "dc", "ac", "cmap")


def decoded_maps(d):
    """the maps of a jxl_decode.Decoded in the layout of the crafted ones (its qf is raw)"""
    return {"acs": d.acs.astype(np.uint8), "qf": (d.qf - 1).astype(np.uint8),
            "dc": d.dc.astype(np.int32), "ac": d.ac.astype(np.int32), "cmap": d.cmap.astype(np.int8)}


_refs = {}


def reference(case):
    """(jxl_decode.Decoded of the stream with its float64 image, seconds it took), once"""
    if case.name not in _refs:
        import jxl_decode

        t0 = time.perf_counter()
        d = jxl_decode.decode(stream(case), want_pixels=False)
        d.rgb = jxl_decode.reconstruct(d)
        d.rgb.setflags(write=False)
        _refs[case.name] = (d, time.perf_counter() - t0)
    return _refs[case.name]


def reconstruct_f32(d):
    """jxl_decode.reconstruct with its planes rounded to f32 between the stages
    (after the inverse transforms, after Gaborish, after every EPF pass): what
    any f32 implementation of the same arithmetic may differ by"""
    import jxl_decode as J

    def r32(p):
        return np.asarray(p, np.float64).astype(np.float32).astype(np.float64)

    saved = J.gaborish, J._epf_step, J.xyb_to_srgb8
    try:
        J.gaborish = lambda P: r32(saved[0](r32(P)))
        J._epf_step = lambda planes, *a, **k: [r32(o) for o in saved[1]([r32(p) for p in planes],
                                                                         *a, **k)]
        J.xyb_to_srgb8 = lambda X, Y, B: saved[2](r32(X), r32(Y), r32(B))
        return J.reconstruct(d)
    finally:
        J.gaborish, J._epf_step, J.xyb_to_srgb8 = saved


def tile_shares(a, b):
    """(largest |difference|, differing share over the frame, the worst differing
    share of one 64x64 tile) of two (H, W, 3) uint8 images; an edge tile's share
    is over the samples it has"""
    diff = np.abs(a.astype(np.int32) - b.astype(np.int32))
    worst = 0.0
    for y in range(0, diff.shape[0], 64):
        for x in range(0, diff.shape[1], 64):
            t = diff[y:y + 64, x:x + 64]
            worst = max(worst, float(np.count_nonzero(t)) / t.size)
    return int(diff.max()), float(np.count_nonzero(diff)) / diff.size, worst
