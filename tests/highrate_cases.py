"""Frames and settings for distances below 0.1 (helper of test_highrate_cases.py,
test_gpu_highrate.py and test_oracle_ubsan.py; not a conftest).

The library accepts 0 < distance <= 25 and computes with max(distance, 1e-6)
(include/jxg.h JXG_MIN_DISTANCE).  Down there the quantizers clamp at +-32767,
the token record (csrc/jxg_acrec.h: cluster | tok << 8 | nbits << 14 | bits
<< 18) is at the edge of every field (|q| = 32767 -> tok 63, nbits 13), the raw
quant field is at its ceiling of 256 (stored 255) and the global scale at its
clamp of 73727 for distance <= 0.79 * 1024 / 73727 = 0.010972.

A setting is (effort, proposals, coder, oracle filter mask): coder 1 = ANS,
mask 7 = cjxl's defaults (Gaborish, EPF, the masking quant field), mask 0 with
coder 0 = the plain preset.  CASES lists (image, distance, setting); what each
case reaches is asserted from the oracle's maps in test_highrate_cases.py
(EDGES there), so a changed image fails instead of going soft.

What X and B reach: in the edge, triangle and white-noise frames only Y gets
to 16384 (X at most 10096, white72 at the floor under cjxl's defaults; B at most
10780, half264 in merged varblocks of the plain preset).  Two-colour edges do
not help -- chroma from luma removes what follows Y (blue | yellow halves: B
95) -- but noise over the eight corners of the sRGB cube in 2x2 cells does:
`corners72` reaches X 17735, Y 32767 (clamped) and B 21487 at 0.001 under
cjxl's defaults, all three channels in the top token class in one frame.
"""
import functools

import numpy as np

ANS, PREFIX = 1, 0
CJXL7 = (7, 3, ANS, 7)     # cjxl's defaults, effort 7, both proposals
PLAIN5 = (5, 3, PREFIX, 0)  # plain preset, merges up to 32 px
CJXL8 = (8, 0, ANS, 7)     # effort 8: the 128 / 256 px levels
PLAIN7 = (7, 0, PREFIX, 0)
SETTINGS = (CJXL7, PLAIN5, CJXL8, PLAIN7)

CLASS8 = (0, 1, 2, 3, 12, 13)  # strategy codes of the 8x8 class; every other code is merged
G_CLAMP = 73727
FLOOR = 1e-6  # JXG_MIN_DISTANCE / JXO_MIN_DISTANCE


def setting_id(s):
    return "e%d_p%d_%s_m%d" % (s[0], s[1], "ans" if s[2] else "prefix", s[3])


def white72():
    return np.random.default_rng(3).integers(0, 256, (40, 72, 3), dtype=np.uint8)


def half(w, h):
    img = np.zeros((h, w, 3), dtype=np.uint8)
    img[:, w // 2 + 5:] = 255
    return img


def tri64(w=264, h=200):
    y, x = np.mgrid[0:h, 0:w]
    t = np.abs(((x + y // 3) % 64) - 32) / 32.0 * 255.0
    g = np.rint(t).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


def two_colours(w, h, left, right):
    """`left` before column w // 2 + 5 and `right` from it on; the rows from
    h // 2 + 3 down mirrored left-right"""
    img = np.empty((h, w, 3), dtype=np.uint8)
    img[:, :w // 2 + 5] = left
    img[:, w // 2 + 5:] = right
    img[h // 2 + 3:] = img[h // 2 + 3:, ::-1].copy()
    return img


def colour264():
    return two_colours(264, 200, (255, 0, 0), (0, 0, 255))


def corners72():
    """72x40: 2x2 cells, each one of the 8 corners of the sRGB cube (bit 2 of the
    index red, bit 1 green, bit 0 blue)"""
    idx = np.random.default_rng(26).integers(0, 8, (20, 36))
    idx = np.repeat(np.repeat(idx, 2, axis=0), 2, axis=1)
    return (np.stack([idx >> 2 & 1, idx >> 1 & 1, idx & 1], -1) * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def images():
    out = {
        "white72": white72(),
        "edge72": half(72, 40),
        "half264": half(264, 200),
        "tri64": tri64(),
        "colour264": colour264(),
        "corners72": corners72(),
    }
    for v in out.values():
        v.setflags(write=False)
    return out


# (image, distance, setting): the table of the cases
CASES = (
    ("half264", 0.001, CJXL7),
    ("half264", 0.001, PLAIN5),
    ("half264", 0.004, PLAIN5),
    ("half264", 0.0111, CJXL8),
    ("half264", 0.0108, PLAIN5),
    ("edge72", 0.004, CJXL7),
    ("white72", 0.001, CJXL7),
    ("white72", 0.001, PLAIN7),
    ("tri64", 0.001, PLAIN7),
    ("tri64", 0.001, CJXL8),
    ("colour264", 0.001, CJXL7),
    ("corners72", 0.001, CJXL7),
    ("corners72", 0.001, PLAIN5),
)
# and every image at the floor, under every setting
FLOOR_CASES = tuple((name, FLOOR, s) for s in SETTINGS for name in
                    ("white72", "edge72", "half264", "tri64", "colour264", "corners72"))
ALL_CASES = CASES + FLOOR_CASES


def case_id(c):
    return "%s-d%g-%s" % (c[0], c[1], setting_id(c[2]))


@functools.lru_cache(maxsize=None)
def oracle_ref(name, distance, setting):
    """the oracle's encode of a case, once per process (read-only by agreement)"""
    import oracle_ffi

    oracle_ffi.build()
    e, p, coder, mask = setting
    return oracle_ffi.encode(images()[name], distance, e, p, coder, mask)


@functools.lru_cache(maxsize=None)
def decoded(name, distance, setting):
    """the Python decoder's reading of the oracle's bytes (maps only)"""
    import jxl_decode

    return jxl_decode.decode(oracle_ref(name, distance, setting).bytes, want_pixels=False)


@functools.lru_cache(maxsize=None)
def reference_rgb(name, distance, setting):
    """the Python decoder's float64 image of the oracle's bytes (read-only)"""
    import jxl_decode

    rgb = jxl_decode.reconstruct(decoded(name, distance, setting))
    rgb.setflags(write=False)
    return rgb


# the pixel comparisons (GPU reconstruction / decoder against the Python
# decoder): plain and cjxl presets, G clamped and at its ceiling
RECON_CASES = tuple((name, d, s) for name in ("half264", "white72", "tri64")
                    for d in (0.001, 0.0108) for s in (PLAIN5, CJXL7))
RECON_MAX_SHARE = 0.005  # test_gpu_recon.py's bound: no sample off by more than 1, <= 0.5 % differ


def jxg_flags(jxg_mod, setting, keep_maps=False):
    _, _, coder, mask = setting
    f = jxg_mod.FLAG_KEEP_MAPS if keep_maps else 0
    if coder:
        f |= jxg_mod.FLAG_ANS
    if mask & 1:
        f |= jxg_mod.FLAG_GABORISH
    if mask & 2:
        f |= jxg_mod.FLAG_EPF
    if mask & 4:
        f |= jxg_mod.FLAG_AQ_MASKING
    return f


def class_masks(acs):
    """(8x8-class, merged) boolean maps of the blocks of a strategy map (cover
    flags 0x80 dropped)"""
    c8 = np.isin(acs & 0x7F, CLASS8)
    return c8, ~c8


def reach(ref):
    """what an oracle result reaches: max |q| per class and channel (X, Y, B),
    counts at +-32767 and >= 16384 per class, stored qf range, G"""
    a = np.abs(ref.ac.astype(np.int64))  # (bys, bxs, 3, 64)
    c8, mg = class_masks(ref.acs)
    out = {"qf": (int(ref.qf.min()), int(ref.qf.max())), "G": int(ref.global_scale),
           "qdc": int(ref.quant_dc)}
    for key, m in (("c8", c8), ("merged", mg)):
        sel = a[m]  # (n, 3, 64)
        out[key] = {
            "max": [int(sel[:, c].max()) if sel.size else 0 for c in range(3)],
            "sat": int((sel == 32767).sum()),
            "big": int((sel >= 16384).sum()),
        }
    return out


def token_of(q):
    """(tok, nbits, extra bits, the two mantissa bits in the token) of the
    hybrid-integer token of signed coefficients q (csrc/jxg_device.h
    pack_signed / hybrid420, restated): the packed value v is 2 q for q >= 0
    and -2 q - 1 for q < 0; v < 16 is its own token; otherwise n = floor(log2
    v), m = v - 2^n, tok = 16 + ((n - 4) << 2) + (m >> (n - 2)), nbits = n - 2,
    bits = the low nbits of v"""
    q = np.asarray(q, dtype=np.int64)
    v = np.where(q >= 0, 2 * q, -2 * q - 1)
    n = np.zeros_like(v)
    for b in range(1, 32):
        n = np.where(v >> b != 0, b, n)
    m = v - (np.int64(1) << n)
    small = v < 16
    sh = np.maximum(n - 2, 0)
    top2 = np.where(small, 0, m >> sh)
    tok = np.where(small, v, 16 + ((n - 4) << 2) + top2)
    nbits = np.where(small, 0, n - 2)
    bits = np.where(small, 0, v & ((np.int64(1) << sh) - 1))
    return tok, nbits, bits, top2
