"""Frame sequences and presets for one context kept across frames (helper of
test_reuse_cases.py and test_gpu_context_reuse.py; not a conftest).

The drop-in boundary keeps one context per (distance, effort) and pushes every
image of a corpus through it, so everything a context carries from frame to
frame (csrc/jxg_ctx.h: buffers that only grow, the plan upload key, the cached
context map, the statistics arena, the LF look-back words, the ready flags)
meets a frame of another size and another kind of content.  MAIN is the
sequence for that: it shrinks and grows across every structural boundary and
its neighbours differ in content class, so that a list, count, flag or
histogram left over from the frame before changes bytes.  E8 is the effort-8
sequence, whose frames each need another set of explicit quant tables in
HfGlobal.  What the sequences reach is asserted from the oracle alone in
test_reuse_cases.py, so a changed frame fails there instead of going soft.
"""
import functools

import numpy as np

from test_gpu_parity import smooth_rgb8
from test_recon_cases import gradient_rgb8

ANS, PREFIX = 1, 0
CJXL = 7  # the oracle's filters mask of cjxl's defaults (Gaborish 1 | EPF 2 | masking AQ 4)

# name -> (distance, effort, proposals, coder, oracle filters mask, KEEP_MAPS, sequence)
PRESETS = {
    "e7_cjxl_pf": (1.0, 7, 3, ANS, CJXL, False, "main"),
    "e5_prefix": (1.0, 5, 0, PREFIX, 0, False, "main"),
    "e8_cjxl": (1.0, 8, 0, ANS, CJXL, False, "e8"),
    "e3_plain": (1.0, 3, 0, PREFIX, 0, False, "main"),
    "e7_ans_keep": (1.0, 7, 0, ANS, 0, True, "main"),
}
# the presets with a search (effort >= 5) that run MAIN: its properties hold for these
SEARCHING = ("e7_cjxl_pf", "e5_prefix", "e7_ans_keep")

CLASS8 = (0, 1, 2, 3, 12, 13)
MERGED = (6, 7, 4, 10, 11, 5, 19, 20, 18)  # 16x8 ... 64x64, the nine merged shapes
BIG = (21, 22, 23, 24, 25, 26)             # 128 / 256 px, effort 8


def noise_rgb8(w, h, seed):
    """white noise: no varblock merges at any effort"""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def flat_rgb8(w, h, colour):
    """one colour: every AC coefficient quantizes to zero"""
    return np.full((h, w, 3), colour, dtype=np.uint8)


def _synth(w, h, seed):
    from jxg.synth import synth_rgb8

    return synth_rgb8(w, h, seed)


def _natural(w, h, seed):
    from jxg.synth import natural_rgb8

    return natural_rgb8(w, h, seed)


# (content class, generator, width, height, seed or colour).  The last frame is
# the first again.
MAIN = (
    ("smooth", smooth_rgb8, 777, 555, 777 * 31 + 555),  # 70 x 98 blocks: two LF chunks of 4096
    ("noise", noise_rgb8, 64, 64, 1),                   # one 64 px tile
    ("flat", flat_rgb8, 257, 65, (90, 140, 200)),       # one past a pass group and a tile
    ("smooth", smooth_rgb8, 2100, 72, 2100 * 31 + 72),  # two LF groups
    ("noise", noise_rgb8, 9, 7, 2),                     # one partial tile
    ("flat", flat_rgb8, 1, 1, (255, 255, 255)),
    ("natural", _natural, 333, 250, 8),
    ("synth", _synth, 777, 555, 0x4A584C21),            # the first frame's plan key, other content
    ("flat", flat_rgb8, 64, 64, (0, 0, 0)),
    ("smooth", smooth_rgb8, 777, 555, 777 * 31 + 555),
)

# effort 8 at d1, ANS, filters mask 7: the streams carry qm_params kinds
# {6, 7}, {}, {7}, {6} in this order
E8 = (
    ("gradient", gradient_rgb8, 520, 300, 520 * 7 + 300),
    ("synth", _synth, 300, 200, 0x4A584C22),
    ("gradient", gradient_rgb8, 512, 256, 512 * 7 + 256),
    ("gradient", gradient_rgb8, 264, 264, 264 * 7 + 264),
)
E8_QM_KINDS = ((6, 7), (), (7,), (6,))

SEQUENCES = {"main": MAIN, "e8": E8}


@functools.lru_cache(maxsize=None)
def frames(seq):
    """the frames of a sequence, (H, W, 3) uint8, read-only"""
    out = []
    for _, gen, w, h, arg in SEQUENCES[seq]:
        img = gen(w, h, arg)
        assert img.shape == (h, w, 3) and img.dtype == np.uint8
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


def preset_frames(preset):
    return frames(PRESETS[preset][6])


@functools.lru_cache(maxsize=None)
def oracle_refs(preset):
    """the oracle's encode of every frame of the preset's sequence, once per
    process (read-only by agreement)"""
    import oracle_ffi

    oracle_ffi.build()
    d, e, p, coder, mask = PRESETS[preset][:5]
    return tuple(oracle_ffi.encode(f, d, e, p, coder, mask) for f in preset_frames(preset))


def jxg_flags(jxg_mod, preset):
    _, _, _, coder, mask, keep, _ = PRESETS[preset]
    f = jxg_mod.FLAG_KEEP_MAPS if keep else 0
    if coder:
        f |= jxg_mod.FLAG_ANS
    if mask & 1:
        f |= jxg_mod.FLAG_GABORISH
    if mask & 2:
        f |= jxg_mod.FLAG_EPF
    if mask & 4:
        f |= jxg_mod.FLAG_AQ_MASKING
    return f


def encoder(jxg_mod, preset):
    d, e, p = PRESETS[preset][:3]
    return jxg_mod.Encoder(distance=d, effort=e, proposals=p, flags=jxg_flags(jxg_mod, preset))


def first_ids(acs):
    """the strategy ids at the varblocks' first blocks"""
    return set(int(t) for t in np.unique(acs[(acs & 0x80) == 0]))


def hf_global(data):
    """the bytes of a codestream's HfGlobal section (dequant matrices, context
    map, histograms), or None for a one-group frame, which has one section"""
    import jxl_decode

    d = jxl_decode.decode(data, toc_only=True)
    if len(d.section_sizes) == 1:
        return None
    nlf = ((d.xsize + 2047) // 2048) * ((d.ysize + 2047) // 2048)
    o = d.section_offsets[1 + nlf]
    return data[o:o + d.section_sizes[1 + nlf]]
