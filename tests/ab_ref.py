"""Reference of the A/B report, numpy: the strategy
transitions of two encodes of one image with the bits and the error of both
sides.  Inputs per side: the strategy bytes (bit 7: a covered non-first block),
the block error map, the first-block cost map (a varblock's cost at its first
block, 0 elsewhere).  Every value is an integer."""
import numpy as np

N = 27
# (down, across) in 8x8 blocks per raw AcStrategy id, written out by hand: the
# names are rows x columns in pixels (DCT32X16: 32 rows, 16 columns)
DIMS = {
    0: (1, 1),    # DCT8
    1: (1, 1),    # IDENTITY
    2: (1, 1),    # DCT2X2
    3: (1, 1),    # DCT4X4
    4: (2, 2),    # DCT16X16
    5: (4, 4),    # DCT32X32
    6: (2, 1),    # DCT16X8
    7: (1, 2),    # DCT8X16
    8: (4, 1),    # DCT32X8
    9: (1, 4),    # DCT8X32
    10: (4, 2),   # DCT32X16
    11: (2, 4),   # DCT16X32
    12: (1, 1),   # DCT4X8
    13: (1, 1),   # DCT8X4
    14: (1, 1),   # AFV0
    15: (1, 1),   # AFV1
    16: (1, 1),   # AFV2
    17: (1, 1),   # AFV3
    18: (8, 8),   # DCT64X64
    19: (8, 4),   # DCT64X32
    20: (4, 8),   # DCT32X64
    21: (16, 16),  # DCT128X128
    22: (16, 8),   # DCT128X64
    23: (8, 16),   # DCT64X128
    24: (32, 32),  # DCT256X256
    25: (32, 16),  # DCT256X128
    26: (16, 32),  # DCT128X256
}


def first_blocks(acs):
    """[(by, bx, id, down, across)] of the varblocks, raster order of first blocks"""
    acs = np.asarray(acs)
    out = []
    for by, bx in np.argwhere((acs & 0x80) == 0):
        t = int(acs[by, bx]) & 0x7F
        out.append((int(by), int(bx), t) + DIMS[t])
    return out


def shares(acs, cost):
    """the cost share of every block: a varblock of cost C over n blocks gives
    block k (raster order inside the varblock) C // n + (k < C % n)"""
    acs = np.asarray(acs)
    cost = np.asarray(cost)
    out = np.zeros(acs.shape, np.uint32)
    seen = np.zeros(acs.shape, np.int32)
    for by, bx, t, down, across in first_blocks(acs):
        c = int(cost[by, bx])
        n = down * across
        for k in range(n):
            y, x = by + k // across, bx + k % across
            out[y, x] = c // n + (1 if k < c % n else 0)
            seen[y, x] += 1
    assert (seen == 1).all(), "the varblocks do not tile the frame"
    return out


def pixels(bys, bxs, w, h):
    """image pixels of every block, cropped to w x h"""
    py = np.minimum(8, h - 8 * np.arange(bys))
    px = np.minimum(8, w - 8 * np.arange(bxs))
    return np.outer(py, px).astype(np.uint64)


def reference(acs_a, acs_b, sse_a, sse_b, cost_a, cost_b, w, h):
    """blocks, pixels, sse_a, sse_b, cost_a, cost_b: [27, 27] uint64 indexed
    [from, to]; block_delta (2, bys, bxs) int32; share_a / share_b"""
    acs_a, acs_b = np.asarray(acs_a), np.asarray(acs_b)
    bys, bxs = acs_a.shape
    assert acs_b.shape == (bys, bxs) == ((h + 7) // 8, (w + 7) // 8)
    sh_a, sh_b = shares(acs_a, cost_a), shares(acs_b, cost_b)
    px = pixels(bys, bxs, w, h)
    vals = {"blocks": np.ones((bys, bxs), np.uint64), "pixels": px,
            "sse_a": np.asarray(sse_a).astype(np.uint64), "sse_b": np.asarray(sse_b).astype(np.uint64),
            "cost_a": sh_a.astype(np.uint64), "cost_b": sh_b.astype(np.uint64)}
    out = {k: np.zeros((N, N), np.uint64) for k in vals}
    fr, to = acs_a & 0x7F, acs_b & 0x7F
    for by in range(bys):
        for bx in range(bxs):
            f, t = int(fr[by, bx]), int(to[by, bx])
            for k, v in vals.items():
                out[k][f, t] += v[by, bx]
    out["block_delta"] = np.stack([
        np.asarray(sse_b).astype(np.int64) - np.asarray(sse_a).astype(np.int64),
        sh_b.astype(np.int64) - sh_a.astype(np.int64)]).astype(np.int32)
    out["share_a"], out["share_b"] = sh_a, sh_b
    return out
