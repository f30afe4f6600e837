"""numpy reference of the strategy report (jxg_strategy_report_rgb8, DESIGN.md
3.16): every field is an integer sum over the maps the project already
exposes, so the GPU's table must equal this one exactly."""
import numpy as np

NUM_STRATEGIES = 27
FIELDS = ("varblocks", "blocks", "pixels", "nonzeros", "qf_sum", "sse")


def reference_block_sse(orig, decoded):
    """(bys, bxs) uint64: squared RGB8 sample differences per 8x8 block, image
    pixels only (edge blocks are cropped: the padding adds nothing)"""
    o = np.asarray(orig, dtype=np.int64)
    d = np.asarray(decoded, dtype=np.int64)
    assert o.shape == d.shape and o.ndim == 3 and o.shape[2] == 3
    h, w = o.shape[:2]
    bys, bxs = (h + 7) // 8, (w + 7) // 8
    e = np.zeros((bys * 8, bxs * 8), np.int64)
    e[:h, :w] = ((o - d) ** 2).sum(axis=2)
    return e.reshape(bys, 8, bxs, 8).sum(axis=(1, 3)).astype(np.uint64)


def reference_report(acs, qf, ac, orig, decoded, w, h):
    """acs (bys, bxs) raw strategy bytes (bit 7: covered non-first block), qf
    (bys, bxs) stored quant field (raw - 1), ac (bys, bxs, 3, 64) -> dict of
    uint64 arrays [27] (nonzeros [27, 3]) like Encoder.strategy_report"""
    acs = np.asarray(acs)
    bys, bxs = (h + 7) // 8, (w + 7) // 8
    assert acs.shape == (bys, bxs) and np.asarray(ac).shape == (bys, bxs, 3, 64)
    ids = acs & 0x7F
    first = (acs & 0x80) == 0
    yy, xx = np.mgrid[0:bys, 0:bxs]
    px = np.minimum(8, w - xx * 8) * np.minimum(8, h - yy * 8)
    bsse = reference_block_sse(orig, decoded)
    nz = (np.asarray(ac) != 0).sum(axis=3)  # (bys, bxs, 3)
    out = {k: np.zeros(NUM_STRATEGIES, np.uint64) for k in FIELDS if k != "nonzeros"}
    out["nonzeros"] = np.zeros((NUM_STRATEGIES, 3), np.uint64)
    for t in range(NUM_STRATEGIES):
        m = ids == t
        out["varblocks"][t] = int((m & first).sum())
        out["blocks"][t] = int(m.sum())
        out["pixels"][t] = int(px[m].sum())
        out["nonzeros"][t] = nz[m].sum(axis=0)
        out["qf_sum"][t] = int((np.asarray(qf)[m].astype(np.int64) + 1).sum())
        out["sse"][t] = int(bsse[m].sum())
    assert int(ids.max()) < NUM_STRATEGIES
    return out
