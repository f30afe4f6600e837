"""Reference of the rate report, pure Python: what every token
of a codestream's pass groups costs, taken from the stream itself.

The oracle decoder (oracle/jxl_decode.py, untouched) decodes the codestream
while a logging subclass stands in for its EntropyStream.  For the HF stream
(its context count is a multiple of 7425) the subclass notes per read the
histogram, the token, the raw bits (reader position around the uint config's
read) and, for prefix codes, the code length (reader position around
read_symbol).  A (varblock, channel) segment starts at every read whose context
modulo 7425 is below 555 -- the non-zero-count contexts -- and the segments map,
in order, to the first blocks of each group in raster order with channels Y, X,
B: decode()'s own loop.  Costs are integers in 1 / 256 bit."""
import math

import numpy as np

import jxl_decode

UNIT = 256
NCTX = 7425
NZ_CTX = 555  # 15 block contexts x 37 non-zero buckets


def symbol_cost(f: int) -> int:
    """the Python formula of jxg_rate_symbol_cost"""
    if f <= 0 or f > 4096:
        return 0
    return int(math.floor(256.0 * math.log2(4096.0 / f) + 0.5))


class _LoggingStream(jxl_decode.EntropyStream):
    hf_prefix = None  # the HF stream's coder
    groups = None  # [(segments [[tokens, cost], ...], emitted bits)] while a decode is logged

    def __init__(self, br, nctx):
        super().__init__(br, nctx)
        self._hf = nctx >= NCTX and nctx % NCTX == 0
        self._segs = None
        if self._hf:
            _LoggingStream.hf_prefix = bool(self.prefix)

    def begin(self, br):
        if self._hf:
            self._br, self._p0, self._segs = br, br.pos, []
        super().begin(br)

    def read(self, br, ctx):
        if not self._hf:
            return super().read(br, ctx)
        h = self.ctxmap[ctx]
        p = br.pos
        tok = self.read_symbol(br, h)
        length = br.pos - p
        p = br.pos
        val = self.cfgs[h].read(tok, br)
        nbits = br.pos - p
        if self.prefix:
            cost = UNIT * (length + nbits)
        else:
            cost = symbol_cost(self.freqs[h][tok]) + UNIT * nbits
        if ctx % NCTX < NZ_CTX:
            self._segs.append([0, 0])
        self._segs[-1][0] += 1
        self._segs[-1][1] += cost
        return val

    def end(self):
        super().end()
        if self._hf:
            _LoggingStream.groups.append((self._segs, self._br.pos - self._p0))
            self._segs = None


def reference(data: bytes) -> dict:
    """tokens / cost [27, 3] uint64 (X, Y, B), block_cost (bys, bxs) uint32,
    per pass group its summed cost (1 / 256 bit), the bits the reader consumed
    in its AC stream (ANS: the 32-bit state included) and its section's bytes
    in the TOC; ans; stream_bits"""
    saved = jxl_decode.EntropyStream
    _LoggingStream.groups = []
    jxl_decode.EntropyStream = _LoggingStream
    try:
        d = jxl_decode.decode(data, want_pixels=False)
        groups, prefix = _LoggingStream.groups, _LoggingStream.hf_prefix
    finally:
        jxl_decode.EntropyStream = saved
        _LoggingStream.groups = None
    bxs, bys = d.bxs, d.bys
    gxs = (d.xsize + 255) // 256
    ng = gxs * ((d.ysize + 255) // 256)
    assert len(groups) == ng
    tokens = np.zeros((27, 3), np.uint64)
    cost = np.zeros((27, 3), np.uint64)
    bmap = np.zeros((bys, bxs), np.uint32)
    gcost = []
    for g, (segs, _) in enumerate(groups):
        bx0, by0 = (g % gxs) * 32, (g // gxs) * 32
        it = iter(segs)
        total = 0
        for by in range(by0, min(by0 + 32, bys)):
            for bx in range(bx0, min(bx0 + 32, bxs)):
                t = int(d.acs[by, bx])
                if t & 0x80:
                    continue
                for c in (1, 0, 2):
                    n, k = next(it)
                    tokens[t, c] += np.uint64(n)
                    cost[t, c] += np.uint64(k)
                    bmap[by, bx] += np.uint32(k)
                    total += k
        assert next(it, None) is None, "segments left over in group %d" % g
        gcost.append(total)
    nlf = ((d.xsize + 2047) // 2048) * ((d.ysize + 2047) // 2048)
    sizes = d.section_sizes
    gbytes = [sizes[0]] if ng == 1 else [sizes[2 + nlf + g] for g in range(ng)]
    return {"tokens": tokens, "cost": cost, "block_cost": bmap, "group_cost": gcost,
            "group_bits": [b for _, b in groups], "group_bytes": gbytes, "groups": ng,
            "ans": 0 if prefix else 1, "stream_bits": 8 * len(data)}

