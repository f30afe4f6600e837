"""Index ranges of the merge stage's LDS image (ADVICE r3 medium / VERDICT r3
item 8): round 3's outlined merge_write build faulted; one hypothesis was an
out-of-range S.co / S.qsum / S.llf index that the DS instructions tolerate and
a generic (flat) access does not.  This restates the index math of
csrc/jxg_merge_kernel.h (Pass, col_pass, quant_pass) and
csrc/jxg_merge_write.hip (row_pass, write_pass) in Python and enumerates every thread, item and loop index of every shape, with
every varblock valid (the largest index set), checking each LDS index against
its array.  CPU only: the kernels' own arithmetic is the same integer math."""
import itertools

import pytest

KMS = 65
KPLANE = 64 * KMS
CO = 2 * KPLANE          # MergeLds::co
THREADS = 256
SHAPES = [(1, 0), (0, 1), (1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 3), (3, 3)]  # (lcy, lcx)


class Pass:
    def __init__(self, lcy, lcx):
        self.lcy, self.lcx = lcy, lcx
        self.R, self.C = 8 << lcy, 8 << lcx
        self.lR, self.lC = 3 + lcy, 3 + lcx
        self.lGX = 3 - lcx
        self.lNV = 6 - lcx - lcy
        self.NV = 1 << self.lNV

    def bx0(self, v):
        return (v & ((1 << self.lGX) - 1)) << self.lcx

    def by0(self, v):
        return (v >> self.lGX) << self.lcy

    def off(self, v, plane):
        return plane * KPLANE + self.by0(v) * 8 * KMS + self.bx0(v) * 8


def pass_plane(p, lc):
    return 1 if p else lc


def row_pass_indices(P, nch, p):
    """every S.co index row_pass<C, NCH> writes"""
    out = []
    C, R = P.C, P.R
    lvr = P.lNV + P.lR
    if C == 64:
        npairs = nch * P.NV * R // 2
        n = ((npairs + 63) >> 6) << 7
        for tid in range(THREADS):
            for i in range(tid, n, THREADS):
                h = (i >> 6) & 1
                pp = ((i >> 7) << 6) | (i & 63)
                r = pp * 2
                if pp >= npairs:
                    continue
                c, v, y = r >> lvr, (r >> P.lR) & (P.NV - 1), r & (R - 1)
                assert v < 32
                off = P.off(v, pass_plane(p, c)) + y * KMS
                for k in range(32):
                    out += [off + 2 * k + h, off + KMS + 2 * k + h]
    else:
        per = (nch * 4096 // C + THREADS - 1) // THREADS
        nrows = nch * P.NV * R
        lgx = P.lGX
        for tid in range(THREADS):
            for k in range(per):
                rr = tid + k * THREADS
                if rr >= nrows:
                    continue
                c = rr >> lvr
                i = rr & ((1 << lvr) - 1)
                y = (i >> lgx) & (R - 1)
                v = ((i >> (lgx + P.lR)) << lgx) | (i & ((1 << lgx) - 1))
                assert v < P.NV
                off = P.off(v, pass_plane(p, c)) + y * KMS
                out += [off + q for q in range(C)]
    return out


def col_pass_indices(P, nch, p):
    out, valid = [], []
    R = P.R
    lR = R.bit_length() - 1
    nb, lnb = 64 // R, 6 - lR
    npairs = nch * nb * 32
    for pidx in range(npairs):
        X, band, c = pidx & 31, (pidx >> 5) & (nb - 1), pidx >> (5 + lnb)
        off = pass_plane(p, c) * KPLANE + band * R * KMS + X
        valid += [(band << P.lGX) | (X >> P.lC), (band << P.lGX) | ((X + 32) >> P.lC)]
        for k in range(R):
            out += [off + k * KMS, off + 32 + k * KMS]
    return out, valid


def quant_pass_indices(P, ch_id, write):
    """S.co (coefficient plane, Y plane), S.llf, S.qsum indices of quant_pass"""
    rpc = 8 if P.lcy == 0 else 16
    nit = 2 if rpc == 8 else 1
    chan_plane = 0 if ch_id == 1 else 1
    co, llf, qsum = [], [], []
    for tid in range(THREADS):
        for it in range(nit):
            j = tid + it * THREADS
            ch = j >> (P.lNV + P.lC)
            v = (j >> P.lC) & (P.NV - 1)
            x = j & (P.C - 1)
            bx0, by0 = P.bx0(v), P.by0(v)
            for kk in range(0, rpc, 2):
                ky = ch * rpc + kk
                for dk in (0, 1):
                    co.append(P.off(v, chan_plane) + x + (ky + dk) * KMS)
                    co.append(P.off(v, 0) + x + (ky + dk) * KMS)
                    if write and ch == 0 and x < (1 << P.lcx) and kk + dk < (1 << P.lcy):
                        llf.append((by0 + ky + dk) * 8 + bx0 + x)
            qsum.append((ch, v))
    return co, llf, qsum


def write_entry_llf(P):
    cb = (1 << P.lcy) * (1 << P.lcx)
    lcb = P.lcy + P.lcx
    out = []
    for i in range(P.NV * cb):
        v = i >> lcb
        bx0, by0 = P.bx0(v), P.by0(v)
        for ky, kx in itertools.product(range(1 << P.lcy), range(1 << P.lcx)):
            out.append((by0 + ky) * 8 + bx0 + kx)
    return out


@pytest.mark.parametrize("lcy,lcx", SHAPES)
def test_merge_lds_indices_in_range(lcy, lcx):
    P = Pass(lcy, lcx)
    assert P.NV <= 32
    for nch, p in ((2, 0), (1, 1)):  # pass 0: Y and X; pass 1: B
        idx = row_pass_indices(P, nch, p)
        assert min(idx) >= 0 and max(idx) < CO, ("row_pass", lcy, lcx, min(idx), max(idx))
        idx, valid = col_pass_indices(P, nch, p)
        assert min(idx) >= 0 and max(idx) < CO, ("col_pass", lcy, lcx, max(idx))
        assert max(valid) < P.NV and min(valid) >= 0
    for ch_id in (1, 0, 2):
        for write in (False, True):
            co, llf, qsum = quant_pass_indices(P, ch_id, write)
            assert min(co) >= 0 and max(co) < CO, ("quant_pass", lcy, lcx, max(co))
            assert all(0 <= b < 64 for b in llf)
            assert all(0 <= c < 4 and 0 <= v < 32 for c, v in qsum)
    assert all(0 <= b < 64 for b in write_entry_llf(P))


@pytest.mark.parametrize("lcy,lcx", SHAPES)
def test_merge_row_pass_covers_each_coefficient_once(lcy, lcx):
    """every (plane, row, column) of the shape's image is written exactly once
    per pass: no two threads race on one LDS word"""
    P = Pass(lcy, lcx)
    for nch, p in ((2, 0), (1, 1)):
        idx = row_pass_indices(P, nch, p)
        assert len(idx) == len(set(idx)) == nch * 4096
