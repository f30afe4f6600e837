"""What the sweep and report tests share: the six sweep points, the small
natural image and what fresh contexts give for it (computed once per kind of
report), bit-exact comparisons of quality dicts and report dicts, and a
two-point sweep through the raw ABI whose first point is refused."""
import ctypes

import numpy as np

INVALID_ARG = -1
QKEYS = ("sse", "samples", "mse", "psnr", "ssim")


def points(jxg):
    d = jxg.FLAGS_CJXL_DEFAULTS
    return [
        dict(distance=1.0, effort=5, proposals=0, flags=d),
        dict(distance=4.0, effort=5, proposals=0, flags=d & ~jxg.FLAG_ANS),   # prefix codes
        dict(distance=1.0, effort=7, proposals=3, flags=d),                   # both hooks
        dict(distance=4.0, effort=7, proposals=0, flags=d),
        dict(distance=1.0, effort=8, proposals=0, flags=d),
        dict(distance=4.0, effort=8, proposals=0, flags=d),
    ]


_cache = {}


def cached(key, make):
    """make() once per key; the tests share the result and leave it unchanged"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def natural():
    def make():
        from jxg.synth import natural_rgb8

        img = natural_rgb8(200, 136, 5)
        img.setflags(write=False)
        return img

    return cached("natural", make)


def bits(v):
    return np.float64(v).tobytes() if isinstance(v, float) else v


def qbits(q, ms=True):
    """a point's quality words, floats by their bits; with ms also ms_ssim (where
    the dict has it) and the per-scale cs list"""
    out = [bits(q[k]) for k in QKEYS]
    if ms:
        out += [bits(q["ms_ssim"])] if "ms_ssim" in q else []
        out.append(np.array(q.get("cs", []), np.float64).tobytes())
    return out


def same(keys, also=lambda a, b, k: True):
    """a comparison of two report dicts: every key's array equal, and also(a, b, key)"""
    return lambda a, b: all(np.array_equal(a[k], b[k]) and also(a, b, k) for k in keys)


class RefusedAndGood:
    """A sweep of natural() through jxg_sweep_rgb8 itself: point 0 is refused
    (effort 0), point 1 is `good`.  Calling it with a quality level returns
    (status of the call, the two codestreams or None); .st holds the points'
    statuses of the last call."""

    def __init__(self, jxg, enc, good):
        self.lib, self.ctx = jxg.load(), enc._ctx
        self.img = np.array(natural())
        self.pts = (jxg._SweepPoint * 2)(
            jxg._SweepPoint(1.0, 0, 0, 0),
            jxg._SweepPoint(good["distance"], good["effort"], good["proposals"], good["flags"]))
        self.outs = (jxg._Buffer * 2)()
        self.qs = (jxg._Quality * 2)()
        self.st = (ctypes.c_int * 2)()

    def __call__(self, quality):
        ret = self.lib.jxg_sweep_rgb8(self.ctx, self.img.ctypes.data, 200, 136, 600, self.pts, 2,
                                      quality, self.outs, self.qs if quality else None, self.st)
        datas = [ctypes.string_at(o.data, o.size) if o.data else None for o in self.outs]
        for o in self.outs:
            self.lib.jxg_buffer_free(ctypes.byref(o))
        return ret, datas


def poisoned(ctype, n):
    """n result structs filled with 0xA5: a getter has to overwrite all of them"""
    arr = (ctype * n)()
    for r in arr:
        ctypes.memset(ctypes.byref(r), 0xA5, ctypes.sizeof(r))
    return arr
