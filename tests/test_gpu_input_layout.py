"""Input layout: an image that is a window of a larger buffer -- a base
pointer that is not 4-byte aligned (a crop of a device image) and a row stride
above 3 * width -- gives exactly the result of the tight image, through every
entry point that reads or writes RGB8.

The buffer around the window holds a position-dependent poison, (37 i + 11) &
0xFF at byte i, so a read that clamps to the buffer instead of the window (the
AQ halo, the Gaborish ring, the edge replication) changes the result, and a
write outside the window shows.

The front kernel reads 12-byte chunks as three dwords when (stride | base) & 3
== 0 and clamped bytes otherwise (csrc/jxg_front_kernel.h issue_tile_loads);
sse_kernel and ms_pyramid_kernel choose per row (csrc/jxg_metrics.hip).  The
two widths are 200 (3 w = 0 mod 4) and 67 (3 w = 1 mod 4); the strides are
3 w + 1, + 4 and + 37, the tight one, and 3 w + 3, the only one of them that is
a multiple of 4 at width 67, so both paths run on both widths.  The 67-wide
frame has chunks that straddle the window's right edge.  The sharded entry
points are not covered here."""
import ctypes

import numpy as np
import pytest

import metrics
import msssim_ref

pytestmark = pytest.mark.gpu

CJXL = 7  # the oracle's filters mask of cjxl's defaults
# name -> (distance, effort, proposals, coder, oracle filters mask)
PRESETS = {"e7_cjxl_pf": (1.0, 7, 3, 1, CJXL), "e4_plain": (1.0, 4, 0, 0, 0)}
SIZES = [(200, 136), (67, 41)]
OFFSETS = (0, 1, 2, 3)
EXTRA = (0, 1, 3, 4, 37)  # row stride - 3 * width; 0 is the tight case
LAYOUTS = [(off, extra) for extra in EXTRA for off in OFFSETS]


def _flags(jxg, preset):
    _, _, _, coder, mask = PRESETS[preset]
    return (jxg.FLAG_ANS if coder else 0) | (jxg.FLAGS_CJXL_DEFAULTS & ~jxg.FLAG_ANS if mask else 0)


def _encoder(jxg, preset, extra_flags=0):
    d, e, p = PRESETS[preset][:3]
    return jxg.Encoder(distance=d, effort=e, proposals=p, flags=_flags(jxg, preset) | extra_flags)


_imgs, _refs = {}, {}


def _image(w, h, k=0):
    """the k-th frame of a size (read-only)"""
    from jxg.synth import synth_rgb8

    if (w, h, k) not in _imgs:
        img = synth_rgb8(w, h, 0x4A584C40 + 16 * k + w)
        img.setflags(write=False)
        _imgs[w, h, k] = img
    return _imgs[w, h, k]


def _ref(oracle, preset, w, h, k=0):
    """the oracle's bytes of the tight image, once"""
    if (preset, w, h, k) not in _refs:
        _refs[preset, w, h, k] = oracle.encode(_image(w, h, k), *PRESETS[preset]).bytes
    return _refs[preset, w, h, k]


class Window:
    """`img` (or, with img None, nothing) as a w x h window at byte `lead + off`
    of a poisoned buffer, rows `stride` bytes apart; the buffer's first byte is
    64-byte aligned on the host and lies at the start of an allocation on the
    device, lead is a multiple of 64, and at least two rows of poison lie on
    either side"""

    def __init__(self, w, h, off, extra, img=None):
        self.w, self.h, self.off = w, h, off
        self.stride = 3 * w + extra
        lead = 64 * ((2 * self.stride + 63) // 64)
        self.start = lead + off
        n = self.start + h * self.stride + 2 * self.stride + 64
        raw = np.empty(n + 64, np.uint8)
        a = (-raw.ctypes.data) % 64
        self.host = raw[a:a + n]
        self.host[:] = ((37 * np.arange(n, dtype=np.int64) + 11) & 0xFF).astype(np.uint8)
        self.inside = np.zeros(n, bool)
        self._rows(self.inside)[:] = True
        self.poison = self.host.copy()
        if img is not None:
            self._rows(self.host)[:] = np.asarray(img).reshape(h, 3 * w)
        self.dev = None

    def _rows(self, buf):
        return np.lib.stride_tricks.as_strided(buf[self.start:], shape=(self.h, 3 * self.w),
                                               strides=(self.stride, 1))

    @property
    def host_ptr(self):
        assert self.host.ctypes.data % 64 == 0
        return self.host.ctypes.data + self.start

    def to_device(self):
        import torch

        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 64 == 0
        return self

    @property
    def dev_ptr(self):
        return self.dev.data_ptr() + self.start

    def read_back(self):
        """(the window's pixels, whether every byte outside it is still its poison)"""
        got = self.dev.cpu().numpy() if self.dev is not None else self.host
        intact = np.array_equal(got[~self.inside], self.poison[~self.inside])
        return self._rows(got).reshape(self.h, self.w, 3).copy(), intact


def _sync():
    import torch

    torch.cuda.synchronize()


def _take(jxg, buf):
    return jxg.Encoder._take(buf)


def _where(off, extra):
    return "offset %d, stride 3w + %d" % (off, extra)


@pytest.mark.parametrize("preset", list(PRESETS))
@pytest.mark.parametrize("w,h", SIZES)
def test_encode_host_windows(jxg_mod, oracle, preset, w, h):
    """jxg_encode_rgb8 itself, as tests/test_gpu_edge.py calls it"""
    lib = jxg_mod.load()
    want, bad = _ref(oracle, preset, w, h), []
    with _encoder(jxg_mod, preset) as enc:
        for off, extra in LAYOUTS:
            win = Window(w, h, off, extra, _image(w, h))
            buf = jxg_mod._Buffer()
            st = lib.jxg_encode_rgb8(enc._ctx, ctypes.c_void_p(win.host_ptr), w, h, win.stride,
                                     ctypes.byref(buf))
            assert st == 0, _where(off, extra)
            if _take(jxg_mod, buf) != want:
                bad.append(_where(off, extra))
    assert not bad, bad


@pytest.mark.parametrize("preset", list(PRESETS))
@pytest.mark.parametrize("w,h", SIZES)
def test_encode_device_windows(jxg_mod, oracle, preset, w, h):
    want, bad = _ref(oracle, preset, w, h), []
    wins = [Window(w, h, off, extra, _image(w, h)).to_device() for off, extra in LAYOUTS]
    _sync()
    with _encoder(jxg_mod, preset) as enc:
        for win, (off, extra) in zip(wins, LAYOUTS):
            if enc.encode_device(win.dev_ptr, w, h, win.stride) != want:
                bad.append(_where(off, extra))
    assert not bad, bad
    # and a fresh context per layout: nothing the first, tight frame left helps
    for k in (5, 11, 18):
        with _encoder(jxg_mod, preset) as enc:
            assert enc.encode_device(wins[k].dev_ptr, w, h, wins[k].stride) == want, LAYOUTS[k]


@pytest.mark.parametrize("device", [False, True], ids=["submit", "submit_device"])
@pytest.mark.parametrize("w,h", SIZES)
def test_four_layouts_in_flight(jxg_mod, oracle, w, h, device):
    """four frames in flight, four offsets: small frames share one batched
    launch, which then carries four layouts"""
    preset = "e7_cjxl_pf"
    lib = jxg_mod.load()
    fn = lib.jxg_submit_rgb8_device if device else lib.jxg_submit_rgb8
    want = [_ref(oracle, preset, w, h, k) for k in range(4)]
    assert len(set(want)) == 4
    bad = []
    with _encoder(jxg_mod, preset) as enc:
        # the four offsets at one stride, then at four strides
        for extras in [(e,) * 4 for e in EXTRA] + [(0, 1, 4, 37), (37, 3, 1, 0)]:
            wins = [Window(w, h, off, extra, _image(w, h, k))
                    for k, (off, extra) in enumerate(zip(OFFSETS, extras))]
            if device:
                for win in wins:
                    win.to_device()
                _sync()
            for win in wins:
                ptr = win.dev_ptr if device else win.host_ptr
                assert fn(enc._ctx, ctypes.c_void_p(ptr), w, h, win.stride) == 0
            assert enc.pending() == 4
            got = [enc.receive() for _ in range(4)]
            bad += ["frame %d, %s" % (k, _where(OFFSETS[k], extras[k])) for k in range(4)
                    if got[k] != want[k]]
    assert not bad, bad


@pytest.mark.parametrize("device", [False, True], ids=["encode_batch", "encode_batch_device"])
@pytest.mark.parametrize("w,h", SIZES)
def test_batch_shares_a_stride_not_an_alignment(jxg_mod, oracle, w, h, device):
    preset = "e7_cjxl_pf"
    lib = jxg_mod.load()
    fn = lib.jxg_encode_batch_rgb8_device if device else lib.jxg_encode_batch_rgb8
    want = [_ref(oracle, preset, w, h, k) for k in range(4)]
    bad = []
    with _encoder(jxg_mod, preset) as enc:
        for extra in EXTRA:
            for offs in (OFFSETS, (3, 0, 1, 1)):
                wins = [Window(w, h, off, extra, _image(w, h, k)) for k, off in enumerate(offs)]
                if device:
                    for win in wins:
                        win.to_device()
                    _sync()
                ptrs = (ctypes.c_void_p * 4)(*[win.dev_ptr if device else win.host_ptr
                                               for win in wins])
                outs = (jxg_mod._Buffer * 4)()
                assert fn(enc._ctx, ptrs, 4, w, h, wins[0].stride, outs) == 0
                got = [_take(jxg_mod, outs[k]) for k in range(4)]
                bad += ["frame %d, %s" % (k, _where(offs[k], extra)) for k in range(4)
                        if got[k] != want[k]]
    assert not bad, bad


# ---------------------------------------------------------------------------
# the other device readers of RGB8: one misaligned window each, against the
# tight host variant
# ---------------------------------------------------------------------------
W, H = 67, 41          # chunks straddle the window's right edge
OFF, EXTRA1 = 3, 1     # base = 3 mod 4, stride 3 w + 1 = 202: rows at 3, 1, 3, 1 mod 4


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def _sweep_points(jxg):
    d = jxg.FLAGS_CJXL_DEFAULTS
    return [dict(distance=1.0, effort=7, proposals=3, flags=d),
            dict(distance=2.0, effort=4, proposals=0, flags=0),
            dict(distance=3.0, effort=8, proposals=0, flags=d)]


def test_sweep_forced_traced_device(jxg_mod, oracle):
    jxg = jxg_mod
    img = _image(W, H)
    win = Window(W, H, OFF, EXTRA1, img).to_device()
    _sync()
    pts = _sweep_points(jxg)
    with _encoder(jxg, "e7_cjxl_pf", jxg.FLAG_KEEP_MAPS) as enc:
        # sweep: bytes, quality and riders of the tight host sweep
        kw = dict(quality="ssim", strategies=True, rates=True, trace=True)
        want = enc.sweep(img, pts, **kw)
        got = enc.sweep_device(win.dev_ptr, W, H, pts, row_stride=win.stride, **kw)
        assert _same(got, want)
        for (data, _), p in zip(want, pts):
            coder = 1 if p["flags"] & jxg.FLAG_ANS else 0
            assert data == oracle.encode(img, p["distance"], p["effort"], p["proposals"], coder,
                                         CJXL if p["flags"] else 0).bytes
        # traced
        ref = _ref(oracle, "e7_cjxl_pf", W, H)
        assert enc.encode_traced(img) == ref
        want = (enc.search_trace(), enc.stats()["acs"], enc.reconstruct())
        assert enc.encode_traced_device(win.dev_ptr, W, H, win.stride) == ref
        assert _same((enc.search_trace(), enc.stats()["acs"], enc.reconstruct()), want)
        # forced, with the search's own map (hooks play no part in a forced encode)
        acs = want[1]
        want = (enc.encode_forced(img, acs), enc.reconstruct())
        got = (enc.encode_forced_device(win.dev_ptr, W, H, acs, row_stride=win.stride),
               enc.reconstruct())
        assert _same(got, want)


def test_strategy_and_ab_report_device(jxg_mod, oracle):
    jxg = jxg_mod
    img = _image(W, H)
    win = Window(W, H, OFF, EXTRA1, img).to_device()
    _sync()
    with _encoder(jxg, "e7_cjxl_pf") as a, jxg.Encoder(
            distance=2.0, effort=5, flags=jxg.FLAGS_CJXL_DEFAULTS) as b:
        assert a.encode(img) == _ref(oracle, "e7_cjxl_pf", W, H)
        b.encode_device(win.dev_ptr, W, H, win.stride)
        want = a.strategy_report(img)
        assert int(want["sse"].sum()) > 0
        assert _same(a.strategy_report_device(win.dev_ptr, win.stride), want)
        want = jxg.ab_report(a, b, img)
        assert int(want["sse_a"].sum()) > 0 and int(want["sse_b"].sum()) > 0
        assert _same(jxg.ab_report_device(a, b, win.dev_ptr, win.stride), want)
    _, intact = win.read_back()
    assert intact


def test_compare_and_msssim_device(jxg_mod):
    """orig and comp at different alignments and strides, against
    oracle/metrics.py and tests/msssim_ref.py at the tolerances of
    test_gpu_metrics.py and test_gpu_msssim.py"""
    from test_gpu_metrics import _pair

    a, b = _pair(177, 191, 177 * 1000 + 191)  # 3 w = 1 mod 4; min side >= 176
    h, w = a.shape[:2]
    ref = msssim_ref.msssim(a, b)
    assert min(ref["cs"] + ref["ssim"]) > 0.88
    with jxg_mod.Encoder(distance=1.0, effort=7) as enc:
        for (oa, ea), (ob, eb) in (((1, 37), (2, 1)), ((3, 0), (0, 4)), ((0, 4), (3, 1))):
            wa = Window(w, h, oa, ea, a).to_device()
            wb = Window(w, h, ob, eb, b).to_device()
            _sync()
            q = enc.compare_device(wa.dev_ptr, wb.dev_ptr, w, h, wa.stride, wb.stride)
            assert q["sse"] == metrics.sse(a, b) and q["samples"] == a.size
            assert q["mse"] == metrics.mse(a, b)
            assert q["psnr"] == metrics.psnr(metrics.mse(a, b))
            assert q["ssim"] == pytest.approx(metrics.ssim(a, b), rel=1e-12, abs=1e-15)
            got = enc.msssim_device(wa.dev_ptr, wb.dev_ptr, w, h, wa.stride, wb.stride)
            for j in range(5):
                assert got["cs"][j] == pytest.approx(ref["cs"][j], rel=1e-12, abs=1e-15), j
                assert got["ssim"][j] == pytest.approx(ref["ssim"][j], rel=1e-12, abs=1e-15), j
            assert got["ms_ssim"] == pytest.approx(ref["ms_ssim"], rel=1e-11)
            # bit-equal to the tight host variants: same kernels, same order
            assert _same(q, enc.compare(a, b)) and _same(got, enc.msssim(a, b))


# ---------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("off,extra", [(1, 1), (3, 37), (2, 0), (0, 4)])
@pytest.mark.parametrize("w,h", SIZES)
def test_writers_keep_to_the_window(jxg_mod, oracle, w, h, off, extra):
    img = _image(w, h)
    with _encoder(jxg_mod, "e7_cjxl_pf") as enc:
        data = enc.encode(img)
        assert data == _ref(oracle, "e7_cjxl_pf", w, h)
        want = enc.reconstruct()
        win = Window(w, h, off, extra).to_device()
        _sync()
        enc.reconstruct_device(win.dev_ptr, win.stride)
        got, intact = win.read_back()
        assert np.array_equal(got, want), "reconstruct_device"
        assert intact, "reconstruct_device wrote outside the window"
        want = enc.decode(data)
        win = Window(w, h, off, extra).to_device()
        _sync()
        enc.decode_device(data, win.dev_ptr, win.stride)
        got, intact = win.read_back()
        assert np.array_equal(got, want), "decode_device"
        assert intact, "decode_device wrote outside the window"
        # several frames, several layouts, one call
        wins = [Window(w, h, o, e).to_device() for o, e in ((off, extra), (3 - off, 37 - extra))]
        _sync()
        assert enc.decode_batch_device([data, data], [x.dev_ptr for x in wins],
                                       [x.stride for x in wins]) == [0, 0]
        for x in wins:
            got, intact = x.read_back()
            assert np.array_equal(got, want), "decode_batch_device"
            assert intact, "decode_batch_device wrote outside the window"
