"""Search-trace summaries in a sweep (jxg_set_sweep_trace / jxg_sweep_trace,
DESIGN.md 3.20): every point of effort >= 5 runs as a traced job on its lane.

1. codestreams, quality words and summaries equal the one-at-a-time calls, over
   lanes that serve traced and untraced points in turn;
2. the summaries are not vacuous (hook F's flips, hook P's overrides);
3. the 128 / 256 px levels on a lane, and lanes whose buffers outlive a frame;
4. every rider at once;
5. the context afterwards;
6. refusals through the raw ABI;
7. the device variant.

Equality is exact everywhere: the summary is integer sums over the same planes
the same kernels write, whichever stream runs them.
"""
import ctypes

import numpy as np
import pytest

import sweep_cases
from sweep_cases import INVALID_ARG, QKEYS, cached, poisoned, qbits
from test_gpu_trace import flat_edges, gradient, natural, u32

pytestmark = pytest.mark.gpu

SUMMARY_KEYS = ("flip", "hook_p", "merged_over", "margin", "margin_skipped")


def _eight(jxg):
    """the six shared points, one without a search, one with hook F alone and
    no flags: at 3 lanes every lane serves two points or more, and lane 0 a
    traced one, a traced one, then the untraced one"""
    d = jxg.FLAGS_CJXL_DEFAULTS
    return sweep_cases.points(jxg) + [
        dict(distance=1.0, effort=4, proposals=0, flags=d),
        dict(distance=1.0, effort=7, proposals=2, flags=0),
    ]


def _key(p):
    return (p["distance"], p["effort"], p["proposals"], p["flags"])


def _one(jxg, img_key, img, p):
    """(plain bytes, summary or None) of point p on fresh contexts"""
    def make():
        with jxg.Encoder(**p) as enc:
            data = enc.encode(img)
        if p["effort"] < 5:
            return data, None
        with jxg.Encoder(**p) as enc:
            assert enc.encode_traced(img) == data
            return data, enc.search_trace(maps=False)

    return cached(("sweep_trace_one", img_key) + _key(p), make)


def _same_summary(a, b):
    """field by field, the arrays as u32"""
    assert set(a) == set(b) == {"blocks", "max_px"} | set(SUMMARY_KEYS)
    if a["blocks"] != b["blocks"] or a["max_px"] != b["max_px"]:
        return False
    for k in SUMMARY_KEYS:
        assert a[k].dtype == b[k].dtype == np.uint32 and a[k].shape == b[k].shape, k
        if not np.array_equal(a[k], b[k]):
            return False
    return True


def _is_zero(s):
    return s["blocks"] == 0 and s["max_px"] == 0 and not any(s[k].any() for k in SUMMARY_KEYS)


def _check_points(jxg, got, img_key, img, pts, what=""):
    for i, (p, (data, q)) in enumerate(zip(pts, got)):
        ref_data, ref_sum = _one(jxg, img_key, img, p)
        assert data == ref_data, "%s point %d: bytes differ from a fresh encode" % (what, i)
        if ref_sum is None:
            assert _is_zero(q["trace"]), "%s point %d: effort < 5 is zero-filled" % (what, i)
        else:
            assert q["trace"]["blocks"] == ((img.shape[1] + 7) // 8) * ((img.shape[0] + 7) // 8)
            assert _same_summary(q["trace"], ref_sum), "%s point %d: summary" % (what, i)


# ---------------------------------------------------------------------------
# 1. equality with the one-at-a-time calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("quality", [None, "ssim"])
def test_sweep_equals_one_at_a_time(jxg_mod, quality):
    jxg = jxg_mod
    img = sweep_cases.natural()
    pts = _eight(jxg)
    with jxg.Encoder() as enc:
        enc.set_pipeline_lanes(3)
        on = enc.sweep(img, pts, quality=quality, trace=True)
        assert enc.sweep_timings()["lanes"] == 3
        off = enc.sweep(img, pts, quality=quality)
        again = enc.sweep(img, pts, quality=quality, trace=True)  # every lane: untraced, then traced
    _check_points(jxg, on, "natural", img, pts, "first")
    _check_points(jxg, again, "natural", img, pts, "again")
    for i, ((data, q), (odata, oq)) in enumerate(zip(on, off)):
        assert data == odata, "point %d: bytes with the switch off" % i
        if quality is None:
            assert set(q) == {"trace"} and oq is None
        else:
            assert set(q) == set(QKEYS) | {"trace"} and set(oq) == set(QKEYS)
            assert qbits(q) == qbits(oq), "point %d: quality words" % i
    assert [p["effort"] for p in pts].count(4) == 1
    assert sum(_is_zero(q["trace"]) for _, q in on) == 1
    assert {q["trace"]["max_px"] for _, q in on} == {0, 32, 64, 256}


# ---------------------------------------------------------------------------
# 2. not vacuous
# ---------------------------------------------------------------------------
def test_flips_and_overrides_are_counted(jxg_mod):
    jxg = jxg_mod
    img = flat_edges()
    d = jxg.FLAGS_CJXL_DEFAULTS
    pts = [dict(distance=2.0, effort=5, proposals=0, flags=d),
           dict(distance=1.0, effort=7, proposals=3, flags=d),
           dict(distance=1.0, effort=6, proposals=1, flags=d)]
    with jxg.Encoder() as enc:
        got = enc.sweep(img, pts, quality=None, trace=True)
    _check_points(jxg, got, "flat_edges", img, pts)
    s = got[1][1]["trace"]
    flip = s["flip"].astype(np.int64)
    assert flip.sum() == s["blocks"] == 25 * 17
    assert flip.sum() - np.trace(flip) == 30
    assert s["hook_p"].sum() == 49
    assert s["margin_skipped"].sum() > 0
    # without hook F the matrix is diagonal; without hook P nothing is overridden
    f0 = got[0][1]["trace"]["flip"].astype(np.int64)
    assert f0.sum() == np.trace(f0) and not got[0][1]["trace"]["hook_p"].any()
    assert got[2][1]["trace"]["hook_p"].any()


# ---------------------------------------------------------------------------
# 3. the 128 / 256 px levels on a lane; buffers larger than the frame
# ---------------------------------------------------------------------------
def test_big_levels_and_reused_buffers(jxg_mod):
    jxg = jxg_mod
    d = jxg.FLAGS_CJXL_DEFAULTS
    sq, tall = gradient(512, 512), gradient(520, 776)
    assert tall.shape[:2] == (776, 520)
    pts_sq = [dict(distance=1.0, effort=8, proposals=0, flags=d),
              dict(distance=1.0, effort=8, proposals=2, flags=d)]
    pts_tall = [dict(distance=3.0, effort=8, proposals=3, flags=d)]
    small = natural(136, 72)
    nat = sweep_cases.natural()
    pts = sweep_cases.points(jxg)
    with jxg.Encoder() as enc:
        enc.set_pipeline_lanes(2)
        for key, img, p in (("grad512", sq, pts_sq), ("grad520x776", tall, pts_tall)):
            got = enc.sweep(img, p, quality=None, trace=True)
            _check_points(jxg, got, key, img, p, key)
            assert all(q["trace"]["max_px"] == 256 for _, q in got)
        # the lanes' trace buffers now hold 65 x 97 blocks: smaller frames in them
        got = enc.sweep(small, pts, quality=None, trace=True)
        _check_points(jxg, got, "natural136x72", small, pts, "136 x 72")
        got = enc.sweep(nat, pts, quality=None, trace=True)
        _check_points(jxg, got, "natural", nat, pts, "200 x 136")


# ---------------------------------------------------------------------------
# 4. all riders together
# ---------------------------------------------------------------------------
def test_every_rider_with_the_trace(jxg_mod):
    jxg = jxg_mod
    img = sweep_cases.natural()
    pts = sweep_cases.points(jxg)[1:4]
    base = [-1, 0, 0]
    report_keys = ("strategies", "rates", "ab")
    with jxg.Encoder() as enc:
        full = enc.sweep(img, pts, quality="msssim", strategies=True, rates=True, ab=base,
                         trace=True)
        alone = {
            "msssim": enc.sweep(img, pts, quality="msssim"),
            "strategies": enc.sweep(img, pts, quality="ssim", strategies=True),
            "rates": enc.sweep(img, pts, quality="ssim", rates=True),
            "ab": enc.sweep(img, pts, quality="ssim", ab=base),
            "trace": enc.sweep(img, pts, quality="ssim", trace=True),
        }
    for i, (data, q) in enumerate(full):
        assert set(q) == set(QKEYS) | {"ms_ssim", "cs", "strategies", "rates", "trace"} | (
            {"ab"} if base[i] >= 0 else set()), "point %d" % i
        for rider, res in alone.items():
            assert data == res[i][0], "point %d: codestream with %s alone" % (i, rider)
            assert qbits(q, ms=False) == qbits(res[i][1], ms=False), "point %d: %s" % (i, rider)
        assert qbits(q) == qbits(alone["msssim"][i][1]), "point %d: ms_ssim / cs" % i
        for key in report_keys:
            if key == "ab" and base[i] < 0:
                continue
            a, b = q[key], alone[key][i][1][key]
            arrays = [k for k in a if isinstance(a[k], np.ndarray)]
            assert sweep_cases.same(arrays)(a, b), "point %d: %s" % (i, key)
            assert all(a[k] == b[k] for k in a if k not in arrays), "point %d: %s" % (i, key)
        assert _same_summary(q["trace"], alone["trace"][i][1]["trace"]), "point %d: trace" % i
        assert _same_summary(q["trace"], _one(jxg, "natural", img, pts[i])[1])


# ---------------------------------------------------------------------------
# 5. the context afterwards
# ---------------------------------------------------------------------------
def _same_trace(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray) and a[k].dtype == np.float32:
            if not np.array_equal(u32(a[k]), u32(b[k])):
                return False
        elif isinstance(a[k], np.ndarray):
            if not np.array_equal(a[k], b[k]):
                return False
        elif a[k] != b[k]:
            return False
    return True


def test_the_context_after_a_traced_sweep(jxg_mod):
    jxg = jxg_mod
    lib = jxg.load()
    img = sweep_cases.natural()
    large = gradient(512, 512)
    p = sweep_cases.points(jxg)[2]  # d1 e7, both hooks
    pts = sweep_cases.points(jxg)[:4]
    with jxg.Encoder(**p) as fresh:
        want_data = fresh.encode_traced(img)
        want = fresh.search_trace(maps=True)
    with jxg.Encoder(**p) as enc:
        before = enc.encode(img)
        assert before == want_data
        frames = [np.array(img), np.array(img)[::-1].copy()]
        batch_before = enc.encode_batch(frames)
        # the context is lane 0 of its sweeps: a larger frame first, then this one
        enc.sweep(large, [dict(distance=1.0, effort=8, proposals=0, flags=p["flags"])],
                  quality=None, trace=True)
        on = enc.sweep(img, pts, quality=None, trace=True)
        with pytest.raises(jxg.JxgError):
            enc.search_trace(maps=False)
        s = jxg._TraceSummary()
        assert lib.jxg_search_trace(enc._ctx, None, ctypes.byref(s)) == INVALID_ARG
        assert enc.encode_traced(img) == want_data
        assert _same_trace(enc.search_trace(maps=True), want)
        assert enc.encode(img) == before
        # switch off after on: the same codestreams, and no summaries to fetch
        off = enc.sweep(img, pts, quality=None)
        assert [d for d, _ in off] == [d for d, _ in on]
        assert all(q is None for _, q in off)
        out = poisoned(jxg._TraceSummary, len(pts))
        assert lib.jxg_sweep_trace(enc._ctx, out, len(pts)) == INVALID_ARG
        assert bytes(out) == b"\xa5" * ctypes.sizeof(out)
        # a batch with the switch left on is a plain batch
        assert lib.jxg_set_sweep_trace(enc._ctx, 1) == 0
        try:
            assert enc.encode_batch(frames) == batch_before
        finally:
            assert lib.jxg_set_sweep_trace(enc._ctx, 0) == 0
        assert enc.encode_batch(frames) == batch_before


# ---------------------------------------------------------------------------
# 6. refusals through the raw ABI
# ---------------------------------------------------------------------------
def test_refusals_through_the_abi(jxg_mod):
    jxg = jxg_mod
    lib = jxg.load()
    good = sweep_cases.points(jxg)[2]
    img = sweep_cases.natural()
    with jxg.Encoder() as enc:
        ctx = enc._ctx
        run = sweep_cases.RefusedAndGood(jxg, enc, good)
        assert lib.jxg_set_sweep_trace(ctx, 1) == 0
        for quality in (0, 2):
            ret, datas = run(quality)
            assert ret == INVALID_ARG and list(run.st) == [INVALID_ARG, 0]
            assert datas[0] is None and datas[1] == _one(jxg, "natural", img, good)[0]
            out = poisoned(jxg._TraceSummary, 2)
            assert lib.jxg_sweep_trace(ctx, out, 2) == 0
            assert bytes(out[0]) == bytes(ctypes.sizeof(out[0])), "a refused point is zero-filled"
            assert _same_summary(out[1].as_dict(), _one(jxg, "natural", img, good)[1])

            def untouched(*args):
                arr = poisoned(jxg._TraceSummary, 3)
                assert lib.jxg_sweep_trace(*[arr if a is Ellipsis else a for a in args]) == INVALID_ARG
                return bytes(arr) == b"\xa5" * ctypes.sizeof(arr)

            assert untouched(ctx, ..., 1) and untouched(ctx, ..., 3), "a wrong n"
            assert lib.jxg_sweep_trace(ctx, None, 2) == INVALID_ARG
        enc.submit(img)
        try:
            assert untouched(ctx, ..., 2), "a streamed frame is pending"
            for on in (0, 1):
                assert lib.jxg_set_sweep_trace(ctx, on) == INVALID_ARG
        finally:
            enc.receive()
        out = poisoned(jxg._TraceSummary, 2)
        assert lib.jxg_sweep_trace(ctx, out, 2) == 0 and out[1].blocks == 25 * 17
        assert lib.jxg_set_sweep_trace(ctx, 0) == 0


# ---------------------------------------------------------------------------
# 7. the device variant
# ---------------------------------------------------------------------------
def test_device_variant_with_a_padded_stride(jxg_mod):
    import torch

    jxg = jxg_mod
    img = sweep_cases.natural()
    h, w = img.shape[:2]
    stride = 3 * w + 5
    buf = torch.full((h, stride), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:, :3 * w] = torch.from_numpy(np.array(img).reshape(h, 3 * w)).cuda()
    torch.cuda.synchronize()
    pts = _eight(jxg)
    with jxg.Encoder() as enc:
        got = enc.sweep_device(buf.data_ptr(), w, h, pts, quality="psnr", row_stride=stride,
                               trace=True)
    _check_points(jxg, got, "natural", img, pts)
    assert bool((buf[:, 3 * w:] == 0xA5).all())
